"""rgx_table_merge_device (merge_kernels.hip: k_merge_unpack, k_merge_heads, k_merge_reduce, k_merge_strand, k_merge_rank, k_merge_table, with the
radix sorts and the scan between them) on parts no extraction leaves behind, against the restatement of the merge contract in tests/merge_ref.py:
every column of the result -- tid, start, end, thick_start, thick_end, read_count, name_index, strand, left_ok, right_ok -- in row order, and the
BED12 text against the host merge's.  The parts are ragged and empty, lie in HBM with a stride and plausible rows in the slack behind
part_rows[g], number up to 255, share one key or all keys or none, differ in one field of the key, and name their contigs so that string order
is not tid order.  Everything is integers: every comparison is ==.

That these tests can fail was shown once, on scratch builds with one-line faults that change values, not addresses:
  * atomicMin on u.first in k_merge_reduce as atomicMax (every key keeps the fill value, the names follow the key order):
    test_device_merge_equals_the_restatement_in_every_column fails for both one_field cases, N256, N257, N513, every_key_in_every_part,
    two_parts_min_anchor_0 and the 255 mixed parts, and test_refusals_come_before_any_launch_and_leave_the_context_usable fails (9 tests);
    N1 and the one key in 255 parts have one name to give and pass.
  * k_merge_unpack ignoring part_rows[g] was NOT run (the slack rows would be written behind the N rows the columns are carved for).
    Restated on a CPU -- the slack rows merged as if they were rows -- every case gains rows (N1: 4 for 1; the 255 mixed parts: 2513 for 2000;
    a count of 999999 shows in each), so every case of test_device_merge_equals_the_restatement_in_every_column would fail.
"""
import ctypes as C

import numpy as np
import pytest

import merge_ref as mref

pytestmark = pytest.mark.gpu

CASES = mref.all_cases()
RGX_ERR_ARG = 7


def _upload(case):
    import torch
    buf = torch.from_numpy(case.buffer().view(np.int32).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()            # the context's stream does not wait for torch's
    return buf


def _device_merge(gpu_ctx, case, proto):
    from regtools_amd import distributed
    buf = _upload(case)
    assert buf.numel() == len(case.parts) * case.stride * 12
    dev = distributed.merge_device(gpu_ctx, buf.data_ptr(), case.stride, case.part_rows, C.byref(proto), case.min_anchor)
    assert np.array_equal(buf.cpu().numpy().view(np.uint32).reshape(-1, 12), case.buffer())        # the caller's rows are read, never written
    return dev


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_device_merge_equals_the_restatement_in_every_column(gpu_ctx, case):
    from regtools_amd import distributed
    proto, keep = mref.names_table(case.names)
    want = mref.merge(case.parts, case.names, case.min_anchor)
    dev = _device_merge(gpu_ctx, case, proto)
    got = mref.table_columns(dev.table)
    print("%s: %d parts, %d rows, %d unique" % (case.name, len(case.parts), case.N, dev.n))
    assert dev.n == len(want["tid"]) == len(case.keys())
    for col in mref.COLS:
        assert got[col] == want[col], (case.name, col)
    assert 999999 not in got["read_count"]                       # no slack row shows
    host = distributed.merge_packed(case.packed_parts(), C.byref(proto), case.min_anchor)
    assert dev.bed12(False) == host.bed12(False) and dev.bed12() == host.bed12()


def test_refusals_come_before_any_launch_and_leave_the_context_usable(gpu_ctx):
    from regtools_amd import _ffi
    L = _ffi.lib()
    case = [c for c in CASES if c.name == "every_key_in_every_part"][0]
    proto, keep = mref.names_table(case.names)
    want = mref.merge(case.parts, case.names, case.min_anchor)
    buf = _upload(case)

    def call(stride, part_rows, n_parts):
        out = C.POINTER(_ffi.JunctionTable)()
        err = C.create_string_buffer(256)
        sizes = (C.c_uint64 * max(1, len(part_rows)))(*part_rows)
        rc = L.rgx_table_merge_device(gpu_ctx._h, C.c_void_p(buf.data_ptr()), stride, sizes, n_parts, case.min_anchor, C.byref(proto), C.byref(out), err, len(err))
        return rc, out

    refusals = [(case.stride, [64, case.stride + 1, 64], 3),                # part_rows[g] > stride
                (1 << 24, [64, 1 << 24, 64], 3),                            # part_rows[g] >= 2^24
                (case.stride, [], 0),                                       # no parts
                (case.stride, [1] * 256, 256)]                              # one part too many
    for stride, part_rows, n_parts in refusals:
        rc, out = call(stride, part_rows, n_parts)
        assert rc == RGX_ERR_ARG and not out, (stride, part_rows[:3], n_parts)
        rc, out = call(case.stride, case.part_rows, len(case.part_rows))    # a good merge follows each refusal
        assert rc == 0
        got = mref.table_columns(out)
        L.rgx_table_free(out)
        assert all(got[col] == want[col] for col in mref.COLS)
