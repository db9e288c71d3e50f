"""BGZF member discovery on the device (members_kernels.hip: k_magic_count, k_magic_fill, k_member_link, k_member_jump, k_member_compact, k_member_fix,
k_member_upos, k_member_query, k_member_stop, driven by MemberDiscovery as EventsRun::stage_members drives it) through the stage entry
rgx_k_members, against the serial restatement of tests/members_ref.py: every output -- the candidate offsets, the member list (cpos, upos, clen,
isize), the counts, the inflated total, the three queries and the stop -- compared with == on integers.  The files are the ones no compressor
writes: member starts and decoy headers at every offset of the 4 KiB magic tile and of a thread's 16 bytes, two candidates in one thread's 16
bytes, a file cut at every length around the 34-byte end of the fast path, chains of 2^k and 2^k + 1 members, broken and foreign links, second
chain roots, more than 2048 members and more than 2^32 inflated bytes.  A cut file is uploaded WHOLE and only bam_len is cut, so the bytes behind
bam_len are the headers and footers a kernel that ignored the length would find.

That these tests can fail was shown once, on scratch builds with one-line faults that change values, not addresses:
  * the prefilter loop of magic_mask16 as `k < 15` (a header in a thread's last byte is missed on the fast path): both tile tests, the
    two-in-one-thread test, the cut-file test, test_chains_of_powers_of_two_and_one_more from 255 members on, both broken-link tests, the decoy
    and the one-context tests, all of test_upos_*, and the query test fail (25 tests; the chains of 1 to 5 members put no header there).
  * `carry` of k_member_upos as uint32_t: test_upos_carries_past_two_to_the_32 fails, and nothing else (1 test).
  * `reach[i]` of k_member_link without its `off == root2` term: both test_bsize_one_short_or_one_long_and_the_second_root_behind_it,
    test_decoy_that_links_into_the_real_chain and test_one_context_keeps_nothing_between_calls fail (4 tests).
  * one jump round fewer in chain() SURVIVES, on the GPU (41 passed) as on paper: round r hands `reach` on by 2^r links, so the
    ceil(log2 n) rounds of the loop already reach chain positions 0 .. 2^ceil(log2 n) - 1 >= n - 1 and the round behind the loop is spare.
    Two rounds fewer was not run; restated on a CPU with the rounds taken one after the other (the kernel's race can only reach further),
    the member list comes out short for every chain of test_chains_of_powers_of_two_and_one_more from 2 members on in its decoy-free half
    (the candidates are then the chain), and for none of the decoy files, whose candidate count is twice the chain.
"""
import ctypes as C

import numpy as np
import pytest

import members_ref as mr

pytestmark = pytest.mark.gpu

ERRLEN = 512


def _run(gpu_ctx, data, bam_len=None, root2=mr.NONE, true_sizes=None, q=(0, 0, 0)):
    """rgx_k_members on data[:bam_len] (all of data, and 64 bytes more, lie in HBM) -> the dict members_ref.discover returns."""
    import torch
    from regtools_amd import _ffi
    L = _ffi.lib()
    bam_len = len(data) if bam_len is None else bam_len
    d = torch.from_numpy(np.frombuffer(bytes(data) + mr.FIXED * 4, dtype=np.uint8).copy()).cuda()
    d_sizes = None
    if true_sizes is not None:
        d_sizes = torch.from_numpy(np.asarray(true_sizes, dtype=np.uint32).view(np.int32).copy()).cuda()
    torch.cuda.synchronize()                    # the context's stream does not wait for torch's
    out = C.POINTER(_ffi.MembersResult)()
    err = C.create_string_buffer(ERRLEN)
    qq = (C.c_uint64 * 3)(*q)
    rc = L.rgx_k_members(gpu_ctx._h, d.data_ptr(), bam_len, root2, d_sizes.data_ptr() if d_sizes is not None else None, qq, C.byref(out), err, ERRLEN)
    assert rc == 0, err.value
    r = out.contents
    nc, nm = int(r.n_candidates), int(r.n_members)
    cand = np.ctypeslib.as_array(r.candidates, shape=(max(nc, 1),))[:nc].copy()
    mem = np.zeros((nm, 4), dtype=np.uint64)
    if nm:
        raw = np.ctypeslib.as_array(C.cast(r.members, C.POINTER(C.c_uint8)), shape=(nm * 24,)).copy()
        mem[:, 0] = raw.view(np.uint64).reshape(nm, 3)[:, 0]
        mem[:, 1] = raw.view(np.uint64).reshape(nm, 3)[:, 1]
        mem[:, 2] = raw.view(np.uint32).reshape(nm, 6)[:, 4]
        mem[:, 3] = raw.view(np.uint32).reshape(nm, 6)[:, 5]
    got = {"candidates": cand, "members": mem, "total": int(r.total_inflated), "q_index": list(r.q_index), "q_upos": list(r.q_upos),
           "stop": int(r.stop)}
    L.rgx_members_result_free(out)
    return got


def _check(gpu_ctx, data, bam_len=None, root2=mr.NONE, true_sizes=None, q=(0, 0, 0), what=None):
    bam_len = len(data) if bam_len is None else bam_len
    want = mr.discover(data[:bam_len], root2, true_sizes, q)
    got = _run(gpu_ctx, data, bam_len, root2, true_sizes, q)
    what = (what, bam_len, root2, q)
    assert np.array_equal(got["candidates"], np.array(want["candidates"], dtype=np.uint64)), what
    assert got["members"].shape[0] == len(want["members"]), (what, got["members"].shape[0], len(want["members"]))
    wm = mr.members_array(want["members"])
    for col, name in enumerate(("cpos", "upos", "clen", "isize")):
        bad = np.nonzero(got["members"][:, col] != wm[:, col])[0]
        assert bad.size == 0, (what, name, "first at member", int(bad[0]), int(got["members"][bad[0], col]), int(wm[bad[0], col]))
    assert got["total"] == want["total"], what
    assert got["q_index"] == want["q_index"] and got["q_upos"] == want["q_upos"], (what, got["q_index"], want["q_index"])
    assert got["stop"] == want["stop"], (what, got["stop"], want["stop"])
    return want


# ---- the magic tile -----------------------------------------------------------------------------------------------------------------
def test_member_starts_at_every_offset_of_the_tile(gpu_ctx):
    want = _check(gpu_ctx, mr.plain_run(4200), what="33-byte members")
    assert {o % 4096 for o in want["candidates"]} == set(range(4096)) and len(want["members"]) == 4200


def test_decoys_at_every_offset_of_the_tile(gpu_ctx):
    want = _check(gpu_ctx, mr.decoy_run(4200), what="51-byte members with decoys")
    starts = {m[0] - 18 for m in want["members"]}
    decoys = {o for o in want["candidates"] if o not in starts}
    assert {o % 4096 for o in starts} == set(range(4096)) == {o % 4096 for o in decoys}


def test_two_candidates_in_one_threads_sixteen_bytes(gpu_ctx):
    data, ks = mr.two_in_one_thread()
    want = _check(gpu_ctx, data, what="two in one thread")
    starts = {m[0] - 18 for m in want["members"]}
    assert sorted(k % 16 for k in ks) == list(range(16))
    assert all(k in want["candidates"] and k + 6 in want["candidates"] and k not in starts and k + 6 not in starts for k in ks)


# ---- the end of the file ------------------------------------------------------------------------------------------------------------
def test_file_cut_at_every_length_near_its_end(gpu_ctx):
    data = mr.small_file()
    n = len(data)
    last = mr.candidates(data)[-1]
    assert n - 64 <= last + 17 and last + 18 <= n            # a final header with exactly 17 and 18 bytes left is among the cuts
    for cut in [0, 1, 17, 18, 27, 28] + list(range(n - 64, n + 1)):
        want = _check(gpu_ctx, data, bam_len=cut, q=(0, max(cut, 28) - 28, cut), what="cut")
        if cut < 18:
            assert want["candidates"] == [] and want["members"] == [] and want["q_index"] == [0, 0, 0] and want["stop"] == 0xffffffff


# ---- chain lengths against the jump rounds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mr.CHAIN_LENGTHS)
def test_chains_of_powers_of_two_and_one_more(gpu_ctx, n):
    for data, n_cand in ((mr.decoy_run(n), 2 * n), (mr.plain_run(n), n)):       # (without decoys the candidates ARE the chain: the fewest rounds)
        want = _check(gpu_ctx, data, q=(0, len(data) - len(data) // n, 0), what="chain of %d" % n)
        assert len(want["candidates"]) == n_cand and len(want["members"]) == n
        assert want["q_index"][1] == n - 1                                      # the last member is in the list


# ---- broken and foreign links -------------------------------------------------------------------------------------------------------
N_LINKS, MID = 40, 20


@pytest.mark.parametrize("delta", [-1, 1])
def test_bsize_one_short_or_one_long_and_the_second_root_behind_it(gpu_ctx, delta):
    data = mr.decoy_run(N_LINKS, blen_delta={MID: delta})
    want = _check(gpu_ctx, data, what="broken link")
    assert len(want["members"]) == MID + 1
    want = _check(gpu_ctx, data, root2=51 * (MID + 1), q=(51 * (MID + 1), 51 * MID, 51 * (N_LINKS - 1)), what="two segments in one list")
    assert len(want["members"]) == N_LINKS and want["q_index"] == [MID + 1, MID, N_LINKS - 1]


def test_decoy_that_links_into_the_real_chain(gpu_ctx):
    data = mr.decoy_run(N_LINKS, land_on_next={10})
    d10 = 51 * 10 + mr.DATA_AT
    want = _check(gpu_ctx, data, q=(d10, 51 * 11, 0), what="foreign link, no second root")
    assert len(want["members"]) == N_LINKS and want["q_index"][0] == N_LINKS           # not reached from offset 0
    want = _check(gpu_ctx, data, root2=d10, q=(d10, 51 * 11, 0), what="second root on the decoy")
    assert len(want["members"]) == N_LINKS + 1 and want["q_index"][:2] == [11, 12]      # the decoy is listed
    plain = mr.discover(data)["members"]
    for root2 in (0, 7, 51 * 5, len(data), mr.NONE - 64):                                # offset 0, no candidate, a member already reached
        assert _check(gpu_ctx, data, root2=root2, what="second root that adds nothing")["members"] == plain


def test_one_context_keeps_nothing_between_calls(gpu_ctx):
    data = mr.decoy_run(N_LINKS, land_on_next={10}, blen_delta={MID: -1})
    d10 = 51 * 10 + mr.DATA_AT
    a = _check(gpu_ctx, data, what="plain")
    b = _check(gpu_ctx, data, root2=51 * (MID + 1), what="second root")
    c = _check(gpu_ctx, data, root2=d10, what="second root on a decoy")
    d = _check(gpu_ctx, data, what="plain again")
    assert a == d and len(a["members"]) == MID + 1 and len(b["members"]) == N_LINKS and len(c["members"]) == MID + 2
    big = mr.decoy_run(40000)
    assert len(big) > 2000000
    _check(gpu_ctx, big, root2=51 * 777 + mr.DATA_AT, q=(51 * 39999, 0, 0), what="2 MB")
    small = mr.member(b"ab") + mr.member(b"ab") + mr.member(b"abc")
    assert len(small) == 100
    want = _check(gpu_ctx, small, q=(66, 33, 0), what="100 bytes behind 2 MB")
    assert len(want["members"]) == 3 == len(want["candidates"])


# ---- upos ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mr.UPOS_LENGTHS)
def test_upos_across_the_trips_of_2048_members(gpu_ctx, n):
    data = mr.plain_run(n, mr.drawn_footers(n, n))
    want = _check(gpu_ctx, data, q=(33 * (n - 1), 33 * 2047 if n > 2047 else 0, 0), what="drawn footers")
    assert len(want["members"]) == n
    _check(gpu_ctx, data, true_sizes=mr.drawn_true_sizes(n, n + 1), q=(33 * (n - 1), 0, 0), what="drawn footers, true sizes")


def test_upos_carries_past_two_to_the_32(gpu_ctx):
    data = mr.plain_run(mr.BIG_N, np.full(mr.BIG_N, 65536))
    want = _check(gpu_ctx, data, q=(33 * (mr.BIG_N - 1), 33 * 65536, 33 * 65535), what="70,000 members of 65536")
    assert want["total"] == mr.BIG_TOTAL > 1 << 32 and want["q_upos"] == [65536 * (mr.BIG_N - 1), 1 << 32, (1 << 32) - 65536]
    _check(gpu_ctx, data, true_sizes=mr.drawn_true_sizes(mr.BIG_N, 5), q=(33 * (mr.BIG_N - 1), 0, 0), what="70,000 members, true sizes")
    _check(gpu_ctx, data, true_sizes=np.full(mr.BIG_N, 65536), q=(33 * (mr.BIG_N - 1), 0, 0), what="70,000 members, true sizes of 65536")


# ---- query and stop -----------------------------------------------------------------------------------------------------------------
def test_queries_hit_and_miss_and_the_stop_rule(gpu_ctx):
    n = 64
    f = np.full(n, 100)
    f[[10, 40]] = [0, 70000]
    data = mr.decoy_run(n, f)
    at = lambda k: 51 * k
    want = _check(gpu_ctx, data, q=(at(0), at(n - 1), at(31)), what="hits: first, last, middle")
    assert want["q_index"] == [0, n - 1, 31] and want["stop"] == 10
    want = _check(gpu_ctx, data, q=(at(31) + 1, at(31) + mr.DATA_AT, len(data)), what="misses: between members, a decoy, behind the file")
    assert want["q_index"] == [n, n, n] and want["stop"] == 0xffffffff                 # q_index[0] a miss: no stop
    want = _check(gpu_ctx, data, q=(mr.NONE - 64, at(5), mr.NONE - 64), what="miss at UINT64_MAX - 64")
    assert want["q_index"] == [n, 5, n]
    stops = [_check(gpu_ctx, data, q=(at(k), 0, 0), what="stop")["stop"] for k in (0, 10, 11, 39, 40, 41, n - 1)]
    assert stops == [10, 10, 40, 40, 40, 0xffffffff, 0xffffffff]       # in front of `from`, exactly at it, behind it, none
    clean = mr.decoy_run(n, np.full(n, 65536))
    assert _check(gpu_ctx, clean, q=(0, 0, 0), what="no stop at all")["stop"] == 0xffffffff
