"""The kernels behind the DEFLATE launch, each on its own against numpy (tests/stage_ref.py): the exclusive scan (launch_scan_u32), the radix sort
(launch_radix_pass / launch_radix_pass_keyed through RadixSort, driven the three ways the product drives it) and the group-by (reduce_events:
k_preagg, k_heads, k_reduce / k_reduce_partials, k_reduce_finish*, k_name_rank, the output-order sort), through the stage entry points
rgx_k_scan_u32 / rgx_k_radix_sort / rgx_k_group_by.  The shapes are the ones a BAM reaches only by luck: sizes on and around the scan tile (4096) and
the radix tiles (512 keys up to 2,097,152, 2048 above), the second loop trips of k_scan_tiles (> 256 tiles) and k_radix_offsets (> 2048 tiles),
last passes of 1 to 7 bits, k_preagg tiles of 1024 distinct keys and of 1024 keys that share one slot of its table, keys whose events lie in tiles
far apart.  Everything is integers: every comparison is np.array_equal.

That these tests can fail was shown once, on scratch builds with one-line faults:
  * the radix mask always 0xff (a pass's `bits` ignored): test_radix_one_word_small fails for every n >= 63 at 1, 5, 9, 13 and 21 bits,
    test_radix_one_word_large at 1, 5, 9, 13 and 21 bits, test_radix_as_the_{group_by,output_order,merge}_sorts and both
    test_radix_second_sort_of_fewer_keys_in_the_same_scratch (41 tests).  The group-by tests cannot see it: their words carry nothing above nbits.
  * `first` combined as a max in k_reduce_partials: test_group_by_sizes_and_shapes[one_key and runs from 1025 events on], all of
    test_group_by_group_counts, ..._two_groups_share_a_rank, both ..._one_key_in_tiles_far_apart, the three twice_across cases of
    ..._keys_that_share_one_slot_of_the_tile_table, all of ..._keys_that_differ_in_one_word and ..._strand_byte_is_the_last_events (28 tests).
  * k_preagg's probe step without its wrap at 2048 slots was NOT run (it would leave the LDS table); restated on a CPU, 1023 probes of the tile
    step from slot 2047 to slot 0 in each slot-2047 case of ..._keys_that_share_one_slot_of_the_tile_table (none in the slot-0 and slot-1000
    cases), and 71 probes in 46 tiles of test_group_by_sizes_and_shapes[300000-distinct]."""
import ctypes as C

import numpy as np
import pytest

import stage_ref

pytestmark = pytest.mark.gpu

ERRLEN = 512


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _empty(n):
    import torch
    return torch.empty(int(n), dtype=torch.int32, device="cuda")


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _sync():
    import torch
    torch.cuda.synchronize()        # the context's stream does not wait for torch's


def bitlen(v):
    return int(v).bit_length()


# ---- scan ---------------------------------------------------------------------------------------------------------------------------
SCAN_N = [0, 1, 15, 16, 17, 4095, 4096, 4097, 1048576, 1048577, 3145733]       # 1,048,577: the first n with a second trip of k_scan_tiles


def _scan_values(kind, n, rng):
    if kind == "ones":
        return np.ones(n, dtype=np.uint32)
    if kind == "random":
        return rng.integers(0, 4, n, dtype=np.uint32)
    a = np.zeros(n, dtype=np.uint32)
    if n:
        a[n // 3] = 0xfffffff0
    return a


@pytest.mark.parametrize("kind", ["ones", "random", "single"])
@pytest.mark.parametrize("n", SCAN_N)
def test_scan_equals_cumsum(gpu_ctx, n, kind):
    from regtools_amd import _ffi
    L = _ffi.lib()
    a = _scan_values(kind, n, np.random.default_rng(1000 + n))
    exp, exp_total = stage_ref.excl_scan(a)
    assert exp_total < 1 << 32
    exp = exp.astype(np.uint32)
    err = C.create_string_buffer(ERRLEN)
    for in_place in (False, True):
        for with_total in (False, True):
            d_in = _dev(a)
            d_out = d_in if in_place else _dev(np.full(n, 0xdeadbeef, dtype=np.uint32))
            d_total = _dev(np.array([0xdeadbeef], dtype=np.uint32))
            _sync()
            rc = L.rgx_k_scan_u32(gpu_ctx._h, d_in.data_ptr(), d_out.data_ptr(), n, d_total.data_ptr() if with_total else None, err, ERRLEN)
            assert rc == 0, err.value
            assert np.array_equal(_host(d_out), exp), (n, kind, in_place, with_total)
            if not in_place:
                assert np.array_equal(_host(d_in), a)
            assert int(_host(d_total)[0]) == (exp_total if with_total else 0xdeadbeef), (n, kind, in_place, with_total)


# ---- radix sort ---------------------------------------------------------------------------------------------------------------------
def _sort(gpu_ctx, words, nbits, mode, n_scratch=0):
    from regtools_amd import _ffi
    L = _ffi.lib()
    n = len(words[0])
    d_words = [_dev(w) for w in words]
    d_perm = _dev(np.full(n, 0xdeadbeef, dtype=np.uint32))
    ptrs = (C.c_void_p * len(words))(*[t.data_ptr() for t in d_words])
    bits = (C.c_uint32 * len(words))(*nbits)
    err = C.create_string_buffer(ERRLEN)
    _sync()
    rc = L.rgx_k_radix_sort(gpu_ctx._h, n, n_scratch, len(words), ptrs, bits, mode, d_perm.data_ptr(), err, ERRLEN)
    assert rc == 0, err.value
    for w, t in zip(words, d_words):
        assert np.array_equal(_host(t), w)                  # the caller's columns are read, never written
    return _host(d_perm)


def _check_sort(gpu_ctx, words, nbits, n_scratch=0, what=None):
    exp = stage_ref.stable_sort(words, nbits)
    for mode in (0, 1, 2):                                  # RadixSort::by, ::by_keyed, ::by_gathered: one permutation, the reference's
        got = _sort(gpu_ctx, words, nbits, mode, n_scratch)
        assert np.array_equal(got, exp), (what, len(words[0]), nbits, mode)


NBITS = [1, 5, 8, 9, 13, 16, 21, 32]
SMALL_N = [0, 1, 63, 64, 65, 511, 512, 513]
# 1,048,576 = 2048 small tiles, the last size before k_radix_offsets loops; 2,097,152 = kRadixSmallMax, 2,097,153 the first size on large tiles;
# 4,194,305 = 2049 large tiles.  Two widths each (the host's sort is most of their time); between them every last pass of 1, 5, 8 bits and more.
LARGE_N_BITS = [(1048576, 8), (1048576, 21), (1048577, 13), (1048577, 32), (2097152, 5), (2097152, 16), (2097153, 9), (2097153, 32),
                (4194305, 1), (4194305, 21)]


@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("n", SMALL_N)
def test_radix_one_word_small(gpu_ctx, n, nbits):
    w = np.random.default_rng(n * 64 + nbits).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)      # junk above nbits
    _check_sort(gpu_ctx, [w], [nbits])


@pytest.mark.parametrize("n,nbits", LARGE_N_BITS)
def test_radix_one_word_large(gpu_ctx, n, nbits):
    w = np.random.default_rng(n + nbits).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    _check_sort(gpu_ctx, [w], [nbits])


def _distribution(kind, n, rng):
    i = np.arange(n, dtype=np.uint64)
    if kind == "uniform":
        w = rng.integers(0, 1 << 16, n, dtype=np.uint64)
    elif kind == "all_equal":
        w = np.full(n, 0x5a5a, dtype=np.uint64)
    elif kind == "sorted":
        w = i * np.uint64(65535) // np.uint64(max(n - 1, 1))
    elif kind == "reversed":
        w = np.uint64(65535) - i * np.uint64(65535) // np.uint64(max(n - 1, 1))
    elif kind == "alternating":                             # neighbouring lanes never share a digit, every other lane does
        w = np.where(i & np.uint64(1), np.uint64(0x01fe), np.uint64(0xfe01))
    elif kind == "digits_0_255":
        w = rng.integers(0, 2, n, dtype=np.uint64) * np.uint64(0xff) | rng.integers(0, 2, n, dtype=np.uint64) * np.uint64(0xff00)
    else:                                                   # one_odd: each run of 64 keys holds one other key among 63 equal ones
        w = np.full(n, 0x1234, dtype=np.uint64)
        t = np.arange(0, n, 64, dtype=np.uint64)
        at = t + (t // np.uint64(64) * np.uint64(7)) % np.uint64(64)
        w[at[at < n]] = 0x4321
    return (w | rng.integers(0, 1 << 16, n, dtype=np.uint64) << np.uint64(16)).astype(np.uint32)       # junk above the 16 bits sorted on


@pytest.mark.parametrize("kind", ["uniform", "all_equal", "sorted", "reversed", "alternating", "digits_0_255", "one_odd"])
@pytest.mark.parametrize("n", [70001, 2097153])
def test_radix_distributions(gpu_ctx, n, kind):
    _check_sort(gpu_ctx, [_distribution(kind, n, np.random.default_rng(n + len(kind)))], [16], what=kind)


def _few(rng, n, distinct, bits=32):
    """a column of `distinct` different values: ties in every word, so that stability and the order of the words show"""
    return rng.integers(0, 1 << bits, distinct, dtype=np.uint64)[rng.integers(0, distinct, n)].astype(np.uint32)


def test_radix_as_the_group_by_sorts(gpu_ctx):
    """reduce_events: (ilen_cls 21 bits, start 32, tid 13) -- 8 + 8 + 5, four times 8, 8 + 5 bits"""
    rng = np.random.default_rng(31)
    n = 70001
    _check_sort(gpu_ctx, [_few(rng, n, 40), _few(rng, n, 300), _few(rng, n, 25)], [21, 32, 13])


def test_radix_as_the_output_order_sorts(gpu_ctx):
    """reduce_events' order sort: (name rank bitlen(n) bits, thick_end 32, thick_start 32, contig rank 5)"""
    rng = np.random.default_rng(32)
    n = 70001
    name_rank = (rng.permutation(n) + 1).astype(np.uint32)
    _check_sort(gpu_ctx, [name_rank, _few(rng, n, 50), _few(rng, n, 50), _few(rng, n, 25)], [bitlen(n), 32, 32, 5])


def test_radix_as_the_merge_sorts(gpu_ctx):
    """rgx_table_merge_device: (strand class 2 bits, end 32, start 32, tid 5)"""
    rng = np.random.default_rng(33)
    n = 70001
    _check_sort(gpu_ctx, [_few(rng, n, 3), _few(rng, n, 200), _few(rng, n, 200), _few(rng, n, 25)], [2, 32, 32, 5])


@pytest.mark.parametrize("n_first,n_second", [(70001, 5000), (2097153, 1000000)])
def test_radix_second_sort_of_fewer_keys_in_the_same_scratch(gpu_ctx, n_first, n_second):
    """The merge sorts its unique rows in the scratch carved for all its rows (rows.reset()): a sort of fewer keys must fit the scratch of more -- also
    across the tile switch, where the fewer keys (small tiles) need four times the histogram words per key."""
    rng = np.random.default_rng(n_first)
    a = rng.integers(0, 1 << 32, n_first, dtype=np.uint64).astype(np.uint32)
    _check_sort(gpu_ctx, [a], [32])
    b = rng.integers(0, 1 << 32, n_second, dtype=np.uint64).astype(np.uint32)
    _check_sort(gpu_ctx, [b, _few(rng, n_second, 7)], [32, 3], n_scratch=n_first)


# ---- group-by -----------------------------------------------------------------------------------------------------------------------
def _events(tid, start, ilen_cls, rng, strand=None):
    """thick bounds and strand bytes for the key columns: thick_start <= start, thick_end >= end, the byte a strand class prints as"""
    tid, start, ilen_cls = [np.asarray(a, dtype=np.uint32) for a in (tid, start, ilen_cls)]
    n = len(tid)
    ts = start - rng.integers(0, 200, n, dtype=np.uint32)
    te = start + (ilen_cls >> np.uint32(2)) + rng.integers(0, 200, n, dtype=np.uint32)
    if strand is None:
        strand = np.array([ord("+"), ord("-"), ord("?"), ord("?")], dtype=np.uint8)[ilen_cls & np.uint32(3)]
    return dict(tid=tid, start=start, ilen_cls=ilen_cls, ts=ts, te=te, strand=np.asarray(strand, dtype=np.uint8))


def _random_keys(rng, m, n_groups, ilen_bits):
    """m DISTINCT keys (the starts differ)"""
    start = (1000 + rng.permutation(m).astype(np.uint64) * 7).astype(np.uint32)
    max_len = 500000 if ilen_bits == 21 else (1 << 29)
    ilen_cls = rng.integers(70, max_len + 1, m, dtype=np.uint32) << np.uint32(2) | rng.integers(0, 3, m, dtype=np.uint32)
    return rng.integers(0, n_groups, m, dtype=np.uint32), start, ilen_cls


def _group_by(gpu_ctx, ev, n_groups, rank, ilen_bits, form):
    from regtools_amd import _ffi
    L = _ffi.lib()
    n = len(ev["tid"])
    d = {k: _dev(v) for k, v in ev.items()}
    d_rows = _dev(np.full(10 * n, 0xdeadbeef, dtype=np.uint32))
    d_urow, d_pos = _dev(np.full(n, 0xdeadbeef, dtype=np.uint32)), _dev(np.full(n, 0xdeadbeef, dtype=np.uint32))
    rank_c = (C.c_uint32 * n_groups)(*[int(r) for r in rank])
    n_rows = C.c_uint64(0)
    err = C.create_string_buffer(ERRLEN)
    _sync()
    rc = L.rgx_k_group_by(gpu_ctx._h, d["tid"].data_ptr(), d["start"].data_ptr(), d["ilen_cls"].data_ptr(), d["ts"].data_ptr(), d["te"].data_ptr(),
                          d["strand"].data_ptr(), n, max(1, bitlen(n_groups - 1)), ilen_bits, rank_c, n_groups, form, d_rows.data_ptr(), C.byref(n_rows),
                          d_urow.data_ptr() if form == 2 else None, d_pos.data_ptr() if form == 2 else None, err, ERRLEN)
    assert rc == 0, err.value
    u = int(n_rows.value)
    assert u <= n
    flat = _host(d_rows)
    rows = {k: flat[i * u:(i + 1) * u] for i, k in enumerate(stage_ref.ROW_COLUMNS)}
    return rows, _host(d_urow), _host(d_pos)[:u]


def _check_group_by(gpu_ctx, ev, n_groups, rank, ilen_bits, forms=(0, 1, 2), what=None):
    """all forms give the reference's ten columns; form 2's row map sends every event to the reference's output row.  -> the reference's rows"""
    assert int(ev["tid"].max()) < n_groups and (ilen_bits == 32 or int(ev["ilen_cls"].max()) < 1 << ilen_bits)
    exp, row_of_event = stage_ref.group_by(ev["tid"], ev["start"], ev["ilen_cls"], ev["ts"], ev["te"], ev["strand"], rank)
    for form in forms:
        rows, ev_urow, urow_pos = _group_by(gpu_ctx, ev, n_groups, rank, ilen_bits, form)
        assert len(rows["tid"]) == len(exp["tid"]), (what, form, len(rows["tid"]), len(exp["tid"]))
        for k in stage_ref.ROW_COLUMNS:
            assert np.array_equal(rows[k], exp[k]), (what, form, k)
        if form == 2:
            assert int(ev_urow.max()) < len(urow_pos)
            assert np.array_equal(urow_pos[ev_urow], row_of_event), (what, "row map")
    return exp


GROUPS = [1, 2, 256, 257, 70000]
EVENT_N = [1, 255, 256, 1023, 1024, 1025, 2047, 2049, 4097, 300000]


def _shape(shape, n, n_groups, ilen_bits, rng):
    if shape == "one_key":
        t, s, l = _random_keys(rng, 1, n_groups, ilen_bits)
        pick = np.zeros(n, dtype=np.int64)
    elif shape == "distinct":
        t, s, l = _random_keys(rng, n, n_groups, ilen_bits)
        pick = np.arange(n)
    else:
        # file-like: runs of one key, 1 to 3000 events long (shorter where n is small), the keys drawn from a pool so that some come back tiles later;
        # every third run is cut or stretched to end exactly on an edge of k_preagg's 1024-event tiles, or one event past it
        cap = min(3000, max(2, n // 3))
        t, s, l = _random_keys(rng, max(2, n // 50), n_groups, ilen_bits)
        pick, k = [], 0
        while len(pick) < n:
            run = int(rng.integers(1, cap + 1))
            if k % 3 == 2:
                run = 1024 - len(pick) % 1024 + (k // 3) % 2
            pick += [int(rng.integers(0, len(t)))] * run
            k += 1
        pick = np.array(pick[:n])
    return _events(t[pick], s[pick], l[pick], rng)


@pytest.mark.parametrize("shape", ["one_key", "distinct", "runs"])
@pytest.mark.parametrize("n", EVENT_N)
def test_group_by_sizes_and_shapes(gpu_ctx, n, shape):
    rng = np.random.default_rng(n * 3 + len(shape))
    k = EVENT_N.index(n) + len(shape)
    n_groups, ilen_bits = GROUPS[k % len(GROUPS)], (21, 32)[k % 2]                  # every group count and both widths, spread over the cases
    ev = _shape(shape, n, n_groups, ilen_bits, rng)
    exp = _check_group_by(gpu_ctx, ev, n_groups, rng.permutation(n_groups), ilen_bits, what=(shape, n))
    if shape == "one_key":
        assert len(exp["tid"]) == 1 and exp["count"][0] == n and exp["first_seen"][0] == 0 and exp["last_seen"][0] == n - 1
    if shape == "distinct":
        assert len(exp["tid"]) == n


@pytest.mark.parametrize("ilen_bits", [21, 32])
@pytest.mark.parametrize("n_groups", GROUPS)
def test_group_by_group_counts(gpu_ctx, n_groups, ilen_bits):
    """group_bits 1, 1, 8, 9, 17: the last pass over the tid is 1, 8 or 1 bits wide; the order sort's rank word likewise"""
    rng = np.random.default_rng(n_groups + ilen_bits)
    ev = _shape("runs", 4097, n_groups, ilen_bits, rng)
    d = _shape("distinct", 3000, n_groups, ilen_bits, rng)
    ev = {k: np.concatenate([ev[k], d[k]]) for k in ev}
    _check_group_by(gpu_ctx, ev, n_groups, rng.permutation(n_groups), ilen_bits, what=("groups", n_groups))


def test_group_by_two_groups_share_a_rank(gpu_ctx):
    """contigs of one name (chrom_string_ranks gives them one rank): their rows interleave by thick bounds and name"""
    rng = np.random.default_rng(77)
    n_groups = 6
    rank = np.array([2, 0, 2, 1, 0, 3])
    t, s, l = _random_keys(rng, 400, n_groups, 21)
    pick = rng.integers(0, 400, 5000)
    ev = _events(t[pick], s[pick], l[pick], rng)
    ev["ts"][:] = ev["start"] - rng.integers(0, 3, 5000, dtype=np.uint32)           # many rows with equal thick_start: thick_end and the name decide
    exp = _check_group_by(gpu_ctx, ev, n_groups, rank, 21, what="shared rank")
    assert len(set(exp["tid"][np.array(rank)[exp["tid"]] == 2].tolist())) == 2


def test_group_by_all_distinct_past_the_large_radix_tiles(gpu_ctx):
    """2.3 M distinct keys: more than kRadixSmallMax partial rows AND unique rows, so the key sort and the order sort both run on 2048-key tiles"""
    rng = np.random.default_rng(23)
    n = 2300000
    ev = _shape("distinct", n, 257, 21, rng)
    exp = _check_group_by(gpu_ctx, ev, 257, rng.permutation(257), 21, what="2.3M distinct")
    assert len(exp["tid"]) == n > 2097152


@pytest.mark.parametrize("extremes_at_ends", [True, False])
def test_group_by_one_key_in_tiles_far_apart(gpu_ctx, extremes_at_ends):
    """A x 700, B x 700, A x 700, ...: a key's first event, last event, smallest thick_start and largest thick_end come from different partial rows --
    once with the extremes ON the first and last events, once on events of tiles in between only"""
    rng = np.random.default_rng(700 + extremes_at_ends)
    t, s, l = _random_keys(rng, 2, 25, 21)
    pick = (np.arange(700 * 8) // 700) % 2
    ev = _events(t[pick], s[pick], l[pick], rng)
    ev["ts"][:] = ev["start"] - rng.integers(50, 100, len(pick), dtype=np.uint32)
    ev["te"][:] = ev["start"] + (ev["ilen_cls"] >> np.uint32(2)) + rng.integers(50, 100, len(pick), dtype=np.uint32)
    for key in (0, 1):
        at = np.nonzero(pick == key)[0]
        lo, hi = (at[0], at[-1]) if extremes_at_ends else (at[1500], at[2000])      # events 2900.. / 3300..: tiles 2 to 4 of 6
        ev["ts"][lo] = ev["start"][lo] - 150
        ev["te"][hi] = ev["start"][hi] + (ev["ilen_cls"][hi] >> np.uint32(2)) + 150
    exp = _check_group_by(gpu_ctx, ev, 25, rng.permutation(25), 21, what=("far apart", extremes_at_ends))
    assert len(exp["tid"]) == 2 and exp["count"].tolist() == [2800, 2800]
    assert sorted(exp["first_seen"].tolist()) == [0, 700] and sorted(exp["last_seen"].tolist()) == [4899, 5599]
    assert np.array_equal(exp["start"] - exp["ts"], [150, 150]) and np.array_equal(exp["te"] - exp["end"], [150, 150])


@pytest.fixture(scope="module")
def colliding():
    rng = np.random.default_rng(2047)
    return {slot: stage_ref.colliding_keys(slot, 1024, rng) for slot in (0, 1000, 2047)}


@pytest.mark.parametrize("layout", ["once", "twice_across", "twice_within"])
@pytest.mark.parametrize("slot", [0, 1000, 2047])
def test_group_by_keys_that_share_one_slot_of_the_tile_table(gpu_ctx, colliding, slot, layout):
    """1024 keys whose probes all start in one slot of k_preagg's 2048-slot table, in one aligned 1024-event tile: a probe chain 1024 long (from slot
    2047 it wraps to slot 0).  once: every key once.  twice_across: 2048 events, each tile holds every key once (two full chains, every key in two partial
    rows).  twice_within: each tile holds 512 of the keys twice (a chain is walked to an occupied slot that matches)."""
    rng = np.random.default_rng(slot + len(layout))
    t, s, l = colliding[slot]
    if layout == "once":
        pick = rng.permutation(1024)
    elif layout == "twice_across":
        pick = np.concatenate([rng.permutation(1024), rng.permutation(1024)])
    else:
        half = rng.permutation(1024)
        pick = np.concatenate([rng.permutation(np.repeat(half[:512], 2)), rng.permutation(np.repeat(half[512:], 2))])
    ev = _events(t[pick], s[pick], l[pick], rng)
    exp = _check_group_by(gpu_ctx, ev, 25, rng.permutation(25), 21, what=("colliding", slot, layout))
    assert len(exp["tid"]) == 1024 and set(exp["count"].tolist()) == ({1} if layout == "once" else {2})


@pytest.mark.parametrize("word", ["tid", "class_bits", "start_high_half"])
def test_group_by_keys_that_differ_in_one_word(gpu_ctx, word):
    """distinct keys stay distinct rows when only the tid, only the two class bits of ilen_cls, or only the high half of start tells them apart"""
    rng = np.random.default_rng(len(word))
    if word == "tid":
        m, n_groups = 300, 300
        t, s, l = np.arange(m), np.full(m, 123456), np.full(m, 1000 << 2 | 1)
    elif word == "class_bits":
        m, n_groups = 6, 25
        t, s, l = np.full(m, 7), np.full(m, 99000), np.array([500 << 2, 500 << 2 | 1, 500 << 2 | 2, 501 << 2, 501 << 2 | 1, 501 << 2 | 2])
    else:
        m, n_groups = 4000, 25
        t, s, l = np.full(m, 3), 5000 + (np.arange(m) << 16), np.full(m, 70 << 2)
    pick = rng.integers(0, m, 6000)
    pick[:m] = rng.permutation(m)                                                   # every key at least once
    ev = _events(t[pick], s[pick], l[pick], rng)
    exp = _check_group_by(gpu_ctx, ev, n_groups, rng.permutation(n_groups), 21, what=word)
    assert len(exp["tid"]) == m


def test_group_by_strand_byte_is_the_last_events(gpu_ctx):
    """'?' and '.' are one strand class (2): such events share a row, and the row prints the byte of its LAST event (junctions_extractor.cc:233)"""
    rng = np.random.default_rng(63)
    t, s, l = _random_keys(rng, 5, 25, 21)
    l = (l & ~np.uint32(3)) | np.uint32(2)
    pick = rng.integers(0, 5, 3000)
    strand = np.where(rng.integers(0, 2, 3000) == 1, ord("?"), ord(".")).astype(np.uint8)
    for key, byte in zip(range(5), "?.?.?"):                                        # the last event of each key, both ways round
        strand[np.nonzero(pick == key)[0][-1]] = ord(byte)
    ev = _events(t[pick], s[pick], l[pick], rng, strand=strand)
    exp = _check_group_by(gpu_ctx, ev, 25, rng.permutation(25), 21, what="strand byte")
    assert sorted(exp["strand"].tolist()) == sorted([ord(c) for c in "?.?.?"])
    assert np.array_equal(exp["strand"], strand[exp["last_seen"]].astype(np.uint32))


def test_stage_rows_are_not_taken_for_a_table(gpu_ctx, tmp_path):
    """rgx_k_group_by overwrites the block the last extraction's rows lie in: rgx_last_table_pack_device must refuse that extraction's table afterwards"""
    import os
    import regtools_amd
    from regtools_amd import _ffi, synth
    L = _ffi.lib()
    path = os.path.join(str(tmp_path), "t.bam")
    synth.write(path, 3000, shape="short", seed=5)
    je = regtools_amd.JunctionsExtractor(bam=path, strandness=1, ctx=gpu_ctx)
    je.identify_junctions_from_BAM()
    n = int(je._table.contents.n)
    assert n > 0
    d_dst = _empty(12 * n)
    err = C.create_string_buffer(ERRLEN)
    assert L.rgx_last_table_pack_device(gpu_ctx._h, je._table, d_dst.data_ptr(), n, err, ERRLEN) == 0, err.value
    rng = np.random.default_rng(1)
    t, s, l = _random_keys(rng, 10, 25, 21)
    _check_group_by(gpu_ctx, _events(t, s, l, rng), 25, rng.permutation(25), 21, forms=(0,))
    assert L.rgx_last_table_pack_device(gpu_ctx._h, je._table, d_dst.data_ptr(), n, err, ERRLEN) != 0
    assert b"not the result of the last extraction" in err.value
