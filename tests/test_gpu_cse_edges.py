"""The interval kernels of `cis-splice-effects identify / associate`, `junctions annotate` and `variants annotate` -- k_junction_scan_wave and
k_junction_scan, k_variant_scan, k_max_span / k_window_ranges / k_window_pairs_small / k_window_pairs, k_assoc_pairs (cse_kernels.hip over the cores of
cse_core.h) -- each on its own against plain Python (tests/cse_ref.py), on inputs aimed at their edges (tests/cse_edge_cases.py): junctions with
exactly 0 .. 200 candidate transcripts and the one flag-setting transcript at an exact candidate index around the turns of 64, items that straddle
the turns, transcripts filed at every bin level, both forms of the bin lookup (the direct index and, on annotations of 230 contigs, the binary search,
which no other GPU test reaches), variants around every exon edge under eighteen option sets, windows with exactly 4095 / 4096 / 4097 / 8197
candidates, large windows behind index 255, pair batches of every kind, contig buckets around the trip of 64.  Through the stage entry points
rgx_k_junction_scan (the RAW item list, before annotate_junctions makes it unique), rgx_variant_windows, rgx_k_window_pairs, rgx_k_assoc_pairs.
Everything is integers: every comparison is np.array_equal.  tests/test_cse_edges_host.py pins the references and the cases without a GPU.
Run with `-m gpu` on an MI355X.

That these tests can fail was shown once, on scratch builds with one-line faults under which the count and the fill pass still agree, this file run
once per build (the failing tests of each are listed; everything else passed):
  * k_junction_scan_wave, `seen = wave_scan_or(own, lane)` without `| acc` (the flags are not carried from turn to turn): 15 fail --
    test_junction_scan_raw_items_equal_the_reference[J_totals, J_setter_known, J_setter_donor, J_setter_acceptor, J_items; direct and search] and all
    five test_junction_scan_junction_counts_around_the_workgroup_of_four.  J_geometry (no junction with a second turn) and the
    search-against-direct tests (both layouts wrong alike) pass.
  * k_window_pairs, `rend >= beg` for `rend > beg`: 9 fail -- all eight test_window_pairs_equal_the_definition[W_sizes / W_300 x four batch sizes]
    and test_window_pairs_longest_span_behind_the_first_grid_of_max_span (its window is a large one).  Only windows of more than 4096 candidates
    are wrong: the small kernel keeps its `>`.
  * k_window_ranges, `lo_pos = beg` (the longest span ignored): the same 9 fail.
  * bin_range, `<` for `<=` in the upper bound of the binary search: 30 fail, every one on the 230-contig layout --
    test_junction_scan_raw_items_equal_the_reference[all six cases, search], all six test_junction_scan_search_index_equals_direct_index, all
    eighteen test_variant_scan_equals_the_reference[*-search].  Every test of the 3-contig layout passes: no other GPU test of the suite would
    have seen it.
  * k_assoc_pairs, `e < cee` for `e <= cee`: test_assoc_pairs_equal_the_definition[1000] fails ([1] passes: its one window ends ON a junction's
    start, not on its end).
  * variant_scan, `eb` from pos0 alone: 24 fail -- test_variant_scan_equals_the_reference for the twelve option sets with intronic_min 2 and 50, in
    both layouts (the position one base in front of the 16 KiB border that B_after starts on).  The six option sets with intronic_min 0 pass, as
    they must, and so do the three block-count tests (intronic_min 0).
Not run, because the passes would disagree or leave their buffers: n_items not carried from turn to turn (the fill pass would overwrite the turn
before; on the CPU: J_totals' junctions of 65 and more candidates would report the items of their last turn only), `>=` for `>` in the small kernel's
kBigWindow test (the window of 4096 candidates would be taken by neither kernel and its count slots left unwritten)."""
import ctypes as C

import numpy as np
import pytest

import cse_edge_cases as ec
import cse_ref

pytestmark = pytest.mark.gpu

ERRLEN = 512
JUNCTION_NAMES = sorted(ec.JUNCTION_CASES)


@pytest.fixture(scope="module")
def edge_dir(built, tmp_path_factory):
    return tmp_path_factory.mktemp("cse_edges_gpu")


@pytest.fixture(scope="module")
def annotations(gpu_ctx, edge_dir):
    """(case, reference annotation, loaded rgx_gtf) by (name, layout): every annotation is loaded once for the module"""
    from regtools_amd import _ffi
    L = _ffi.lib()
    loaded = {}

    def get(name, layout):
        if (name, layout) not in loaded:
            case = ec.build(name, edge_dir, layout)
            g, err = C.c_void_p(), C.create_string_buffer(ERRLEN)
            assert L.rgx_gtf_load(gpu_ctx._h, case.gtf.encode(), C.byref(g), err, ERRLEN) == 0, err.value
            # the form of the bin lookup this layout is meant to run
            assert L.rgx_gtf_bin_index(g) == (1 if layout == "direct" else 0), (name, layout)
            loaded[(name, layout)] = (case, cse_ref.Annotation(case.transcripts, case.contigs), g)
        return loaded[(name, layout)]
    yield get
    for _, _, g in loaded.values():
        L.rgx_gtf_free(g)


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _arr(p, n):
    return np.ctypeslib.as_array(p, shape=(int(n),)).copy() if n else np.zeros(0, dtype=np.uint32)


def k_junction_scan(gpu_ctx, g, contig, start, end1, strand, keep_single, form):
    from regtools_amd import _ffi
    L = _ffi.lib()
    n = len(contig)
    contig, start, end1 = np.ascontiguousarray(contig, dtype=np.int32), np.ascontiguousarray(start, dtype=np.uint32), np.ascontiguousarray(end1, dtype=np.uint32)
    out, err = C.POINTER(_ffi.JunctionItems)(), C.create_string_buffer(ERRLEN)
    rc = L.rgx_k_junction_scan(gpu_ctx._h, g, n, _ptr(contig, C.c_int32), _ptr(start, C.c_uint32), _ptr(end1, C.c_uint32), strand.encode(), int(keep_single),
                               form, C.byref(out), err, ERRLEN)
    assert rc == 0, err.value                                    # RGX_OK: the guards behind the three item columns are untouched
    r = out.contents
    off = _arr(r.item_off, n + 1)
    total = int(off[n])
    got = dict(flags=_arr(r.flags, n), visits=_arr(r.visits, n), off=off, kind=_arr(r.item_kind, total), a=_arr(r.item_a, total), b=_arr(r.item_b, total),
               visits_total=int(r.visits_total))
    L.rgx_junction_items_free(out)
    return got


def check_junctions(gpu_ctx, g, ann, contig, start, end1, strand, what):
    """both forms against the reference and against each other, with and without single-exon transcripts"""
    for keep_single in (False, True):
        exp = cse_ref.junction_scan(ann, contig, start, end1, strand, keep_single)
        got = {form: k_junction_scan(gpu_ctx, g, contig, start, end1, strand, keep_single, form) for form in (0, 1)}
        print("%s keep_single=%d: %d junctions, %d items, flags %s" % (what, keep_single, len(contig), len(exp["kind"]), np.bincount(exp["flags"], minlength=8).tolist()))
        for form, name in ((0, "wave"), (1, "lane")):
            for k in ("flags", "off", "kind", "a", "b"):
                assert np.array_equal(got[form][k], exp[k]), (what, keep_single, name, k, _first(got[form][k], exp[k]))
            assert got[form]["visits_total"] == int(exp["visits"].sum()), (what, keep_single, name)
        assert np.array_equal(got[0]["visits"], exp["visits"]), (what, keep_single, _first(got[0]["visits"], exp["visits"]))
        for k in ("flags", "off", "kind", "a", "b"):
            assert np.array_equal(got[0][k], got[1][k]), (what, keep_single, k)
    return exp


def _first(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.asarray(a[:n]) != np.asarray(b[:n]))[0]
    return "lengths %d / %d, first difference at %s" % (len(a), len(b), ("%d: device %d, reference %d" % (d[0], a[d[0]], b[d[0]])) if len(d) else "none")


# ---- a11: the junction scan -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ec.LAYOUTS)
@pytest.mark.parametrize("name", JUNCTION_NAMES)
def test_junction_scan_raw_items_equal_the_reference(gpu_ctx, annotations, name, layout):
    """Flags, exon-visit counts and the raw item lists of both kernel forms, under both forms of the bin lookup: candidate totals on and around the
    turns (J_totals), the only flag-setter at the candidate indexes 0, 62 .. 65, 127, 128 (J_setter_*: nothing before it is listed, everything from it
    on is), items across turn borders and transcripts that return before their loop (J_items), the seven bin levels and the bin borders (J_geometry)."""
    case, ann, g = annotations(name, layout)
    exp = check_junctions(gpu_ctx, g, ann, case.j_contig, case.j_start, case.j_end1, case.j_strand, "%s/%s" % (name, layout))
    assert len(exp["kind"]) > 0


@pytest.mark.parametrize("n", [1, 3, 4, 5, 129])
def test_junction_scan_junction_counts_around_the_workgroup_of_four(gpu_ctx, annotations, n):
    """the first n junctions of J_items: a '?' strand and a contig of -1 stand among ordinary junctions inside the first workgroup of four waves"""
    case, ann, g = annotations("J_items", "direct")
    check_junctions(gpu_ctx, g, ann, case.j_contig[:n], case.j_start[:n], case.j_end1[:n], case.j_strand[:n], "J_items[:%d]" % n)


@pytest.mark.parametrize("name", JUNCTION_NAMES)
def test_junction_scan_search_index_equals_direct_index(gpu_ctx, annotations, name):
    """the same loci on 3 contigs (direct index) and on the first, the middle and the last of 230 (binary search): the same lists, transcript by name"""
    from regtools_amd import _ffi
    L = _ffi.lib()
    res = {}
    for layout in ec.LAYOUTS:
        case, ann, g = annotations(name, layout)
        r = k_junction_scan(gpu_ctx, g, case.j_contig, case.j_start, case.j_end1, case.j_strand, True, 0)
        names = np.array([L.rgx_gtf_transcript_id(g, int(t)) for t in r["a"][r["kind"] == cse_ref.ITEM_TX]])
        r["a"][r["kind"] == cse_ref.ITEM_TX] = 0
        res[layout] = (r, names)
    (d, dn), (s, sn) = res["direct"], res["search"]
    for k in ("flags", "visits", "off", "kind", "a", "b"):
        assert np.array_equal(d[k], s[k]), (name, k)
    assert np.array_equal(dn, sn) and len(dn) > 0


# ---- a10: the variant scan ------------------------------------------------------------------------------------------------------------------------
def k_variant_windows(gpu_ctx, g, contig_names, pos0, o):
    from regtools_amd import _ffi
    L = _ffi.lib()
    n = len(contig_names)
    names = (C.c_char_p * n)(*[c.encode() for c in contig_names])
    pos0 = np.ascontiguousarray(pos0, dtype=np.uint32)
    out, err = C.POINTER(_ffi.VariantHits)(), C.create_string_buffer(ERRLEN)
    rc = L.rgx_variant_windows(gpu_ctx._h, g, n, names, _ptr(pos0, C.c_uint32), o["intronic_min"], o["exonic_min"], o["all_intronic"], o["all_exonic"],
                               o["skip_single"], C.byref(out), err, ERRLEN)
    assert rc == 0, err.value
    h = out.contents
    off = _arr(h.hit_off, n + 1)
    total = int(off[n])
    got = dict(ces=_arr(h.cis_start, n), cee=_arr(h.cis_end, n), off=off, tx=_arr(h.hit_transcript, total), ann=_arr(h.hit_annotation, total),
               dist=_arr(h.hit_distance, total))
    L.rgx_variant_hits_free(out)
    return got


def check_variants(gpu_ctx, g, ann, contig_names, pos0, o, what):
    contig = np.array([ann.contig_index.get(c, -1) for c in contig_names], dtype=np.int32)
    exp = cse_ref.variant_scan(ann, contig, pos0, **o)
    got = k_variant_windows(gpu_ctx, g, contig_names, pos0, o)
    print("%s %s: %d variants, %d hits" % (what, o, len(contig), len(exp["tx"])))
    for k in ("ces", "cee", "off", "tx", "ann", "dist"):
        assert np.array_equal(got[k], exp[k]), (what, o, k, _first(got[k], exp[k]))
    return exp


@pytest.mark.parametrize("layout", ec.LAYOUTS)
@pytest.mark.parametrize("k", range(len(ec.VARIANT_OPTS)))
def test_variant_scan_equals_the_reference(gpu_ctx, annotations, layout, k):
    """354 positions around every exon edge +- exonic_min / intronic_min for E, I in {0, 2/3, 50}, with -I, -E and -S: first, inner and last exons
    on either strand, the seven-level transcripts, positions below intronic_min, positions astride a 16 KiB border, 0, 1 and 70 hits, an unknown
    contig; under both forms of the bin lookup."""
    case, ann, g = annotations("V_edges", layout)
    exp = check_variants(gpu_ctx, g, ann, case.v_contig, case.v_pos0, ec.VARIANT_OPTS[k], "V_edges/%s" % layout)
    assert len(exp["tx"]) > 0


@pytest.mark.parametrize("n", [127, 128, 129])
def test_variant_scan_variant_counts_around_the_block(gpu_ctx, annotations, n):
    """the last n variants (the 70-hit position and the unknown contig among them): one block of 128 threads short of, full, and one over"""
    case, ann, g = annotations("V_edges", "direct")
    check_variants(gpu_ctx, g, ann, case.v_contig[-n:], case.v_pos0[-n:], ec.VARIANT_OPTS[2], "V_edges[-%d:]" % n)


# ---- a9: the window join's pair lists ---------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def k_window_pairs(gpu_ctx, c, batch):
    import torch
    from regtools_amd import _ffi
    L = _ffi.lib()
    d = [_dev(c.tid), _dev(c.rpos), _dev(c.rend)]
    torch.cuda.synchronize()                                     # the context's stream does not wait for torch's
    out, err = C.POINTER(_ffi.PairList)(), C.create_string_buffer(ERRLEN)
    rc = L.rgx_k_window_pairs(gpu_ctx._h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(c.tid), len(c.w_tid), _ptr(c.w_tid, C.c_int32),
                              _ptr(c.w_beg, C.c_int32), _ptr(c.w_end, C.c_int32), batch, C.byref(out), err, ERRLEN)
    assert rc == 0, err.value                                    # RGX_OK: the guards behind both pair lists are untouched, in every batch
    r = out.contents
    got = (_arr(r.first, r.n), _arr(r.window, r.n), int(r.n_batches))
    L.rgx_pair_list_free(out)
    for t, a in zip(d, (c.tid, c.rpos, c.rend)):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), a)  # the caller's columns are read, never written
    return got


_window_ref = {}


def window_ref(c):
    if c.name not in _window_ref:
        _window_ref[c.name] = cse_ref.window_pairs(c.tid, c.rpos, c.rend, c.w_tid, c.w_beg, c.w_end)
    return _window_ref[c.name]


@pytest.mark.parametrize("batch", ec.PAIR_BATCHES)
@pytest.mark.parametrize("name", ["W_sizes", "W_300"])
def test_window_pairs_equal_the_definition(gpu_ctx, name, batch):
    """W_sizes: windows of exactly 0 .. 5, 63 .. 65, 255 .. 257, 4095, 4096, 4097 (the border between the wave-per-window and the
    workgroup-per-slice kernel: each window taken by exactly one) and 8197 candidates (slices of 2049 and 2050: three trips of 1024), half of the
    large windows' candidates ending in front of them; rend == beg out, rend == beg + 1 in, rpos == end - 1 in, rpos == end out; beg = 0 and
    beg below the longest span; contigs without events; a window twice.  W_300: large windows at the indexes 0, 255, 256 and 299 of 300.  In one
    batch, in several, with the large windows alone in theirs, with every window alone."""
    c = ec.build(name, None)
    ev, win, counts = window_ref(c)
    got_ev, got_win, n_batches = k_window_pairs(gpu_ctx, c, batch)
    print("%s batch %d: %d windows, %d pairs, %d batches" % (name, batch, len(counts), len(ev), n_batches))
    assert np.array_equal(got_win, win), _first(got_win, win)
    assert np.array_equal(got_ev, ev), _first(got_ev, ev)
    assert n_batches == cse_ref.pair_batches(counts, batch or 1 << 26, len(c.tid))


def test_window_pairs_longest_span_behind_the_first_grid_of_max_span(gpu_ctx):
    """270,000 events: k_max_span strides; the longest read is event 265,000 and two windows hold it alone"""
    c = ec.build("W_span", None)
    ev, win, counts = window_ref(c)
    got_ev, got_win, n_batches = k_window_pairs(gpu_ctx, c, 0)
    assert np.array_equal(got_win, win) and np.array_equal(got_ev, ev), (_first(got_win, win), _first(got_ev, ev))
    assert n_batches == 1 and got_ev[got_win == 0].tolist() == [c.claims["longest"]]


def test_window_pairs_without_events_or_windows(gpu_ctx):
    c = ec.build("W_sizes", None)
    e = ec.Case()
    e.tid = e.rpos = e.rend = np.zeros(0, dtype=np.uint32)
    e.w_tid, e.w_beg, e.w_end = c.w_tid, c.w_beg, c.w_end
    assert [len(x) for x in k_window_pairs(gpu_ctx, e, 0)[:2]] == [0, 0]
    e.tid, e.rpos, e.rend = c.tid, c.rpos, c.rend
    e.w_tid = e.w_beg = e.w_end = np.zeros(0, dtype=np.int32)
    assert [len(x) for x in k_window_pairs(gpu_ctx, e, 0)[:2]] == [0, 0]


# ---- associate: the pair join -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1000])
def test_assoc_pairs_equal_the_definition(gpu_ctx, n):
    """contig buckets of 0, 1, 63, 64, 65 and 129 junctions (the last contig's the largest: three trips of 64), windows on contig -1, windows with
    ces > cee, a junction's start or end ON ces and ON cee, a junction that covers its window without an end inside; 1 window and 1000"""
    from regtools_amd import _ffi
    L = _ffi.lib()
    c = ec.build("A_%d" % n, None)
    pj, pw = cse_ref.assoc_pairs(c.w_contig, c.w_ces, c.w_cee, c.contig_off, c.j_start, c.j_end)
    out, err = C.POINTER(_ffi.PairList)(), C.create_string_buffer(ERRLEN)
    rc = L.rgx_k_assoc_pairs(gpu_ctx._h, n, _ptr(c.w_contig, C.c_int32), _ptr(c.w_ces, C.c_uint32), _ptr(c.w_cee, C.c_uint32), len(ec.BUCKETS),
                             _ptr(c.contig_off, C.c_uint32), len(c.j_start), _ptr(c.j_start, C.c_uint32), _ptr(c.j_end, C.c_uint32), C.byref(out), err, ERRLEN)
    assert rc == 0, err.value
    r = out.contents
    got_j, got_w = _arr(r.first, r.n), _arr(r.window, r.n)
    L.rgx_pair_list_free(out)
    print("A_%d: %d pairs" % (n, len(pj)))
    assert len(pj) > 0
    assert np.array_equal(got_w, pw), _first(got_w, pw)
    assert np.array_equal(got_j, pj), _first(got_j, pj)
