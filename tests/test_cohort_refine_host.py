"""The refined intron clusters of a cohort matrix without a device: the contract of rgx_cohort_refine in include/regtools_amd.h as
rgx_cohort_refine_host (the library's plain C++ twin) keeps it, and the -l / -J / -p options of `regtools-amd junctions cohort`.
Expectations: literals written out for the hand-made cohort (tests/refine_cases.py) and the Python restatement of tests/refine_ref.py, which
iterates the removal until nothing leaves and asserts that one removal was all.  Every comparison is between integers or bytes and exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cluster_cases
import cluster_ref
import refine_cases as cases
import refine_ref
from cohort_common import HostMatrix, table_from_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "regtools-amd")
RGX_ERR_ARG = 7


def _matrix(tables, names, **kw):
    from regtools_amd import cohort
    hm = HostMatrix(tables, [8] * len(tables), names, **kw)
    assert hm.rc == 0, hm.err.value
    m, hm.h = cohort.CohortMatrix(hm.h), None
    return m


def _hand():
    tables = [table_from_rows(cases.HAND_P), table_from_rows(cases.HAND_Q)]
    return tables, _matrix(tables, ["p", "q"], only_anchored=False, min_total=0)


def test_defaults_remove_nothing():
    from regtools_amd import _ffi
    p = _ffi.RefineParams(7, 7, 7, 7, 7, 7)
    _ffi.lib().rgx_refine_params_default(C.byref(p))
    assert (p.max_intron, p.min_reads, p.ratio_num, p.ratio_den, p.min_rows, p.min_total) == (0, 0, 0, 1, 1, 0)


def test_hand_made_cohort_against_literals():
    from regtools_amd import cohort
    tables, m = _hand()
    assert [(int(t), int(s), int(e), c.decode()) for t, s, e, c in zip(m.tid, m.start, m.end, m.strand)] == cases.HAND_ROWS
    assert [int(x) for x in m.total] == cases.HAND_TOTALS
    for kw, lit in cases.HAND:
        cl, want = cohort.refine_host(m, **kw), refine_ref.refine(m, **kw)
        cases.check_literals(cl, m, lit)
        cases.check_literals(_Want(want), m, {k: v for k, v in lit.items() if k != "text"})      # the literals re-derived through the restatement
        refine_ref.same(cl, want)
        assert cl.counts_text(m) == refine_ref.counts_text(m, want) and cl.n_rounds == 0
        if "text" in lit:
            assert refine_ref.counts_text(m, want).decode().splitlines() == lit["text"]
        cl.close()
    # defaults: what rgx_cohort_cluster_host gives
    a, b = cohort.refine_host(m), cohort.cluster_host(m)
    refine_ref.same_clusters(a, b)
    assert (a.n_ineligible, a.n_weak) == (0, 0) and a.counts_text(m) == b.counts_text(m)
    a.close(); b.close()
    for kw in (dict(min_rows=2), dict(min_total=41), dict(min_rows=2, min_total=100)):
        a, b = cohort.refine_host(m, **kw), cohort.cluster_host(m, **kw)
        refine_ref.same_clusters(a, b)
        a.close(); b.close()
    m.close()
    cluster_cases.free_tables(tables)


class _Want(object):
    """A restatement's dict read like a CohortClusters."""

    def __init__(self, d):
        self.__dict__.update(d)


def test_equality_passes_the_ratio_test():
    from regtools_amd import cohort
    tables, m = _hand()
    for kw, stays in cases.BOUNDARY:
        cl, want = cohort.refine_host(m, **kw), refine_ref.refine(m, **kw)
        refine_ref.same(cl, want)
        assert (int(cl.cluster[2]) != cases.NO) == stays, kw
        cl.close()
    m.close()
    cluster_cases.free_tables(tables)


def test_the_ratio_test_is_made_on_the_whole_products():
    from regtools_amd import cohort
    tables = [table_from_rows(cases.WIDE_P), table_from_rows(cases.WIDE_Q)]
    m = _matrix(tables, ["p", "q"], only_anchored=False)
    num, den = cases.WIDE_RATIO
    x, T = int(m.total[0]), int(m.total.sum())
    assert [int(t) for t in m.total] == [8_000_000_000, 1]
    exact, wrapped = x * den < num * T, (x * den) % 2**64 < (num * T) % 2**64
    assert (exact, wrapped) == (False, True)                 # a left product taken mod 2^64 would remove X too: the case tests the wide path
    cl, want = cohort.refine_host(m, min_ratio=cases.WIDE_RATIO), refine_ref.refine(m, min_ratio=cases.WIDE_RATIO)
    refine_ref.same(cl, want)
    assert cl.n_weak == 1 and [int(c) for c in cl.cluster] == [0, cases.NO] and [int(t) for t in cl.cl_total] == [8_000_000_000]
    cl.close(); m.close()
    cluster_cases.free_tables(tables)


def test_bad_ratios_are_refused():
    from regtools_amd import RegtoolsError, cohort
    tables, m = _hand()
    for ratio in ((2, 1), (1, 0)):
        with pytest.raises(RegtoolsError) as e:
            cohort.refine_host(m, min_ratio=ratio)
        assert e.value.code == RGX_ERR_ARG
    m.close()
    cluster_cases.free_tables(tables)


@pytest.mark.parametrize("rows", [0] + cases.CHAIN_ROWS)
def test_chains_whose_survivors_sit_on_the_compaction_edges(rows):
    from regtools_amd import cohort
    L = rows or 97
    tid, start, end, cls, count = cases.chain(L)
    t = cluster_cases.table_of(0, tid, start, end, count, np.full(L, ord("+"), np.uint32))
    m = cohort.merge_host([cluster_cases.Sample(t)], ["only"])
    assert m.n == L and [int(x) for x in m.total[:3]] == [5, 5, 1][:L]
    kw = dict(min_reads=cases.CHAIN_MIN_READS) if rows else dict(max_intron=1, min_reads=cases.CHAIN_MIN_READS)
    cl, want = cohort.refine_host(m, **kw), refine_ref.refine(m, **kw)
    refine_ref.same(cl, want)
    if rows:
        assert (cl.n_ineligible, cl.n_weak, int(cl.cl_begin[-1])) == (0, L // 3, cases.chain_survivors(L))
        assert (int(cl.cluster[-1]) == cases.NO) == (L % 3 == 0)
    else:
        assert (cl.n_ineligible, cl.n_weak, cl.n_clusters, cl.n_components) == (L, 0, 0, 0) and list(cl.cl_begin) == [0] and list(cl.cs_begin) == [0]
        assert len(cl.cl_row) == len(cl.cs_sample) == 0 and cl.counts_text(m) == b"chrom only\n"
    cl.close(); m.close()
    cluster_cases.free_tables([t])


def test_empty_matrix():
    from regtools_amd import cohort
    m = _matrix([], [])
    cl = cohort.refine_host(m, max_intron=10, min_reads=3, min_ratio=(1, 2))
    assert (cl.n_rows, cl.n_clusters, cl.n_components, cl.n_ineligible, cl.n_weak) == (0, 0, 0, 0, 0) and list(cl.cl_begin) == [0] and list(cl.cs_begin) == [0]
    assert cl.counts_text(m) == b"chrom\n"
    cl.close(); m.close()


def test_heavy_tailed_random_cohort_of_six_samples():
    from regtools_amd import cohort
    G = 6
    tid, start, end, cls = cluster_cases.random_junctions()
    tables = cases.heavy_tables(G, tid, start, end, cls)
    m = cohort.merge_host([cluster_cases.Sample(t) for t in tables], ["g%d" % g for g in range(G)])
    assert m.n == len(tid) == 199_998 and np.array_equal(m.start, start) and np.array_equal(m.end, end) and np.array_equal(m.tid, tid)
    kw = dict(max_intron=200000, min_reads=30, min_ratio=(1, 100))
    rem = refine_ref.removal(m, **kw)
    print("heavy-tailed cohort, G = %d: %d ineligible, %d weak (%d by reads only, %d by ratio only), removed per round %s" % (
        G, rem["n_ineligible"], rem["n_weak"], rem["by_reads"], rem["by_ratio"], rem["removed_per_round"]))
    assert rem["n_ineligible"] >= 5000 and rem["by_reads"] >= 5000 and rem["by_ratio"] >= 5000
    # the giant the refinement is there to break up: the largest component of the unrefined clustering (LeafCutter's first step, every row) is
    # above 1,024 rows; among the eligible rows alone the largest stage-1 component is printed (827 rows with these parameters)
    first_step = cohort.cluster_host(m)
    print("  largest component: %d rows unrefined, %d among the eligible rows" % (np.diff(first_step.cl_begin).max(),
                                                                                   np.bincount(rem["stage1_label"][rem["stage1_alive"]]).max()))
    assert np.diff(first_step.cl_begin).max() > 1024
    for filt in (dict(), dict(min_rows=2, min_total=30)):
        want = refine_ref.clusters_of(m, rem, **filt)
        cl = cohort.refine_host(m, **kw, **filt)
        refine_ref.same(cl, want)
        assert cl.counts_text(m) == refine_ref.counts_text(m, want)
        sizes = np.diff(cl.cl_begin)
        print("  %s: %d components, %d clusters, largest %d rows, %d of two rows or more" % (filt, cl.n_components, cl.n_clusters, sizes.max(), (sizes >= 2).sum()))
        assert (sizes >= 2).sum() >= 10_000 and sizes.max() < 1024
        cl.close()
    # defaults: the unrefined clusters, in every array and count
    a = cohort.refine_host(m)
    refine_ref.same_clusters(a, first_step)
    assert (a.n_ineligible, a.n_weak) == (0, 0)
    a.close(); first_step.close(); m.close()
    cluster_cases.free_tables(tables)


def _run(*args):
    return subprocess.run([EXE, "junctions", "cohort"] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_tool_option_surface(tmp_path):
    h = _run("-h")
    assert h.returncode == 0
    for opt in (b"\t\t-l INT\t", b"\t\t-J INT\t", b"\t\t-p DEC\t", b"-l 100000 -J 5 -p 0.001 -K 2 -T 30"):
        assert opt in h.stdout, opt
    k = str(tmp_path / "clusters.txt")
    # an accepted ratio lets the run get as far as the device it does not find or the file it cannot open
    for ratio in ("0.001", "1", "0", "1.000000000", ".5", "0."):
        r = _run("-s", "XS", "-k", k, "-l", "100000", "-J", "5", "-p", ratio, "a.bam")
        assert r.returncode == 1 and r.stdout == b"" and b"Unrecognized ratio argument!" not in r.stderr and h.stdout not in r.stderr, ratio
        assert not os.path.exists(k)
    for ratio in ("2", "x", "0.0000000001", "-1", "1.000000001", "", ".", "0.5x", "1e-3"):
        r = _run("-s", "XS", "-k", k, "-p", ratio, "a.bam")
        assert r.returncode == 1 and r.stdout == b"" and b"Unrecognized ratio argument!" in r.stderr and not os.path.exists(k), ratio
