"""The intron clusters of a cohort matrix without a device: the contract of include/regtools_amd.h as rgx_cohort_cluster_host (the library's plain
C++ twin of rgx_cohort_cluster) keeps it, the perind.counts-style text, and the -k / -K / -T options of `regtools-amd junctions cohort`.
Expectations: literals written out for the hand-made cohort, tests/cluster_ref.py (a Python union-find) for the random one.  Every comparison is
between integers or bytes and exact."""
import ctypes as C
import os
import subprocess

import numpy as np

import cluster_cases as cases
import cluster_ref
from cohort_common import HostMatrix, table_from_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "regtools-amd")


def _matrix(tables, names, **kw):
    """rgx_cohort_merge_host over raw tables, as a CohortMatrix (which owns it)."""
    from regtools_amd import cohort
    hm = HostMatrix(tables, [8] * len(tables), names, **kw)
    assert hm.rc == 0, hm.err.value
    m, hm.h = cohort.CohortMatrix(hm.h), None
    return m


def _hand():
    tables = [table_from_rows(cases.HAND_P), table_from_rows(cases.HAND_Q)]
    return tables, _matrix(tables, ["p", "q"], only_anchored=False, min_total=0)


def _check_literal(cl, m, want):
    assert (cl.n_rows, cl.n_clusters, cl.n_components) == (len(want["cluster"]), len(want["cl_total"]), want["n_components"])
    for k in ("cluster", "cl_begin", "cl_row", "cl_total", "cs_begin", "cs_sample", "cs_total"):
        assert [int(x) for x in getattr(cl, k)] == want[k], k
    assert cl.counts_text(m).decode().splitlines() == want["text"]
    assert cl.n_rounds == 0                                  # the twin runs no rounds


def test_defaults():
    from regtools_amd import _ffi
    p = _ffi.ClusterParams(7, 7)
    _ffi.lib().rgx_cluster_params_default(C.byref(p))
    assert (p.min_rows, p.min_total) == (1, 0)


def test_hand_made_cohort_against_literals():
    """Shared start, shared end, the transitive triple, the two strands apart, '?' with '.', the two contigs apart, a singleton; a 0/0 and an NA."""
    from regtools_amd import cohort
    tables, m = _hand()
    assert [(int(t), int(s), int(e), c.decode()) for t, s, e, c in zip(m.tid, m.start, m.end, m.strand)] == [
        (0, 100, 200, "+"), (0, 100, 200, "-"), (0, 100, 300, "+"), (0, 150, 300, "+"), (0, 400, 450, "+"), (0, 500, 600, "?"), (0, 500, 700, "."),
        (1, 100, 200, "+")]
    cl = cohort.cluster_host(m)
    _check_literal(cl, m, cases.HAND)
    cluster_ref.same(cl, cluster_ref.clusters(m))
    assert cl.counts_text(m) == cluster_ref.counts_text(m, cluster_ref.clusters(m))
    cl.close(); m.close()
    cases.free_tables(tables)


def test_two_rows_at_a_time():
    from regtools_amd import cohort
    for rows, want in (([(0, 100, 200, 90, 230, 3, "+"), (0, 100, 250, 90, 260, 1, "+")], [0, 0]),          # one start
                       ([(0, 100, 250, 90, 260, 3, "+"), (0, 130, 250, 90, 260, 1, "+")], [0, 0]),          # one end
                       ([(0, 100, 200, 90, 230, 3, "+"), (0, 200, 300, 190, 330, 1, "+")], [0, 1]),         # an end that is another's start: no link
                       ([(0, 100, 200, 90, 230, 3, "+"), (0, 100, 250, 90, 260, 1, "-")], [0, 1]),
                       ([(0, 100, 200, 90, 230, 3, "?"), (0, 100, 250, 90, 260, 1, ".")], [0, 0]),
                       ([(0, 100, 200, 90, 230, 3, "+"), (1, 100, 250, 90, 260, 1, "+")], [0, 1])):
        t = table_from_rows(rows)
        m = _matrix([t], ["s"], only_anchored=False)
        cl = cohort.cluster_host(m)
        assert list(cl.cluster) == want and cl.n_components == cl.n_clusters == max(want) + 1, rows
        cl.close(); m.close()
        cases.free_tables([t])


def test_filters_drop_whole_components_and_renumber():
    from regtools_amd import cohort
    tables, m = _hand()
    cl = cohort.cluster_host(m, min_rows=2)
    _check_literal(cl, m, cases.HAND_MIN_ROWS_2)
    cl.close()
    # the cluster of rows 5 and 6 has 3 reads: kept at exactly 3, dropped just above
    cl = cohort.cluster_host(m, min_total=3)
    _check_literal(cl, m, cases.HAND)
    cl.close()
    cl = cohort.cluster_host(m, min_total=4)
    assert [int(x) for x in cl.cluster] == [0, 1, 0, 0, 2, cases.NO, cases.NO, 3] and [int(x) for x in cl.cl_total] == [10, 5, 6, 7]
    assert cl.n_components == 5 and [int(x) for x in cl.cs_begin] == [0, 2, 3, 4, 5]
    assert cl.counts_text(m).decode().splitlines() == [ln.replace("clu_5", "clu_4") for ln in cases.HAND["text"] if "clu_4" not in ln]
    cl.close()
    for kw in (dict(min_rows=2, min_total=3), dict(min_rows=2, min_total=4), dict(min_rows=3, min_total=10), dict(min_rows=3, min_total=11), dict(min_rows=4)):
        cl, want = cohort.cluster_host(m, **kw), cluster_ref.clusters(m, **kw)
        cluster_ref.same(cl, want)
        assert cl.counts_text(m) == cluster_ref.counts_text(m, want)
        assert cl.n_clusters == {(2, 3): 2, (2, 4): 1, (3, 10): 1, (3, 11): 0, (4, 0): 0}[(kw["min_rows"], kw.get("min_total", 0))]
        cl.close()
    m.close()
    cases.free_tables(tables)


def test_empty_matrix_and_a_matrix_made_with_min_samples():
    from regtools_amd import cohort
    for tables, names in (([], []), ([table_from_rows([])], ["none"])):
        m = _matrix(tables, names)
        cl = cohort.cluster_host(m)
        assert (cl.n_rows, cl.n_clusters, cl.n_components) == (0, 0, 0) and list(cl.cl_begin) == [0] and list(cl.cs_begin) == [0]
        assert len(cl.cluster) == len(cl.cl_row) == len(cl.cs_sample) == 0
        assert cl.counts_text(m) == ("chrom" + "".join(" " + s for s in names) + "\n").encode()
        cl.close(); m.close()
        cases.free_tables(tables)
    tables = [table_from_rows(cases.HAND_P), table_from_rows(cases.HAND_Q)]
    m = _matrix(tables, ["p", "q"], only_anchored=False, min_samples=2)          # only chrA 100-200 + is in both samples
    cl = cohort.cluster_host(m)
    assert m.n == 1 and list(cl.cluster) == [0] and list(cl.cl_total) == [4] and list(cl.cs_total) == [3, 1]
    assert cl.counts_text(m) == b"chrom p q\nchrA:100:200:clu_1_+ 3/3 1/1\n"
    cl.close(); m.close()
    cases.free_tables(tables)


def test_a_count_of_zero_gives_no_denominator():
    """cs_* lists the samples with a non-zero sum: a sample whose only entries in a cluster are zeros is not among them."""
    from regtools_amd import cohort
    tables = [table_from_rows([(0, 100, 200, 90, 230, 0, "+"), (0, 100, 250, 90, 260, 0, "+")]), table_from_rows([(0, 100, 200, 90, 230, 2, "+")])]
    m = _matrix(tables, ["zero", "two"], only_anchored=False, min_total=0)
    cl = cohort.cluster_host(m)
    assert list(cl.cluster) == [0, 0] and list(cl.cs_sample) == [1] and list(cl.cs_total) == [2] and list(cl.cs_begin) == [0, 1]
    assert cl.counts_text(m) == b"chrom zero two\nchrA:100:200:clu_1_+ 0/0 2/2\nchrA:100:250:clu_1_+ 0/0 0/2\n"
    cluster_ref.same(cl, cluster_ref.clusters(m))
    cl.close(); m.close()
    cases.free_tables(tables)


def test_formatter_sizes_then_fills():
    from regtools_amd import _ffi, cohort
    fn = _ffi.lib().rgx_cohort_format_cluster_counts
    tables, m = _hand()
    cl = cohort.cluster_host(m)
    text = cl.counts_text(m)
    n = fn(m._h, cl._h, None, 0)
    assert n == len(text) > 0
    small = C.create_string_buffer(b"#" * n, n)
    assert fn(m._h, cl._h, small, n - 1) == n and small.raw == b"#" * n          # too small: the size again, nothing written
    exact = C.create_string_buffer(b"#" * (n + 4), n + 4)
    assert fn(m._h, cl._h, exact, n) == n and exact.raw == text + b"####"
    cl.close(); m.close()
    cases.free_tables(tables)


def test_random_cohort_of_six_samples_equals_the_restatement():
    from regtools_amd import cohort
    tid, start, end, cls = cases.random_junctions()
    tables = cases.sample_tables(6, tid, start, end, cls)
    m = cohort.merge_host([cases.Sample(t) for t in tables], ["g%d" % g for g in range(6)])
    assert m.n == len(tid) == 199_998 and np.array_equal(m.start, start) and np.array_equal(m.end, end) and np.array_equal(m.tid, tid)
    for kw in (dict(), dict(min_rows=2, min_total=25)):
        want = cluster_ref.clusters(m, **kw)
        cl = cohort.cluster_host(m, **kw)
        cluster_ref.same(cl, want)
        assert cl.counts_text(m) == cluster_ref.counts_text(m, want)
        if not kw:
            sizes = np.diff(cl.cl_begin)
            assert (sizes > 1024).sum() >= 5 and (sizes == 1).sum() >= 10_000 and (sizes >= 2).sum() >= 10_000
        else:
            assert 0 < cl.n_clusters < cl.n_components
        cl.close()
    m.close()
    cases.free_tables(tables)


def _run(*args):
    return subprocess.run([EXE, "junctions", "cohort"] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_tool_option_surface():
    h = _run("-h")
    assert h.returncode == 0
    for opt in (b"\t\t-k FILE\t", b"\t\t-K INT\t", b"\t\t-T INT\t"):
        assert opt in h.stdout, opt
    # -K and -T are read with atoi / atoll like their neighbours ("x" is 0, never a usage error): the run gets as far as the file it cannot open
    for args in (["-K", "x"], ["-K", "2x", "-T", "y"], ["-k", "clusters.txt", "-T", "7"]):
        r = _run("-s", "XS", *args, "a.bam")
        assert r.returncode == 1 and r.stdout == b"" and h.stdout not in r.stderr and not os.path.exists("clusters.txt"), args
    r = _run("-s", "XS", "-K")                               # an option without its argument is a usage error
    assert r.returncode == 1 and h.stdout in r.stderr
