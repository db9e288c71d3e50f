"""The refined intron clusters of a cohort matrix on the device (rgx_cohort_refine: csrc/cluster_kernels.hip k_refine_*, csrc/cohort_cluster.cpp):
the eligibility flags, the stable compaction of both site orders, the second edge pass and component search, the exact 96-bit ratio test and the
alive-aware tally.  Expectations: the literals of tests/refine_cases.py, the library's host twin and the Python restatement of
tests/refine_ref.py, on BOTH matrix paths (the image a finish left in HBM; a matrix uploaded through a cohort that never saw it).  Every
comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import cluster_cases
import cluster_ref
import refine_cases as cases
import refine_ref
from cohort_common import STRANDNESS, cohort_files, table_from_rows  # noqa: F401  (cohort_files is a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "regtools-amd")
RGX_ERR_ARG = 7


def _cohort_of(gpu_ctx, tables, names, **kw):
    import regtools_amd
    co = regtools_amd.Cohort(ctx=gpu_ctx, **kw)
    for t, nm in zip(tables, names):
        co.add(cluster_cases.Sample(t), nm)
    return co


def _both_paths(gpu_ctx, co, m, **kw):
    """refine on the cohort whose finish made m (path 1) and on a second cohort that never saw it (path 0); the two results, compared."""
    import regtools_amd
    a = co.refine(m, **kw)
    assert co.cluster_paths[-1] == 1
    other = regtools_amd.Cohort(ctx=gpu_ctx)
    b = other.refine(m, **kw)
    assert other.cluster_paths == [0]
    refine_ref.same_clusters(a, b)
    assert a.counts_text(m) == b.counts_text(m)
    other.close()
    return a, b


def test_hand_made_cohort_on_both_paths(gpu_ctx):
    from regtools_amd import cohort
    tables = [table_from_rows(cases.HAND_P), table_from_rows(cases.HAND_Q)]
    co = _cohort_of(gpu_ctx, tables, ["p", "q"], only_anchored=False, min_total=0)
    m = co.finish()
    assert [int(x) for x in m.total] == cases.HAND_TOTALS
    for kw, lit in cases.HAND:
        want = refine_ref.refine(m, **kw)
        twin = cohort.refine_host(m, **kw)
        for cl in _both_paths(gpu_ctx, co, m, **kw):
            cases.check_literals(cl, m, lit)
            refine_ref.same(cl, want)
            refine_ref.same_clusters(cl, twin)
            assert cl.counts_text(m) == twin.counts_text(m) == refine_ref.counts_text(m, want) and cl.n_rounds >= 1
    for kw, stays in cases.BOUNDARY:                          # equality passes the ratio test
        for cl in _both_paths(gpu_ctx, co, m, **kw):
            refine_ref.same(cl, refine_ref.refine(m, **kw))
            assert (int(cl.cluster[2]) != cases.NO) == stays, kw
    # identity: default parameters give rgx_cohort_cluster's result, in every array and count
    for kw in (dict(), dict(min_rows=2), dict(min_total=41)):
        a, b = co.refine(m, **kw), co.cluster(m, **kw)
        refine_ref.same_clusters(a, b)
        assert (a.n_ineligible, a.n_weak, a.n_rounds) == (0, 0, b.n_rounds) and a.counts_text(m) == b.counts_text(m)
    co.close()
    cluster_cases.free_tables(tables)


def test_the_ratio_test_is_made_on_the_whole_products(gpu_ctx):
    from regtools_amd import cohort
    tables = [table_from_rows(cases.WIDE_P), table_from_rows(cases.WIDE_Q)]
    co = _cohort_of(gpu_ctx, tables, ["p", "q"], only_anchored=False)
    m = co.finish()
    num, den = cases.WIDE_RATIO
    x, T = int(m.total[0]), int(m.total.sum())
    exact, wrapped = x * den < num * T, (x * den) % 2**64 < (num * T) % 2**64
    assert [int(t) for t in m.total] == [8_000_000_000, 1] and (exact, wrapped) == (False, True)      # mod 2^64, X would be removed too
    want, twin = refine_ref.refine(m, min_ratio=cases.WIDE_RATIO), cohort.refine_host(m, min_ratio=cases.WIDE_RATIO)
    for cl in _both_paths(gpu_ctx, co, m, min_ratio=cases.WIDE_RATIO):
        refine_ref.same(cl, want)
        refine_ref.same_clusters(cl, twin)
        assert cl.n_weak == 1 and [int(c) for c in cl.cluster] == [0, cases.NO] and [int(t) for t in cl.cl_total] == [8_000_000_000]
    co.close()
    cluster_cases.free_tables(tables)


def test_bad_ratios_the_empty_matrix_and_a_cohort_without_samples(gpu_ctx):
    import regtools_amd
    from regtools_amd import RegtoolsError, cohort
    co = regtools_amd.Cohort(ctx=gpu_ctx)
    m = co.finish()
    cl = co.refine(m, max_intron=10, min_reads=3, min_ratio=(1, 2))
    assert (cl.n_rows, cl.n_clusters, cl.n_components, cl.n_ineligible, cl.n_weak, cl.n_rounds) == (0, 0, 0, 0, 0, 0)
    assert list(cl.cl_begin) == [0] and list(cl.cs_begin) == [0] and cl.counts_text(m) == b"chrom\n" and co.cluster_paths == [1]
    # the cohort has no samples; the matrix it refines is somebody else's
    tables = [table_from_rows(cases.HAND_P), table_from_rows(cases.HAND_Q)]
    h = cohort.merge_host([cluster_cases.Sample(t) for t in tables], ["p", "q"], only_anchored=False, min_total=0)
    kw, lit = cases.HAND[1]
    cases.check_literals(co.refine(h, **kw), h, lit)
    assert co.cluster_paths == [1, 0]
    for ratio in ((2, 1), (1, 0)):
        for call in (lambda: co.refine(h, min_ratio=ratio), lambda: cohort.refine_host(h, min_ratio=ratio)):
            with pytest.raises(RegtoolsError) as e:
                call()
            assert e.value.code == RGX_ERR_ARG
    assert co.cluster_paths == [1, 0]                          # a refused call got nowhere
    co.close()
    cluster_cases.free_tables(tables)


@pytest.mark.parametrize("rows", [0] + cases.CHAIN_ROWS)
def test_chains_whose_survivors_sit_on_the_compaction_edges(gpu_ctx, rows):
    """Survivors of the second compaction: 0 (everything ineligible), 1, 63, 64, 65, 4095, 4096, 4097; the last row weak (96, 6144) or alive."""
    from regtools_amd import cohort
    L = rows or 97
    tid, start, end, cls, count = cases.chain(L)
    t = cluster_cases.table_of(0, tid, start, end, count, np.full(L, ord("+"), np.uint32))
    co = _cohort_of(gpu_ctx, [t], ["only"])
    m = co.finish()
    assert m.n == L
    kw = dict(min_reads=cases.CHAIN_MIN_READS) if rows else dict(max_intron=1, min_reads=cases.CHAIN_MIN_READS)
    want, twin = refine_ref.refine(m, **kw), cohort.refine_host(m, **kw)
    for cl in _both_paths(gpu_ctx, co, m, **kw):
        refine_ref.same(cl, want)
        refine_ref.same_clusters(cl, twin)
        if rows:
            assert (cl.n_ineligible, cl.n_weak, int(cl.cl_begin[-1])) == (0, L // 3, cases.chain_survivors(L))
            assert (int(cl.cluster[-1]) == cases.NO) == (L % 3 == 0)
        else:
            assert (cl.n_ineligible, cl.n_weak, cl.n_clusters, cl.n_components) == (L, 0, 0, 0) and list(cl.cl_begin) == [0] and list(cl.cs_begin) == [0]
            assert len(cl.cl_row) == len(cl.cs_sample) == 0 and cl.counts_text(m) == b"chrom only\n"
    co.close()
    cluster_cases.free_tables([t])


# ---- the heavy-tailed random cohort: giant components that the refinement breaks up ------------------------------------------------------
G = 24
# With 24 samples every row's total is at least 34, so the host test's min_reads = 30 would remove nothing by reads; 80 removes 11,282 rows by
# reads only and 41,554 by ratio only (worked out with the restatement), which keeps the assertions of the six-sample case.
REFINE = dict(max_intron=200000, min_reads=80, min_ratio=(1, 100))
FILTERS = [dict(), dict(min_rows=2, min_total=30)]


@pytest.fixture(scope="module")
def heavy_cohort(gpu_ctx):
    """(cohort, its matrix straight behind the finish, the restatement's removal, {filter index: the restatement}, the unrefined clusters)"""
    tid, start, end, cls = cluster_cases.random_junctions()
    tables = cases.heavy_tables(G, tid, start, end, cls)
    co = _cohort_of(gpu_ctx, tables, ["g%02d" % g for g in range(G)])
    m = co.finish()
    assert m.n == len(tid) == 199_998 and np.array_equal(m.start, start) and np.array_equal(m.end, end) and int(m.total.min()) >= 34
    rem = refine_ref.removal(m, **REFINE)
    wants = [refine_ref.clusters_of(m, rem, **kw) for kw in FILTERS]
    first_step = co.cluster(m)
    yield co, m, rem, wants, first_step
    co.close()
    cluster_cases.free_tables(tables)


@pytest.mark.parametrize("which", [0, 1])
def test_heavy_tailed_random_cohort(gpu_ctx, heavy_cohort, which):
    from regtools_amd import cohort
    co, m, rem, wants, first_step = heavy_cohort
    kw, want = dict(REFINE, **FILTERS[which]), wants[which]
    twin = cohort.refine_host(m, **kw)
    a, b = _both_paths(gpu_ctx, co, m, **kw)
    print("heavy-tailed cohort %s: %d ineligible, %d weak (%d by reads only, %d by ratio only), %d components, %d clusters, %d rounds, %.3f ms "
          "(unrefined: %d rounds, %.3f ms)" % (FILTERS[which], a.n_ineligible, a.n_weak, rem["by_reads"], rem["by_ratio"], a.n_components, a.n_clusters,
                                               a.n_rounds, a.ms_cluster, first_step.n_rounds, first_step.ms_cluster))
    for cl in (a, b):
        refine_ref.same(cl, want)
        refine_ref.same_clusters(cl, twin)
    assert a.counts_text(m) == twin.counts_text(m) == refine_ref.counts_text(m, want)
    assert rem["removed_per_round"] == [a.n_weak, 0]
    assert rem["n_ineligible"] >= 5000 and rem["by_reads"] >= 5000 and rem["by_ratio"] >= 5000
    sizes = np.diff(a.cl_begin)
    assert (sizes >= 2).sum() >= 10_000 and sizes.max() < 1024 < np.diff(first_step.cl_begin).max()
    if which == 0:
        # identity on the random cohort: default parameters give the unrefined clusters, in every array and count
        same = co.refine(m)
        refine_ref.same_clusters(same, first_step)
        assert (same.n_ineligible, same.n_weak, same.n_rounds) == (0, 0, first_step.n_rounds)


# ---- the tool ---------------------------------------------------------------------------------------------------------------------------
def _items(samples):
    return [(s["path"], s["name"], dict(strandness=STRANDNESS[s["strand"]])) for s in samples]


def test_the_tool_refines_with_l_J_p(gpu_ctx, cohort_files, tmp_path):  # noqa: F811
    import regtools_amd
    xs = [s for s in cohort_files if s["strand"] == "XS"][:4]
    cx = regtools_amd.Cohort(ctx=gpu_ctx)
    cx.run(_items(xs))
    mx = cx.finish()
    plain = cx.cluster(mx).counts_text(mx)
    # (these four files' junctions share no splice sites -- every cluster is one row -- so -K stays 1; worked out from the oracle's rows: about
    # 2,700 of the 7,259 rows are over 20,000 long and about 3,400 have fewer than 5 reads)
    kw = dict(max_intron=20000, min_reads=5, min_ratio=(1, 100), min_rows=1, min_total=6)
    cl = cx.refine(mx, **kw)
    refined = cl.counts_text(mx)
    refine_ref.same(cl, refine_ref.refine(mx, **kw))
    print("the tool's cohort: %d rows, %d ineligible, %d weak, %d clusters of %d components" % (mx.n, cl.n_ineligible, cl.n_weak, cl.n_clusters, cl.n_components))
    assert cl.n_ineligible > 0 and cl.n_weak > 0 and 0 < cl.n_clusters < cl.n_components and len(plain) > len(refined) > len(plain) // 100
    bed, k = str(tmp_path / "x.bed"), str(tmp_path / "x.clusters")
    paths = [s["path"] for s in xs]
    r = subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-o", bed, "-k", k, "-l", "20000", "-J", "5", "-p", "0.01", "-K", "1", "-T", "6"] + paths,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, REGTOOLS_AMD_STATS="1"))
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert open(k, "rb").read() == refined and open(bed, "rb").read() == mx.bed12()
    assert b"%d rows over the intron limit, %d weak" % (cl.n_ineligible, cl.n_weak) in r.stderr
    # one of the three is enough to refine; without them -k writes what it always wrote
    r = subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-o", bed, "-k", k, "-J", "5"] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(k, "rb").read() == cx.refine(mx, min_reads=5).counts_text(mx)
    r = subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-o", bed, "-k", k] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(k, "rb").read() == plain
    cx.close()
