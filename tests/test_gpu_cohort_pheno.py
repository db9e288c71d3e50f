"""The splicing phenotype table of a clustered cohort on the device (rgx_cohort_phenotypes: csrc/pheno_kernels.hip, csrc/cohort_pheno.cpp): the
row statistics in the contract's summation order (a wave per row, eight lanes from eight samples down), the scan and scatter of the kept rows, the
one stable sort of the table's entries and the ranks from its tie runs.  Expectations: the library's host twin and the numpy restatement of
tests/pheno_ref.py, on BOTH matrix paths (the image a finish left in HBM with the device's own clusters; a merge_host matrix with the twin's
clusters, uploaded).  Integers are compared exactly, mean and sd as bit patterns."""
import os
import subprocess

import numpy as np
import pytest

import cluster_cases
import pheno_cases as pc
import pheno_ref
import refine_cases
from cohort_common import cohort_files  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "regtools-amd")
RGX_ERR_ARG = 7


def _both_paths(gpu_ctx, tables, names, refine=None, cohort_kw=None, text=True, **kw):
    """The table of the cohort of `tables` four ways: on the device straight behind the finish (path 1, the device's clusters), on the device from a
    merge_host matrix (path 0, the twin's clusters), by the twin and by the restatement; text: also as text.  Returns (device table, restatement, matrix, clusters)."""
    import regtools_amd
    from regtools_amd import cohort
    cohort_kw = cohort_kw or {}
    co = regtools_amd.Cohort(ctx=gpu_ctx, **cohort_kw)
    for t, nm in zip(tables, names):
        co.add(cluster_cases.Sample(t), nm)
    m = co.finish()
    cl = co.refine(m, **refine) if refine else co.cluster(m)
    a = co.phenotypes(m, cl, **kw)
    assert co.cluster_paths[-2:] == [1, 1]
    h = cohort.merge_host([cluster_cases.Sample(t) for t in tables], names, **cohort_kw)
    clh = cohort.refine_host(h, **refine) if refine else cohort.cluster_host(h)
    b = co.phenotypes(h, clh, **kw)
    assert co.cluster_paths[-1] == 0
    twin, want = cohort.phenotypes_host(h, clh, **kw), pheno_ref.phenotypes(h, clh, **kw)
    for ph in (a, b):
        pheno_ref.same_tables(ph, twin)
        pheno_ref.same(ph, want)
    if text:
        assert a.text(m, cl) == b.text(h, clh) == twin.text(h, clh)
    co.close()
    return a, want, m, cl


def _shape(gpu_ctx, S, n_rows, seed=None, **kw):
    count = pc.counts(S, n_rows, seed=S * 1000 + n_rows if seed is None else seed, **kw)
    tables = pc.tables(count)
    try:
        return _both_paths(gpu_ctx, tables, pc.names(S), max_missing=(1, 1), min_sd=0.0)[:2]
    finally:
        cluster_cases.free_tables(tables)


@pytest.mark.parametrize("S", [1, 8, 9, 63, 64, 65, 129])
def test_sample_counts_around_the_wave(gpu_ctx, S):
    """One to three trips of a wave's strided loop, and the eight-lane form (S <= 8); missing entries, an empty sample column and equal rows."""
    count = pc.counts(S, 41, seed=S, absent=0.3, empty_clusters=[(0, 0, 3)], duplicates=2)
    tables = pc.tables(count)
    for kw in (dict(), dict(max_missing=(1, 1), min_sd=0.0)):
        ph, want, _, _ = _both_paths(gpu_ctx, tables, pc.names(S), **kw)
        assert (ph.n_rows > 0) == (S > 1)                    # one sample: every row is its own mean and none is kept -- no later launch
    cluster_cases.free_tables(tables)


# K * S on and around the radix sort's tiles (512 entries up to 2,097,152, 2048 above) and the scan's (4096); every row is kept
@pytest.mark.parametrize("S, n_rows", [(23, 89), (8, 256), (64, 32), (3, 683), (7, 73), (8, 64), (19, 27), (17, 241), (3, 4097)])
def test_entry_counts_around_the_tiles(gpu_ctx, S, n_rows):
    ph, want = _shape(gpu_ctx, S, n_rows)
    assert ph.n_rows == n_rows and ph.n_rows * S in (2047, 2048, 2049, 511, 512, 513, 4097, 12291)


def test_tie_runs_across_tile_boundaries_and_a_column_that_is_one_tie(gpu_ctx):
    """3,000 rows of five samples: sample 1 has no reads at all -- its column of 3,000 entries is one run -- and sample 2 none in five clusters of
    six: a run of 2,500 equal values that lies across several tiles of the sort and of the head scan."""
    ph, want = _shape(gpu_ctx, 5, 3000, empty_clusters=[(1, 0, 1), (2, 0, 6), (2, 1, 6), (2, 2, 6), (2, 3, 6), (2, 4, 6)])
    assert ph.n_rows == 3000 and (ph.rank2[:, 1] == 3001).all()
    runs = np.unique(ph.rank2[:, 2], return_counts=True)[1]
    assert runs.max() == 2500


def test_large_sort_tiles(gpu_ctx):
    """70,000 rows of 32 samples: 2,240,000 entries, above the size from which the sort takes tiles of 2048; sample 0 has no reads in two
    clusters of three (a run of 46,668 equal values across those tiles)."""
    count = pc.counts(32, 70_000, seed=32, empty_clusters=[(0, 0, 3), (0, 1, 3)])
    tables = pc.tables(count)
    ph, want = _both_paths(gpu_ctx, tables, pc.names(32), text=False, max_missing=(1, 1), min_sd=0.0)[:2]
    cluster_cases.free_tables(tables)
    assert ph.n_rows == 70_000 and np.unique(ph.rank2[:, 0], return_counts=True)[1].max() == 46_668


def test_one_row_kept_and_no_row_kept(gpu_ctx):
    tables = pc.tables(pc.ONE_KEPT)
    ph, want, _, _ = _both_paths(gpu_ctx, tables, pc.names(3))
    assert ph.row.tolist() == [0] and ph.n_drop_sd == 1 and ph.rank2.tolist() == [[2, 2, 2]]
    ph, want, _, _ = _both_paths(gpu_ctx, tables, pc.names(3), min_sd=0.5)
    assert (ph.n_rows, ph.n_clustered, ph.n_drop_na, ph.n_drop_sd) == (0, 2, 0, 2) and ph.rank2.shape == (0, 3)
    cluster_cases.free_tables(tables)


def test_argument_errors_empty_inputs_and_a_cohort_without_samples(gpu_ctx):
    import regtools_amd
    from regtools_amd import RegtoolsError, cohort
    co = regtools_amd.Cohort(ctx=gpu_ctx)
    m = co.finish()
    cl = co.cluster(m)
    ph = co.phenotypes(m, cl)
    assert (ph.n_rows, ph.n_samples, ph.n_clustered, ph.n_drop_na, ph.n_drop_sd) == (0, 0, 0, 0, 0) and ph.text(m, cl) == b"#Chr\tstart\tend\tID\n"
    # the cohort has no samples; the matrix and the clusters are somebody else's
    tables = pc.tables(pc.counts(3, 6, seed=1))
    h = cohort.merge_host([cluster_cases.Sample(t) for t in tables], pc.names(3))
    clh, none = cohort.cluster_host(h), cohort.cluster_host(h, min_rows=99)
    pheno_ref.same(co.phenotypes(h, clh), pheno_ref.phenotypes(h, clh))
    ph = co.phenotypes(h, none)                              # rows, but none with a cluster: no launch
    assert (ph.n_rows, ph.n_samples, ph.n_clustered) == (0, 3, 0) and ph.rank2.shape == (0, 3)
    paths = list(co.cluster_paths)
    for kw in (dict(max_missing=(1, 0)), dict(max_missing=(3, 2)), dict(min_sd=-0.001), dict(min_sd=float("nan"))):
        with pytest.raises(RegtoolsError) as e:
            co.phenotypes(h, clh, **kw)
        assert e.value.code == RGX_ERR_ARG, kw
    with pytest.raises(RegtoolsError) as e:                  # the clusters of another matrix
        co.phenotypes(h, cl)
    assert e.value.code == RGX_ERR_ARG
    clh.cluster[0] = clh.n_clusters                          # a cluster number the result does not have: refused, not looked up
    with pytest.raises(RegtoolsError) as e:
        co.phenotypes(h, clh)
    assert e.value.code == RGX_ERR_ARG
    clh.cluster[0] = 0
    h._h.contents.n_samples = 1 << 30                        # past 2^32 - 2^16 entries: refused before a launch
    with pytest.raises(RegtoolsError) as e:
        co.phenotypes(h, clh)
    assert e.value.code == RGX_ERR_ARG
    h._h.contents.n_samples = 3
    assert co.cluster_paths == paths                          # a refused call got nowhere
    co.close()
    cluster_cases.free_tables(tables)


# ---- the refined heavy-tailed random cohort of tests/test_gpu_cohort_refine.py: 199,998 rows of 24 samples ---------------------------------
def test_refined_heavy_tailed_random_cohort(gpu_ctx):
    G = 24
    tid, start, end, cls = cluster_cases.random_junctions()
    tables = refine_cases.heavy_tables(G, tid, start, end, cls)
    refine = dict(max_intron=200000, min_reads=80, min_ratio=(1, 100), min_rows=2, min_total=30)
    # (the text of 59,650 rows is 31 MB and seconds of printf per copy: the smaller cohorts compare it)
    ph, want, m, cl = _both_paths(gpu_ctx, tables, ["g%02d" % g for g in range(G)], refine=refine, text=False)
    print("heavy-tailed cohort: %d rows, %d clustered, %d dropped as missing, %d as flat, %d kept, %.3f ms (refine: %.3f ms)" % (
        m.n, ph.n_clustered, ph.n_drop_na, ph.n_drop_sd, ph.n_rows, ph.ms_pheno, cl.ms_cluster))
    assert m.n == 199_998 and (ph.n_clustered, ph.n_drop_na, ph.n_drop_sd, ph.n_rows) == (63_663, 4_013, 0, 59_650)      # (worked out with the twin)
    cluster_cases.free_tables(tables)


# ---- the tool ---------------------------------------------------------------------------------------------------------------------------
def test_the_tool_writes_the_table(gpu_ctx, cohort_files, tmp_path):  # noqa: F811
    import regtools_amd
    from regtools_amd import cohort
    co = regtools_amd.Cohort(ctx=gpu_ctx)
    co.run([(s["path"], s["name"], dict(strandness=0)) for s in cohort_files])
    m = co.finish()
    paths = [s["path"] for s in cohort_files]
    bed, q, k = str(tmp_path / "x.bed"), str(tmp_path / "x.pheno"), str(tmp_path / "x.clusters")

    def run(*args):
        return subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-o", bed] + list(args) + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              env=dict(os.environ, REGTOOLS_AMD_STATS="1"))
    # -q alone clusters as -k would; the twin's formatter over the twin's clusters is the expectation
    cl = cohort.cluster_host(m)
    twin = cohort.phenotypes_host(m, cl)
    r = run("-q", q)
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert open(q, "rb").read() == twin.text(m, cl) and open(bed, "rb").read() == m.bed12() and not os.path.exists(k)
    assert b"phenotypes: %d rows kept of %d clustered, %d dropped as missing, %d as flat" % (
        twin.n_rows, twin.n_clustered, twin.n_drop_na, twin.n_drop_sd) in r.stderr
    print("the tool's cohort: %d rows, %d clustered, %d kept by default" % (m.n, twin.n_clustered, twin.n_rows))
    # with the refinement's and the table's own options, beside -k
    kw = dict(max_intron=20000, min_reads=5, min_ratio=(1, 100), min_rows=2, min_total=6)
    rc = cohort.refine_host(m, **kw)
    twin = cohort.phenotypes_host(m, rc, max_missing=(1, 2), min_sd=0.01)
    r = run("-q", q, "-k", k, "-l", "20000", "-J", "5", "-p", "0.01", "-K", "2", "-T", "6", "-x", "0.5", "-d", "0.01")
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert open(q, "rb").read() == twin.text(m, rc) and open(k, "rb").read() == rc.counts_text(m)
    print("  refined: %d clustered, %d dropped as missing, %d as flat, %d kept" % (twin.n_clustered, twin.n_drop_na, twin.n_drop_sd, twin.n_rows))
    # (these files' junctions share no splice sites: every cluster is one row, whose ratio is 1 wherever it is present, so no row is kept and
    # the table is its header line.  Tables with rows are compared as text in _both_paths above.)
    assert b"phenotypes: %d rows kept of %d clustered, %d dropped as missing, %d as flat" % (
        twin.n_rows, twin.n_clustered, twin.n_drop_na, twin.n_drop_sd) in r.stderr
    # a value that does not parse: status 1, nothing written
    for f in (bed, q, k):
        os.remove(f)
    for args, msg in ((("-x", "1.5"), b"Unrecognized ratio argument!"), (("-d", "-1"), b"Unrecognized deviation argument!")):
        r = run("-q", q, *args)
        assert r.returncode == 1 and msg in r.stderr and not os.path.exists(q) and not os.path.exists(bed)
    co.close()


# (seed, reads): six files over ONE gene model (synth's n_genes: introns between the exons of a gene, some with novel donors), so that junctions
# share donors and acceptors and clusters have several rows -- the ten files above have none
GENE_FILES = [(5, 20000), (5, 30000), (5, 45000), (5, 60000), (5, 25000), (5, 52000)]


def test_the_tool_writes_a_table_with_rows(gpu_ctx, tmp_path):
    import regtools_amd
    from regtools_amd import cohort, synth
    paths = []
    for k, (seed, n_reads) in enumerate(GENE_FILES):
        paths.append(str(tmp_path / ("g%d.bam" % k)))
        synth.write(paths[-1], n_reads, shape="short", seed=seed, n_genes=300)
        if not os.path.exists(paths[-1] + ".bai"):
            synth.index(paths[-1])
    co = regtools_amd.Cohort(ctx=gpu_ctx)
    co.run([(p, "g%d" % k, dict(strandness=0)) for k, p in enumerate(paths)])
    m = co.finish()
    bed, q = str(tmp_path / "x.bed"), str(tmp_path / "x.pheno")

    def run(*args):
        return subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-o", bed, "-q", q] + list(args) + paths, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, env=dict(os.environ, REGTOOLS_AMD_STATS="1"))
    cl = cohort.cluster_host(m)
    twin = cohort.phenotypes_host(m, cl)
    r = run()
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    text = open(q, "rb").read()
    assert text == twin.text(m, cl) == pheno_ref.text(m, cl, twin, cohort.quantile) and text.count(b"\n") == 1 + twin.n_rows
    print("gene-model cohort: %d rows, %d clusters, %d clustered, %d dropped as missing, %d as flat, %d kept" % (
        m.n, cl.n_clusters, twin.n_clustered, twin.n_drop_na, twin.n_drop_sd, twin.n_rows))
    assert twin.n_rows >= 100                                # (753 of 1,713 rows, worked out with the oracle's junctions and the twin)
    kw = dict(max_intron=100000, min_reads=5, min_ratio=(1, 100), min_rows=2, min_total=6)
    rc = cohort.refine_host(m, **kw)
    twin = cohort.phenotypes_host(m, rc, max_missing=(1, 2), min_sd=0.01)
    r = run("-l", "100000", "-J", "5", "-p", "0.01", "-K", "2", "-T", "6", "-x", "0.5", "-d", "0.01")
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert open(q, "rb").read() == twin.text(m, rc) and twin.n_rows >= 100                     # (277 rows kept of 285 clustered)
    assert b"phenotypes: %d rows kept of %d clustered, %d dropped as missing, %d as flat" % (
        twin.n_rows, twin.n_clustered, twin.n_drop_na, twin.n_drop_sd) in r.stderr
    co.close()
