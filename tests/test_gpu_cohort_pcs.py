"""The principal components of the phenotype table on the device (rgx_cohort_pheno_pcs: csrc/pca_kernels.hip, csrc/cohort_pcs.cpp): the Gram
matrix and the column sums of the table's quantiles in the contract's summation order -- 64 x 64 sample tiles, rows in slabs of 16, up to 64 chunks
of rows -- and the host part behind them.  Expectations: the library's host twin in col_sum, gram, variance and component as bit patterns, and the
restatement of tests/pca_ref.py (exact fused multiply-adds) where that is affordable."""
import os
import subprocess

import numpy as np
import pytest

import cluster_cases
import pca_cases as pca
import pca_ref as ref
import pheno_cases as pc
from pca_ref import C_TOL, check_residual, check_structure, same_bits, same_pcs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "regtools-amd")
RGX_ERR_ARG = 7
EXACT_LIMIT = 100_000                        # fused multiply-adds the Fraction restatement is asked for


@pytest.fixture(scope="module")
def co(gpu_ctx):
    import regtools_amd
    c = regtools_amd.Cohort(ctx=gpu_ctx)
    yield c
    c.close()


def _check(co, rank2, n_pcs=None):
    """Device == twin in every array; device == restatement in gram and col_sum when the table is small."""
    from regtools_amd import cohort
    K, S = rank2.shape
    n_pcs = min(K, S, 3) if n_pcs is None else n_pcs
    ph = cohort.pheno_table_from_rank2(rank2)
    dev, twin = co.pheno_pcs(ph, n_pcs), cohort.pheno_pcs_host(ph, n_pcs)
    same_pcs(dev, twin)
    check_structure(dev)
    if K * S * (S + 1) // 2 <= EXACT_LIMIT:
        gram, col = ref.gram_exact(ref.quantiles(rank2, cohort.quantile))
        same_bits(dev.gram, gram)
        same_bits(dev.col_sum, col)
    return dev


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 129])
def test_sample_counts_around_the_tile(co, S):
    """One tile with one sample, a full one, one sample into the second and into the third (six tile pairs); 41 rows: two slabs and 9 rows."""
    _check(co, pca.random_rank2(41, S, seed=S))


def test_three_samples(co):
    """S = 3: gram's 72 bytes are no multiple of 16, and gram, col_sum and the flag word still come back in one piece (every component asked for)."""
    dev = _check(co, pca.random_rank2(41, 3, seed=3), n_pcs=3)
    assert dev.gram.shape == (3, 3) and dev.col_sum.ctypes.data == dev.gram.ctypes.data + 72


@pytest.mark.parametrize("K", [2, 15, 16, 17, 33])
def test_row_counts_around_the_slab(co, K):
    _check(co, pca.random_rank2(K, 5, seed=K))


@pytest.mark.parametrize("K", [1024, 1025, 65536, 65537])
def test_row_counts_around_the_chunks(co, K):
    """One chunk, then two (513 + 512); 64 chunks of 1024 rows, then 63 of 1025 and one of 962."""
    assert len(ref.chunks(K)) == {1024: 1, 1025: 2, 65536: 64, 65537: 64}[K]
    _check(co, pca.random_rank2(K, 3, seed=K))


@pytest.mark.parametrize("K, S, n_f, ties", [(1025, 9, 4, True), (2000, 129, 6, True)])
def test_planted_tables_with_ties(co, K, S, n_f, ties):
    p = _check(co, pca.shape(K, S, n_f, ties), n_pcs=n_f)
    check_residual(p, C_TOL * S * ref.EPS * p.variance[0])


def test_larger_run(co):
    """70,001 rows of 32 samples: 2.2 M entries in 64 uneven chunks (63 of 1094 rows and one of 1079)."""
    assert ref.chunks(70_001)[-2:] == [(67_828, 68_922), (68_922, 70_001)]
    p = _check(co, pca.random_rank2(70_001, 32, seed=70), n_pcs=10)
    print("70001 x 32: %.3f ms, gram %.3f ms, eigen %.3f ms" % (p.ms_pcs, p.ms_gram, p.ms_eigen))


def test_full_path_on_both_matrix_paths(gpu_ctx):
    """finish -> refine -> phenotypes -> pheno_pcs with the matrix still in HBM, and from a merge_host matrix with the twin's clusters."""
    import regtools_amd
    from regtools_amd import cohort
    S = 9
    tables = pc.tables(pc.counts(S, 301, seed=11, absent=0.2))
    refine = dict(max_intron=100000, min_reads=2, min_ratio=(1, 1000))
    kw = dict(max_missing=(1, 1), min_sd=0.0)
    c = regtools_amd.Cohort(ctx=gpu_ctx)
    for t, nm in zip(tables, pc.names(S)):
        c.add(cluster_cases.Sample(t), nm)
    m = c.finish()
    cl = c.refine(m, **refine)
    ph = c.phenotypes(m, cl, **kw)
    assert c.cluster_paths[-2:] == [1, 1]
    a = c.pheno_pcs(ph, 5)
    h = cohort.merge_host([cluster_cases.Sample(t) for t in tables], pc.names(S))
    clh = cohort.refine_host(h, **refine)
    phb = c.phenotypes(h, clh, **kw)
    assert c.cluster_paths[-1] == 0
    b = c.pheno_pcs(phb, 5)
    twin = cohort.pheno_pcs_host(cohort.phenotypes_host(h, clh, **kw), 5)
    assert twin.n_rows == ph.n_rows >= 250
    same_pcs(a, twin)
    same_pcs(b, twin)
    check_structure(a)
    check_residual(a, C_TOL * S * ref.EPS * a.variance[0])
    assert a.text(m) == b.text(h) == twin.text(h) == ref.text(m.sample_name, twin.component)
    c.close()
    cluster_cases.free_tables(tables)


def test_errors(co):
    from regtools_amd import RegtoolsError, cohort
    r2 = pca.random_rank2(40, 70, seed=5)

    def refused(rank2, n_pcs):
        with pytest.raises(RegtoolsError) as e:
            co.pheno_pcs(cohort.pheno_table_from_rank2(rank2), n_pcs)
        assert e.value.code == RGX_ERR_ARG, (rank2.shape, n_pcs)
    # judged on the host, before any launch
    refused(r2[:1], 1)
    refused(np.zeros((40, 0), np.uint32), 1)
    refused(r2, 0)
    refused(r2, 41)
    refused(np.full((2, 2049), 2, np.uint32), 1)
    # noticed by the device's gather and reported through its flag: first and last entry, both tiles, both sides of the range
    for (k, s), bad in (((0, 0), 1), ((39, 69), 81), ((17, 64), 0), ((20, 3), 0xffffffff)):
        b = r2.copy()
        b[k, s] = bad
        refused(b, 2)
    # the cohort is none the worse for it
    _check(co, r2, n_pcs=2)


# (seed, reads): the six files over ONE gene model of tests/test_gpu_cohort_pheno.py, whose clusters have several rows
GENE_FILES = [(5, 20000), (5, 30000), (5, 45000), (5, 60000), (5, 25000), (5, 52000)]


def test_the_tool_writes_the_components(gpu_ctx, tmp_path):
    import regtools_amd
    from regtools_amd import cohort, synth
    paths = []
    for k, (seed, n_reads) in enumerate(GENE_FILES):
        paths.append(str(tmp_path / ("g%d.bam" % k)))
        synth.write(paths[-1], n_reads, shape="short", seed=seed, n_genes=300)
        if not os.path.exists(paths[-1] + ".bai"):
            synth.index(paths[-1])
    c = regtools_amd.Cohort(ctx=gpu_ctx)
    c.run([(p, "g%d" % k, dict(strandness=0)) for k, p in enumerate(paths)])
    m = c.finish()
    bed, q, pcs = str(tmp_path / "x.bed"), str(tmp_path / "x.pheno"), str(tmp_path / "x.PCs")

    def run(*args):
        return subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-o", bed] + list(args) + paths, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, env=dict(os.environ, REGTOOLS_AMD_STATS="1"))
    cl = cohort.cluster_host(m)
    ph = cohort.phenotypes_host(m, cl)
    assert ph.n_rows >= 100 and ph.n_samples == 6
    # -P alone computes the table as -q would and does not write it; the default of ten components is clipped to the six samples
    twin = cohort.pheno_pcs_host(ph, 6)
    r = run("-P", pcs)
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert open(pcs, "rb").read() == twin.text(m) == ref.text(m.sample_name, twin.component) and not os.path.exists(q)
    assert b"pcs: %d rows, 6 samples, 6 components written" % ph.n_rows in r.stderr
    # beside -q, with -C
    twin = cohort.pheno_pcs_host(ph, 2)
    r = run("-P", pcs, "-q", q, "-C", "2")
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert open(pcs, "rb").read() == twin.text(m) and open(q, "rb").read() == ph.text(m, cl)
    assert b"pcs: %d rows, 6 samples, 2 components written" % ph.n_rows in r.stderr
    # a table without rows (no deviation reaches 9): the file is its header line
    r = run("-P", pcs, "-d", "9")
    assert r.returncode == 0 and open(pcs, "rb").read() == b"id\tg0\tg1\tg2\tg3\tg4\tg5\n"
    # a count that does not parse: status 1, nothing written
    for f in (bed, q, pcs):
        os.remove(f)
    for bad in ("0", "-3", "2.5", "ten", ""):
        r = run("-P", pcs, "-q", q, "-C", bad)
        assert r.returncode == 1 and b"Unrecognized component count argument!" in r.stderr, bad
        assert not os.path.exists(pcs) and not os.path.exists(q) and not os.path.exists(bed)
    c.close()
