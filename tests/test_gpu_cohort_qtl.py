"""The nominal cis-sQTL scan on the device (rgx_cohort_qtl_nominal: csrc/qtl_kernels.hip, csrc/cohort_qtl.cpp): residuals a wave per row and per
variant, the usable variants compacted, rows in blocks of 64 against tiles of 64 usable variants, samples in slabs of 16.  Expectations: the
library's host twin in every array of the result as bit patterns, and the restatement of tests/qtl_ref.py (exact fused multiply-adds) where that
is affordable."""
import os
import subprocess

import numpy as np
import pytest

import cluster_cases
import pheno_cases as pc
import qtl_cases as qc
import qtl_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "regtools-amd")
RGX_ERR_ARG = 7


@pytest.fixture(scope="module")
def co(gpu_ctx):
    import regtools_amd
    c = regtools_amd.Cohort(ctx=gpu_ctx)
    yield c
    c.close()


def _check(co, c, **kw):
    """Device == twin in every array.  Returns both (the arrays are views: the results must outlive what is read from them)."""
    from regtools_amd import cohort
    a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window)
    a.update(kw)
    ph = cohort.pheno_table_from_rank2(c.rank2)
    dev, twin = co.qtl_nominal(ph, **a), cohort.qtl_nominal_host(ph, **a)
    assert (dev.n_rows, dev.n_samples, dev.n_variants, dev.n_cov, dev.dof) == (twin.n_rows, twin.n_samples, twin.n_variants, twin.n_cov, twin.dof)
    assert (dev.n_constant, dev.n_explained, dev.n_flat_rows) == (twin.n_constant, twin.n_explained, twin.n_flat_rows)
    ref.same_result(dev, twin)
    return dev, twin


S_SWEEP = [(S, n) for S in (4, 15, 16, 17, 63, 64, 65, 129) for n in sorted({0, 1, S - 3} if S <= 17 else {0, 1})]


@pytest.mark.parametrize("S, n_cov", S_SWEEP)
def test_sample_counts_around_the_slab_and_the_partials(co, S, n_cov):
    """One slab short of a sample, full, one sample over; the 64 partials likewise; every degree of freedom down to 1."""
    dev, _ = _check(co, qc.planted(S, 20, 24, n_cov, seed=S * 100 + n_cov))
    assert dev.n_pairs > 0 and dev.dof == S - n_cov - 2


@pytest.mark.parametrize("K", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 200])
def test_row_blocks_and_variant_tiles(co, K, V):
    """One and several row blocks against one and several tiles of usable variants; a row reaches about half of its contig's variants.  (A table
    of ONE row has one rank, so one quantile in every sample: the row is flat and pairs with nothing.)"""
    dev, _ = _check(co, qc.simple(9, K, V, 1, seed=K * 1000 + V, span=4 * qc.WINDOW, contigs=1))
    assert (dev.variant_verdict == 0).all() and (dev.n_pairs > 0 if K > 1 else dev.n_flat_rows == 1)
    if V == 200 and K > 1:
        assert np.diff(dev.pair_begin.astype(np.int64)).max() > 64      # (a row's pairs span tiles)


def test_the_most_samples(co):
    """S = 2048, the contract's limit: the residual kernels' four vectors fill 64 KiB of LDS, the product kernel walks 128 slabs."""
    dev, _ = _check(co, qc.planted(2048, 6, 9, 2, seed=2048))
    assert dev.n_pairs > 0 and dev.dof == 2044


def test_a_row_block_that_spans_a_contig_boundary(co):
    c = qc.simple(9, 64, 130, 0, seed=77, span=4 * qc.WINDOW, contigs=2)
    assert len(set(c.regions[:, 0])) == 2                               # (the one block has rows of both contigs)
    dev, _ = _check(co, c)
    on = [int((c.var_tid == t).sum()) for t in (0, 1)]
    assert dev.n_pairs > 0 and min(on) > 0
    # no row pairs with a variant of the other contig
    row_of = np.repeat(np.arange(64), np.diff(dev.pair_begin.astype(np.int64)))
    assert (c.var_tid[dev.pair_variant] == c.regions[row_of, 0]).all()


@pytest.mark.parametrize("window", [0, 0xffffffff])
def test_the_narrowest_and_the_widest_window(co, window):
    c = qc.case(65, 40, 40, 3)
    dev, _ = _check(co, c, window=window)
    assert dev.n_pairs > 0
    if window:
        usable_on = [int(((c.var_tid == t) & (dev.variant_verdict == 0)).sum()) for t in c.regions[:, 0]]
        assert list(np.diff(dev.pair_begin.astype(np.int64))) == usable_on


def test_tables_without_pairs(co):
    c = qc.case(30, 20, 24, 2)
    dev, _ = _check(co, c, var_tid=np.zeros(0, np.uint32), var_pos=np.zeros(0, np.uint32), dosage=np.zeros((0, 30), np.int8))
    assert dev.n_pairs == 0 and dev.n_variants == 0 and (dev.best == ref.NO_PAIR).all()
    dev, _ = _check(co, c, dosage=np.where(np.arange(24)[:, None] % 2, -1, 2) * np.ones((24, 30), np.int8))
    assert dev.n_pairs == 0 and dev.n_constant == 24 and (dev.best == ref.NO_PAIR).all()
    r2 = c.rank2.copy()
    r2[3] = 20                                                          # a flat row
    dev, _ = _check(co, qc.Case(**dict(c.__dict__, rank2=r2)))
    assert dev.n_flat_rows == 1 and dev.best[3] == ref.NO_PAIR and dev.n_pairs > 0


@pytest.mark.parametrize("S, K, V, n_cov", qc.PLANTED)
def test_planted_cases(co, S, K, V, n_cov):
    from regtools_amd import cohort
    c = qc.case(S, K, V, n_cov)
    dev, _ = _check(co, c)
    qc.check_conditions(c, dev)
    ref.same_result(dev, ref.restate(c, cohort.quantile))


def test_larger_run(co):
    """4,000 rows x 6,000 variants x 64 samples under a window that gives a row some eighty pairs: 63 row blocks, several tiles each."""
    from regtools_amd import cohort
    c = qc.planted(64, 4000, 6000, 3, seed=4064, window=20000, span=3_000_000)
    dev, _ = _check(co, c)
    qc.check_conditions(c, dev)
    assert dev.n_pairs > 100_000
    print("4000 x 6000 x 64: %d pairs, %.3f ms, residuals %.3f ms, pairs %.3f ms" % (dev.n_pairs, dev.ms_qtl, dev.ms_residual, dev.ms_pairs))
    Q = ref.basis(c.S, c.cov)
    c._T = ref.quantile_table(c.K, cohort.quantile)
    row_of = np.repeat(np.arange(c.K), np.diff(dev.pair_begin.astype(np.int64)))
    for p in np.random.default_rng(1).integers(0, dev.n_pairs, 24):
        k, v = int(row_of[p]), int(dev.pair_variant[p])
        ref.same_bits([dev.yy[k], dev.gg[v], dev.r[p], dev.slope[p]], list(ref.restate_pair(c, cohort.quantile, k, v, Q)))


def test_full_path_on_both_matrix_paths(gpu_ctx):
    """finish -> refine -> phenotypes -> pheno_pcs -> qtl_nominal with the matrix still in HBM, and from a merge_host matrix with the twin's
    clusters."""
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
    pcs = c.pheno_pcs(ph, 3)
    regions = cohort.pheno_regions(m, ph)
    tid, pos, dosage = qc.variants_near(regions, S, 400, seed=12)
    ids = ["v%d" % i for i in range(400)]
    a = c.qtl_nominal(ph, regions, tid, pos, dosage, pcs.component, qc.WINDOW)
    h = cohort.merge_host([cluster_cases.Sample(t) for t in tables], pc.names(S))
    clh = cohort.refine_host(h, **refine)
    phb = c.phenotypes(h, clh, **kw)
    pcs_b = c.pheno_pcs(phb, 3)                                        # (component is a view: the object must outlive the call)
    b = c.qtl_nominal(phb, cohort.pheno_regions(h, phb), tid, pos, dosage, pcs_b.component, qc.WINDOW)
    pht = cohort.phenotypes_host(h, clh, **kw)
    pcs_t = cohort.pheno_pcs_host(pht, 3)
    twin = cohort.qtl_nominal_host(pht, cohort.pheno_regions(h, pht), tid, pos, dosage, pcs_t.component, qc.WINDOW)
    assert twin.n_rows == ph.n_rows >= 250 and twin.n_pairs > 1000
    ref.same_result(a, twin)
    ref.same_result(b, twin)
    pheno_ids = [line.split(b"\t")[3].decode() for line in pht.text(h, clh).split(b"\n")[1:-1]]
    want = ref.text(pheno_ids, ids, pos, regions[:, 1], twin, cohort.qtl_tstat, cohort.qtl_pvalue)
    assert a.text(m, cl, ph, pos, ids) == b.text(h, clh, phb, pos, ids) == twin.text(h, clh, pht, pos, ids) == want
    c.close()
    cluster_cases.free_tables(tables)


def test_errors(co):
    from regtools_amd import RegtoolsError, cohort
    c = qc.case(65, 40, 40, 3)

    def refused(**kw):
        a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window, rank2=c.rank2)
        a.update(kw)
        rank2 = a.pop("rank2")
        with pytest.raises(RegtoolsError) as e:
            co.qtl_nominal(cohort.pheno_table_from_rank2(rank2), **a)
        assert e.value.code == RGX_ERR_ARG, kw.keys()
        return str(e.value)
    # judged on the host, before any launch
    refused(rank2=np.zeros((0, 65), np.uint32), regions=np.zeros((0, 3), np.uint32))
    refused(covariates=np.random.default_rng(1).standard_normal((63, 65)))
    refused(var_pos=c.var_pos[::-1].copy())
    assert "covariate 2" in refused(covariates=np.stack([c.cov[0], c.cov[0]]))
    # noticed by the device and reported through its flag words: the first and the last entry, both sides of the range
    for at, bad in (((0, 0), 3), ((39, 64), -2), ((0, 0), -128), ((39, 64), 127)):
        d = c.dosage.copy()
        d[at] = bad
        assert "dosage" in refused(dosage=d)
    for at, bad in (((0, 0), 1), ((39, 64), 81), ((0, 0), 0), ((39, 64), 0xffffffff)):
        r2 = c.rank2.copy()
        r2[at] = bad
        assert "rank2" in refused(rank2=r2)
    # the cohort is none the worse for it
    _check(co, c)


def test_more_pairs_than_the_result_can_index(co):
    """65,537 rows x 65,536 usable variants on one contig under the widest window: 2^32 + 2^16 pairs, known behind the plan and refused there."""
    from regtools_amd import RegtoolsError, cohort
    K, V, S = 65537, 65536, 3
    rng = np.random.default_rng(8)
    rank2 = (2 * (np.argsort(rng.random((K, S)), axis=0) + 1)).astype(np.uint32)
    regions = np.tile(np.array([[0, 5, 9]], np.uint32), (K, 1))
    dosage = np.tile(np.array([[0, 1, 2]], np.int8), (V, 1))
    with pytest.raises(RegtoolsError) as e:
        co.qtl_nominal(cohort.pheno_table_from_rank2(rank2), regions, np.zeros(V, np.uint32), np.arange(1, V + 1, dtype=np.uint32), dosage, None,
                       0xffffffff)
    assert e.value.code == RGX_ERR_ARG and "4295032832 pairs" in str(e.value)
    _check(co, qc.case(12, 9, 16, 0))


# (seed, reads): the six files over ONE gene model of tests/test_gpu_cohort_pheno.py, whose clusters have several rows
GENE_FILES = [(5, 20000), (5, 30000), (5, 45000), (5, 60000), (5, 25000), (5, 52000)]


def test_the_tool_scans_the_variants_of_a_vcf(gpu_ctx, tmp_path):
    import gzip
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
    cl = cohort.cluster_host(m)
    ph = cohort.phenotypes_host(m, cl)
    assert ph.n_rows >= 100 and ph.n_samples == 6
    regions = cohort.pheno_regions(m, ph)
    vcf, bed, q, pcs, out = (str(tmp_path / n) for n in ("v.vcf", "x.bed", "x.pheno", "x.PCs", "x.qtl"))
    # the file's samples: the cohort's in another order, and one more
    tid, pos, dosage, ids, skipped = qc.write_vcf(vcf, m, regions, 330, seed=6, samples=["g0", "g5", "other", "g3", "g1", "g4", "g2"])
    g = cohort.genotypes(vcf, m)
    assert np.array_equal(g.tid, tid) and np.array_equal(g.pos, pos) and np.array_equal(g.dosage, dosage) and [i.decode() for i in g.ids] == ids
    assert (g.n_records, [g.n_multiallelic, g.n_no_gt, g.n_unknown_contig]) == (330, skipped) and min(skipped) > 0
    assert (np.diff(pos.astype(np.int64))[np.diff(tid.astype(np.int64)) == 0] >= 0).all() and set(np.unique(dosage)) == {-1, 0, 1, 2}

    def run(*args):
        return subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-o", bed] + list(args) + paths, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, env=dict(os.environ, REGTOOLS_AMD_STATS="1"))

    def expected(n_cov, window):
        pcs_t = cohort.pheno_pcs_host(ph, n_cov) if n_cov else None    # (component is a view: the object must outlive the call)
        twin = cohort.qtl_nominal_host(ph, regions, tid, pos, dosage, pcs_t.component if n_cov else None, window)
        assert twin.n_pairs > 100
        text = twin.text(m, cl, ph, pos, ids)
        pheno_ids = [line.split(b"\t")[3].decode() for line in ph.text(m, cl).split(b"\n")[1:-1]]
        assert text == ref.text(pheno_ids, ids, pos, regions[:, 1], twin, cohort.qtl_tstat, cohort.qtl_pvalue)
        return text, twin.n_pairs
    # -Q alone computes the table and the components and writes neither; ten components clipped to the six samples less three
    want, n = expected(3, 100000)
    r = run("-g", vcf, "-Q", out)
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert open(out, "rb").read() == want and not os.path.exists(q) and not os.path.exists(pcs)
    assert b"qtl: %d variants of 330 records (%d multi-allelic, %d without GT, %d on contigs the cohort does not know), 3 covariates, %d pairs written" % (
        len(pos), skipped[0], skipped[1], skipped[2], n) in r.stderr
    # beside -q and -P with -C and -w, from a gzip file
    with open(vcf, "rb") as f, gzip.open(vcf + ".gz", "wb") as z:
        z.write(f.read())
    want, n = expected(1, 500)
    r = run("-g", vcf + ".gz", "-Q", out, "-P", pcs, "-q", q, "-C", "1", "-w", "500")
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert open(out, "rb").read() == want and open(q, "rb").read() == ph.text(m, cl) and open(pcs, "rb").read() == cohort.pheno_pcs_host(ph, 1).text(m)
    # a table without rows: the file is its header line
    r = run("-g", vcf, "-Q", out, "-d", "9")
    assert r.returncode == 0 and open(out, "rb").read() == ref.text([], [], [], [], None, None, None)
    for f in (bed, q, pcs, out):
        os.remove(f)
    # a cohort sample the file does not have: status 1, nothing written
    qc.write_vcf(vcf, m, regions, 20, seed=6, samples=["g0", "g5", "other", "g3", "g1", "g4"])
    r = run("-g", vcf, "-Q", out, "-q", q)
    assert r.returncode == 1 and b"Sample g2 has no genotypes in " + vcf.encode() in r.stderr
    assert not os.path.exists(out) and not os.path.exists(q) and not os.path.exists(bed)
    # -Q without -g, and windows that do not parse
    r = run("-Q", out)
    assert r.returncode == 1 and b"Please supply the genotypes with '-g' option!" in r.stderr and not os.path.exists(out)
    for bad in ("-1", "1.5", "wide", "", "4294967296"):
        r = run("-g", vcf, "-Q", out, "-w", bad)
        assert r.returncode == 1 and b"Unrecognized window argument!" in r.stderr, bad
        assert not os.path.exists(out) and not os.path.exists(bed)
    c.close()
