"""The permutation pass of the cis-sQTL scan on the device (rgx_cohort_qtl_permute: k_qtl_perm of csrc/qtl_perm_kernels.hip without member
lists, csrc/cohort_qtl_perm.cpp): a workgroup per (row, 64 permutations) over all the row's tiles of 64 usable variants, the row's residual in LDS, the permuted panel gathered from it.
Expectations: the library's host twin in every array of the result as bit patterns, the nominal scan's best pair, and the restatement of
tests/qtl_perm_ref.py (exact fused multiply-adds) at sampled (row, permutation)."""
import os
import subprocess

import numpy as np
import pytest

import cluster_cases
import pheno_cases as pc
import qtl_cases as qc
import qtl_perm_cases as pcs
import qtl_perm_ref as pref
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


def _check(co, c, n_perm=5, seed=1, **kw):
    """Device == twin in every array.  Returns both (the arrays are views: the results must outlive what is read from them)."""
    from regtools_amd import cohort
    a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window, n_perm=n_perm, seed=seed)
    a.update(kw)
    ph = cohort.pheno_table_from_rank2(a.pop("rank2", c.rank2))
    dev, twin = co.qtl_permute(ph, **a), cohort.qtl_permute_host(ph, **a)
    assert (dev.n_rows, dev.n_samples, dev.n_variants, dev.n_cov) == (twin.n_rows, twin.n_samples, twin.n_variants, twin.n_cov)
    assert (dev.n_constant, dev.n_explained, dev.n_flat_rows) == (twin.n_constant, twin.n_explained, twin.n_flat_rows)
    pref.same_perm_result(dev, twin)
    tiles = (-(-(dev.n_perm + 1) // 64)) * int((-(-dev.n_cis.astype(np.int64) // 64)).sum())
    assert dev.n_tiles == tiles and twin.n_tiles == 0
    return dev, twin


def _nominal_best(co, c, dev, **kw):
    """best_variant, best_r and best_slope are the device's nominal scan's best pair, bit for bit."""
    from regtools_amd import cohort
    a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window)
    a.update(kw)
    nom = co.qtl_nominal(cohort.pheno_table_from_rank2(c.rank2), **a)
    has = nom.best != ref.NO_PAIR
    assert np.array_equal(dev.n_cis, np.diff(nom.pair_begin.astype(np.int64))) and (dev.best_variant[~has] == pref.NO_PAIR).all()
    assert np.array_equal(dev.best_variant[has], nom.pair_variant[nom.best[has]])
    ref.same_bits(dev.best_r[has], nom.r[nom.best[has]])
    ref.same_bits(dev.best_slope[has], nom.slope[nom.best[has]])
    ref.same_bits(dev.perm_r[:, 0][has], np.abs(nom.r[nom.best[has]]))
    return nom


S_SWEEP = [(S, n) for S in (4, 15, 16, 17, 63, 64, 65, 129) for n in (0, 1)]


@pytest.mark.parametrize("S, n_cov", S_SWEEP)
def test_sample_counts_around_the_slab(co, S, n_cov):
    """One slab short of a sample, full, one sample over, several slabs with a partial one."""
    dev, _ = _check(co, qc.planted(S, 20, 24, n_cov, seed=S * 100 + n_cov), n_perm=5, seed=S)
    assert dev.n_pairs > 0 and dev.dof == S - n_cov - 2 and (dev.perm_r[:, 1:] != dev.perm_r[:, :1]).any()


@pytest.mark.parametrize("B1", [2, 63, 64, 65, 130])
@pytest.mark.parametrize("n_cis", [1, 63, 64, 65, 200])
def test_permutation_tiles_and_variant_tiles(co, B1, n_cis):
    """One and several blocks of 64 permutations (the last one partial, full, one over) against rows whose cis variants fill one and several tiles
    of 64 (partial, full, one over)."""
    V = max(n_cis, 8) if n_cis < 200 else 200
    c = pcs.rows_with(9, n_cis, V, seed=B1 * 1000 + n_cis)
    dev, _ = _check(co, c, n_perm=B1 - 1, seed=B1)
    assert (dev.variant_verdict == 0).all() and dev.n_cis[0] == n_cis
    if n_cis == 200:
        assert dev.n_cis.max() > 64                                      # (a row's variants span tiles)
    _nominal_best(co, c, dev)


def test_the_most_samples(co):
    """S = 2048, the contract's limit: the row's 16 KiB in LDS and the largest uint16 index, 128 slabs."""
    c = qc.planted(2048, 6, 9, 2, seed=2048)
    dev, _ = _check(co, c, n_perm=3, seed=2)
    assert dev.n_pairs > 0 and dev.dof == 2044
    _nominal_best(co, c, dev)


def test_a_row_block_that_spans_a_contig_boundary(co):
    c = qc.simple(9, 64, 130, 0, seed=77, span=4 * qc.WINDOW, contigs=2)
    assert len(set(c.regions[:, 0])) == 2
    dev, _ = _check(co, c, n_perm=9)
    assert dev.n_pairs > 0 and (c.var_tid[dev.best_variant[dev.n_cis > 0]] == c.regions[dev.n_cis > 0, 0]).all()
    _nominal_best(co, c, dev)


@pytest.mark.parametrize("window", [0, 0xffffffff])
def test_the_narrowest_and_the_widest_window(co, window):
    c = qc.case(65, 40, 40, 3)
    dev, _ = _check(co, c, window=window)
    assert dev.n_pairs > 0
    if window:
        assert list(dev.n_cis) == [int(((c.var_tid == t) & (dev.variant_verdict == 0)).sum()) for t in c.regions[:, 0]]


def test_tables_without_pairs(co):
    c = qc.case(30, 20, 24, 2)
    dev, _ = _check(co, c, var_tid=np.zeros(0, np.uint32), var_pos=np.zeros(0, np.uint32), dosage=np.zeros((0, 30), np.int8))
    assert dev.n_pairs == 0 and dev.n_variants == 0 and (dev.best_variant == pref.NO_PAIR).all() and not dev.perm_r.any()
    assert (dev.n_ge == 5).all() and (dev.beta_status == 2).all()
    dev, _ = _check(co, c, dosage=np.where(np.arange(24)[:, None] % 2, -1, 2) * np.ones((24, 30), np.int8))
    assert dev.n_pairs == 0 and dev.n_constant == 24 and (dev.best_variant == pref.NO_PAIR).all() and not dev.perm_r.any()
    r2 = c.rank2.copy()
    r2[3] = 20                                                           # a flat row, and the planted row without pairs behind it
    dev, _ = _check(co, c, rank2=r2)
    assert dev.n_flat_rows == 1 and dev.best_variant[3] == pref.NO_PAIR and not dev.perm_r[3].any() and dev.n_cis[19] == 0 and dev.n_pairs > 0
    assert np.signbit(dev.perm_r).sum() == 0


def test_equal_dosages_tie_and_the_earliest_wins(co):
    from regtools_amd import cohort
    c = qc.case(64, 16, 20, 1)
    nom = cohort.qtl_nominal_host(cohort.pheno_table_from_rank2(c.rank2), *c.args())
    k = int(np.argmax(np.diff(nom.pair_begin.astype(np.int64))))
    cis = nom.pair_variant[nom.pair_begin[k]:nom.pair_begin[k + 1]]
    v = int(nom.pair_variant[nom.best[k]])
    assert len(cis) >= 3
    for other in (int(cis[0]) if cis[0] != v else int(cis[1]), int(cis[-1]) if cis[-1] != v else int(cis[-2])):
        d = c.dosage.copy()
        d[other] = d[v]                                                  # two variants of the row's window with equal dosages: equal |r|
        dev, _ = _check(co, c, dosage=d)
        assert dev.best_variant[k] == min(v, other)
        _nominal_best(co, c, dev, dosage=d)


@pytest.mark.parametrize("S, K, V, n_cov", qc.PLANTED + [pcs.STRONG])
def test_planted_cases(co, S, K, V, n_cov):
    c = qc.case(S, K, V, n_cov) if (S, K, V, n_cov) != pcs.STRONG else pcs.strong_case()
    dev, _ = _check(co, c, n_perm=7 if (S, K, V, n_cov) != pcs.STRONG else pcs.STRONG_B, seed=11)
    assert dev.n_pairs > 0
    _nominal_best(co, c, dev)


def test_larger_run_against_the_restatement(co):
    """2,000 rows x 3,000 variants x 64 samples, 99 permutations: two blocks of permutations per row, rows of one and of several variant tiles."""
    from regtools_amd import cohort
    c = qc.planted(64, 2000, 3000, 3, seed=2064, window=60000, span=3_000_000)
    B, seed = 99, 17
    dev, _ = _check(co, c, n_perm=B, seed=seed)
    assert dev.n_pairs > 100_000 and dev.n_cis.max() > 64
    print("2000 x 3000 x 64, B = 99: %d pairs, %d tiles, %.3f ms, residuals %.3f ms, products %.3f ms, beta %.3f ms" % (
        dev.n_pairs, dev.n_tiles, dev.ms_perm, dev.ms_residual, dev.ms_products, dev.ms_beta))
    # 24 (row, permutation): three permutations of eight rows, the row with the most variants among them (a variant is restated once per row)
    rng = np.random.default_rng(1)
    rows = [int(np.argmax(dev.n_cis))] + [int(k) for k in rng.choice(np.nonzero(dev.n_cis > 0)[0], 7, replace=False)]
    only = set((k, int(b)) for k in rows for b in rng.choice(B + 1, 3, replace=False))
    want = pref.restate(c, cohort.quantile, pref.permutations(64, B, seed), only=only, verdict=dev.variant_verdict)
    assert len(only) == 24
    for k, b in only:
        ref.same_bits([dev.perm_r[k, b], dev.yy[k]], [want.perm_r[k, b], want.yy[k]])
        assert dev.n_cis[k] == want.n_cis[k] > 0


def test_full_path_with_the_text(gpu_ctx):
    """finish -> refine -> phenotypes -> pheno_pcs -> qtl_permute with the matrix still in HBM."""
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
    comp = c.pheno_pcs(ph, 3)
    regions = cohort.pheno_regions(m, ph)
    tid, pos, dosage = qc.variants_near(regions, S, 400, seed=12)
    ids = ["v%d" % i for i in range(400)]
    a = c.qtl_permute(ph, regions, tid, pos, dosage, comp.component, qc.WINDOW, n_perm=70, seed=4)
    h = cohort.merge_host([cluster_cases.Sample(t) for t in tables], pc.names(S))
    clh = cohort.refine_host(h, **refine)
    pht = cohort.phenotypes_host(h, clh, **kw)
    comp_t = cohort.pheno_pcs_host(pht, 3)
    twin = cohort.qtl_permute_host(pht, cohort.pheno_regions(h, pht), tid, pos, dosage, comp_t.component, qc.WINDOW, n_perm=70, seed=4)
    assert twin.n_rows == ph.n_rows >= 250 and twin.n_pairs > 1000
    pref.same_perm_result(a, twin)
    pheno_ids = [line.split(b"\t")[3].decode() for line in pht.text(h, clh).split(b"\n")[1:-1]]
    want = pref.text(pheno_ids, ids, pos, regions[:, 1], twin, cohort.qtl_tstat, cohort.qtl_pvalue)
    assert a.text(m, cl, ph, pos, ids) == twin.text(h, clh, pht, pos, ids) == want and want.count(b"\n") == int((twin.n_cis > 0).sum()) + 1
    c.close()
    cluster_cases.free_tables(tables)


def test_errors(co):
    from regtools_amd import RegtoolsError, cohort
    c = qc.case(65, 40, 40, 3)

    def refused(**kw):
        a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window, rank2=c.rank2, n_perm=5)
        a.update(kw)
        rank2 = a.pop("rank2")
        with pytest.raises(RegtoolsError) as e:
            co.qtl_permute(cohort.pheno_table_from_rank2(rank2), **a)
        assert e.value.code == RGX_ERR_ARG, kw.keys()
        return str(e.value)
    # judged on the host, before any launch
    refused(var_pos=c.var_pos[::-1].copy())
    assert "1 to 65535" in refused(n_perm=0) and "1 to 65535" in refused(n_perm=65536)
    perms = pref.permutations(65, 3, 1)
    perms[2, 0] = perms[2, 1]
    assert "row 2" in refused(perms=perms)
    assert "identity" in refused(perms=pref.permutations(65, 3, 1)[1:])
    # noticed by the device and reported through its flag words
    for at, bad in (((0, 0), 3), ((39, 64), -2)):
        d = c.dosage.copy()
        d[at] = bad
        assert "dosage" in refused(dosage=d)
    for at, bad in (((0, 0), 1), ((39, 64), 81)):
        r2 = c.rank2.copy()
        r2[at] = bad
        assert "rank2" in refused(rank2=r2)
    # the cohort is none the worse for it
    _check(co, c)


# (seed, reads): the six files over ONE gene model of tests/test_gpu_cohort_pheno.py, whose clusters have several rows
GENE_FILES = [(5, 20000), (5, 30000), (5, 45000), (5, 60000), (5, 25000), (5, 52000)]


def test_the_tool_runs_the_permutation_pass(gpu_ctx, tmp_path):
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
    vcf, bed, nominal, out = (str(tmp_path / n) for n in ("v.vcf", "x.bed", "x.qtl", "x.perm"))
    tid, pos, dosage, ids, skipped = qc.write_vcf(vcf, m, regions, 330, seed=6, samples=["g0", "g5", "other", "g3", "g1", "g4", "g2"])

    def run(*args):
        return subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-o", bed] + list(args) + paths, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, env=dict(os.environ, REGTOOLS_AMD_STATS="1"))

    def expected(n_cov, window, n_perm, seed):
        comp = cohort.pheno_pcs_host(ph, n_cov) if n_cov else None     # (component is a view: the object must outlive the call)
        twin = cohort.qtl_permute_host(ph, regions, tid, pos, dosage, comp.component if n_cov else None, window, n_perm=n_perm, seed=seed)
        assert twin.n_pairs > 100
        text = twin.text(m, cl, ph, pos, ids)
        pheno_ids = [line.split(b"\t")[3].decode() for line in ph.text(m, cl).split(b"\n")[1:-1]]
        assert text == pref.text(pheno_ids, ids, pos, regions[:, 1], twin, cohort.qtl_tstat, cohort.qtl_pvalue)
        return text, twin
    # -R alone: the defaults, 1000 permutations from seed 0, three covariates (ten components clipped to the six samples less three)
    want, twin = expected(3, 100000, 1000, 0)
    r = run("-g", vcf, "-R", out)
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert open(out, "rb").read() == want and not os.path.exists(nominal)
    assert b"perm: 1000 permutations from seed 0, %d variants, 3 covariates, %d pairs, %d rows written" % (
        len(pos), twin.n_pairs, int((twin.n_cis > 0).sum())) in r.stderr
    # beside -Q, with -B, -e, -C and -w
    want, twin = expected(1, 500, 37, 12345678901234567890)
    r = run("-g", vcf, "-R", out, "-Q", nominal, "-B", "37", "-e", "12345678901234567890", "-C", "1", "-w", "500")
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    comp = cohort.pheno_pcs_host(ph, 1)
    assert open(out, "rb").read() == want
    assert open(nominal, "rb").read() == cohort.qtl_nominal_host(ph, regions, tid, pos, dosage, comp.component, 500).text(m, cl, ph, pos, ids)
    # a table without rows: the file is its header line
    r = run("-g", vcf, "-R", out, "-d", "9")
    assert r.returncode == 0 and open(out, "rb").read() == pref.text([], [], [], [], None, None, None)
    for f in (bed, nominal, out):
        os.remove(f)
    # -R without -g, and arguments that do not parse
    r = run("-R", out)
    assert r.returncode == 1 and b"Please supply the genotypes with '-g' option!" in r.stderr and not os.path.exists(out)
    for bad in ("0", "-1", "65536", "1.5", "many", ""):
        r = run("-g", vcf, "-R", out, "-B", bad)
        assert r.returncode == 1 and b"Unrecognized permutations argument!" in r.stderr, bad
        assert not os.path.exists(out) and not os.path.exists(bed)
    for bad in ("-1", "1.5", "seed", "", "18446744073709551616"):
        r = run("-g", vcf, "-R", out, "-e", bad)
        assert r.returncode == 1 and b"Unrecognized seed argument!" in r.stderr, bad
        assert not os.path.exists(out) and not os.path.exists(bed)
    c.close()
