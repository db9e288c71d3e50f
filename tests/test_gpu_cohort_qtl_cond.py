"""The conditional permutation pass on the device (rgx_cohort_qtl_permute_conditional: csrc/qtl_cond_kernels.hip behind csrc/cohort_qtl_cond.cpp): a
wave per series for the basis and the row, a wave per place for beta and gg', a workgroup per (series, 64 permutations) over all the row's tiles
with the rank-m correction in the epilogue.  Expectations: the library's host twin in every array of the result as bit patterns, the tile count's
formula, and the restatement of tests/qtl_cond_ref.py (exact fused multiply-adds) at sampled (series, permutation)."""
import os
import subprocess

import numpy as np
import pytest

import cluster_cases
import pheno_cases as pc
import qtl_cases as qc
import qtl_cond_cases as cc
import qtl_cond_ref as cref
import qtl_perm_cases as pcs
import qtl_perm_ref as pref

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


def _check(co, c, series, n_perm=5, seed=1, **kw):
    """Device == twin in every array, and the tile count.  Returns both (the arrays are views: the results must outlive what is read from them)."""
    from regtools_amd import cohort
    a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window, n_perm=n_perm, seed=seed)
    a.update(kw)
    ph = cohort.pheno_table_from_rank2(a.pop("rank2", c.rank2))
    rows, begin, var = cohort.qtl_series(series)
    a.update(series_row=rows, cond_begin=begin, cond_variant=var)
    dev, twin = co.qtl_permute_conditional(ph, **a), cohort.qtl_permute_conditional_host(ph, **a)
    cref.same_cond_result(dev, twin)
    assert np.array_equal(dev.series_row, rows) and np.array_equal(dev.cond_begin, begin) and np.array_equal(dev.cond_variant, var)
    assert np.array_equal(dev.dof, c.S - c.n_cov - 2 - np.diff(begin.astype(np.int64)))
    tiles = (-(-(dev.n_perm + 1) // 64)) * int((-(-dev.n_window.astype(np.int64) // 64))[dev.cond_status == 0].sum())
    assert dev.n_tiles == tiles and twin.n_tiles == 0
    assert (dev.n_cis <= dev.n_window).all() and dev.n_pairs == int(dev.n_cis.sum())
    return dev, twin


def _cis(c, **kw):
    from regtools_amd import cohort
    return cc.cis_lists(c, cohort, **kw)


@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("S", [15, 16, 17, 63, 64, 65, 129])
def test_sample_counts_around_the_slab(co, S, m):
    """One slab short of a sample, full, one sample over, several slabs with a partial one."""
    c = qc.planted(S, 20, 24, 1, seed=S * 100 + m)
    series = cc.draw(_cis(c), (m,), seed=S, per_size=8)
    dev, _ = _check(co, c, series, n_perm=5, seed=S)
    assert len(series) >= 4 and dev.n_pairs > 0 and (dev.perm_r[:, 1:] != dev.perm_r[:, :1]).any()
    # a conditioning variant leaves nothing of itself: it is cis to its row and takes no part
    assert (dev.n_cis[dev.cond_status == 0] <= dev.n_window[dev.cond_status == 0] - m).all()


def test_the_most_samples_and_the_most_variants(co):
    """S = 2048, the contract's limit, with m = 8: the row's 16 KiB and the 4 KB of alphas in LDS beside the panels, 128 slabs."""
    c = pcs.rows_with(2048, 12, 16, seed=2048)
    cis = _cis(c)
    assert len(cis[0]) == 12
    dev, _ = _check(co, c, [(0, cis[0][2:10])], n_perm=3, seed=2)
    assert dev.n_cis[0] == 4 and dev.dof[0] == 2048 - 2 - 8 and dev.cond_status[0] == 0


@pytest.mark.parametrize("B1", [2, 64, 65, 130])
@pytest.mark.parametrize("n_cis", [1, 63, 64, 65, 200])
def test_permutation_tiles_and_variant_tiles(co, B1, n_cis):
    """One and several blocks of 64 permutations against a series whose variants that take part fill one and several tiles of 64 (partial, full,
    one over) once its m = 2 conditioning variants, which lie among them, have dropped out.  24 samples: among 200 variants of 9 samples one or
    another is a combination of the intercept and the two, and the count would not be the planned one."""
    c = pcs.rows_with(24, n_cis + 2, max(n_cis + 2, 8), seed=B1 * 1000 + n_cis)
    cis = _cis(c)
    assert len(cis[0]) == n_cis + 2
    at = (0, len(cis[0]) // 2) if n_cis > 1 else (0, 2)
    dev, _ = _check(co, c, [(0, [cis[0][at[0]], cis[0][at[1]]])], n_perm=B1 - 1, seed=B1)
    assert dev.n_cis[0] == n_cis and dev.n_window[0] == n_cis + 2 and dev.best_variant[0] not in (cis[0][at[0]], cis[0][at[1]])


def test_a_mixed_list_of_series(co):
    """m = 1 .. 8 side by side, a row in several series, a collinear set, a series whose variants all drop out, a flat row."""
    c = qc.simple(40, 12, 60, 1, seed=4060, span=12000)
    cis = _cis(c)
    big = int(np.argmax([len(x) for x in cis]))
    assert len(cis[big]) >= 10
    series = [(big, cis[big][:m]) for m in range(1, 9)] + [(big, cis[big][3:5][::-1])]
    series += cc.draw(cis, (1, 2, 3), seed=3, per_size=4)
    # two variants of one row with equal dosages, both in a set: the second adds nothing to the first
    d = c.dosage.copy()
    d[cis[big][1]] = d[cis[big][0]]
    n_collinear = sum(1 for k, cv in series if cis[big][0] in cv and cis[big][1] in cv)
    # every cis variant of a row in its set
    small = [k for k in range(c.K) if 1 <= len(cis[k]) <= 8 and not set(cis[k]) & {cis[big][0], cis[big][1]}]
    assert small
    series.append((small[0], cis[small[0]]))
    # a flat row: its variants are cis to it all the same
    flat = [k for k in range(c.K) if k not in (big, small[0]) and cis[k]][0]
    r2 = c.rank2.copy()
    r2[flat] = c.K + 1
    series.append((flat, cis[flat][:1]))
    dev, _ = _check(co, c, series, n_perm=7, dosage=d, rank2=r2)
    assert dev.n_collinear == n_collinear >= 7 and dev.n_flat_series == sum(1 for k, _ in series if k == flat) >= 1
    assert dev.cond_status[-1] == 2 and dev.n_window[-1] == 0
    assert dev.cond_status[-2] == 0 and dev.n_cis[-2] == 0 and dev.n_window[-2] == len(cis[small[0]]) and dev.best_variant[-2] == pref.NO_PAIR
    assert not dev.perm_r[dev.n_cis == 0].any() and (dev.beta_status[dev.n_cis == 0] == 2).all() and dev.cond_status[0] == 0 and dev.n_cis[0] > 0
    # the duplicate of a conditioning variant takes no part either
    assert dev.n_cis[0] == dev.n_window[0] - 2


def test_a_table_that_spans_a_contig_boundary(co):
    c = qc.simple(9, 64, 130, 0, seed=77, span=4 * qc.WINDOW, contigs=2)
    assert len(set(c.regions[:, 0])) == 2
    series = cc.draw(_cis(c), (1, 2), seed=7, per_size=40)
    dev, _ = _check(co, c, series, n_perm=9)
    has = dev.n_cis > 0
    assert has.sum() > 20 and (c.var_tid[dev.best_variant[has]] == c.regions[dev.series_row[has], 0]).all()


@pytest.mark.parametrize("window", [0, 0xffffffff])
def test_the_narrowest_and_the_widest_window(co, window):
    c = qc.case(65, 40, 40, 3)
    series = cc.draw(_cis(c, window=window), (1,), seed=5, per_size=12, spare=0)
    dev, _ = _check(co, c, series, window=window)
    assert len(series) >= 3 and (dev.cond_status == 0).all()
    if window:
        assert dev.n_pairs > 0
        assert list(dev.n_window) == [int(((c.var_tid == c.regions[k, 0]) & (dev.variant_verdict == 0)).sum()) for k, _ in series]


def test_larger_run_against_the_restatement(co):
    """2,000 rows x 3,000 variants x 64 samples, 99 permutations, 600 series of m = 1 .. 3: two blocks of permutations per series, rows of one
    and of several variant tiles."""
    from regtools_amd import cohort
    c = qc.planted(64, 2000, 3000, 3, seed=2064, window=60000, span=3_000_000)
    B, seed = 99, 17
    series = cc.draw(_cis(c), (1, 2, 3), seed=9, per_size=200)
    dev, _ = _check(co, c, series, n_perm=B, seed=seed)
    assert len(series) == 600 and dev.n_pairs > 30_000 and dev.n_window.max() > 64
    print("600 series on 2000 x 3000 x 64, B = 99: %d pairs, %d tiles, %.3f ms, residuals %.3f ms, preparation %.3f ms, products %.3f ms, beta %.3f ms"
          % (dev.n_pairs, dev.n_tiles, dev.ms_cond, dev.ms_residual, dev.ms_prepare, dev.ms_products, dev.ms_beta))
    # 12 (series, permutation): the identity and two permutations of four series, the one with the most variants among them
    rng = np.random.default_rng(1)
    pick = [int(np.argmax(dev.n_cis))] + [int(n) for n in rng.choice(np.nonzero(dev.n_cis > 0)[0], 3, replace=False)]
    only = set((n, int(b)) for n in pick for b in [0] + list(1 + rng.choice(B, 2, replace=False)))
    want = cref.restate(c, cohort.quantile, pref.permutations(64, B, seed), series, only=only, verdict=dev.variant_verdict)
    assert len(only) == 12
    cref.same_as_restated(dev, want, only=only)


def test_full_path(gpu_ctx):
    """finish -> refine -> phenotypes -> pheno_pcs -> qtl_permute -> qtl_permute_conditional on every row's best variant, the matrix still in HBM."""
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
    first = c.qtl_permute(ph, regions, tid, pos, dosage, comp.component, qc.WINDOW, n_perm=70, seed=4)
    rows = np.nonzero(first.n_cis > 0)[0]
    lists = cohort.qtl_series([(int(k), [int(first.best_variant[k])]) for k in rows])
    a = c.qtl_permute_conditional(ph, regions, *lists, tid, pos, dosage, comp.component, qc.WINDOW, n_perm=70, seed=4)
    h = cohort.merge_host([cluster_cases.Sample(t) for t in tables], pc.names(S))
    clh = cohort.refine_host(h, **refine)
    pht = cohort.phenotypes_host(h, clh, **kw)
    comp_t = cohort.pheno_pcs_host(pht, 3)
    twin = cohort.qtl_permute_conditional_host(pht, cohort.pheno_regions(h, pht), *lists, tid, pos, dosage, comp_t.component, qc.WINDOW, n_perm=70,
                                               seed=4)
    assert len(rows) >= 200 and twin.n_pairs > 500 and (twin.dof == S - 3 - 2 - 1).all()
    cref.same_cond_result(a, twin)
    assert (a.best_variant != first.best_variant[rows]).all() and (a.n_cis < first.n_cis[rows]).all()
    c.close()
    cluster_cases.free_tables(tables)


def test_errors(co):
    from regtools_amd import RegtoolsError, cohort
    c = qc.case(65, 40, 40, 3)
    cis = _cis(c)
    good = cc.draw(cis, (1, 2), seed=2, per_size=5)
    k = good[-1][0]

    def refused(series, **kw):
        a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window, n_perm=5)
        a.update(kw)
        with pytest.raises(RegtoolsError) as e:
            co.qtl_permute_conditional(cohort.pheno_table_from_rank2(c.rank2), a.pop("regions"), *cohort.qtl_series(series), **a)
        assert e.value.code == RGX_ERR_ARG, series
        return str(e.value)
    # judged on the host, before any launch
    assert "at least one series" in refused([])
    assert "names row 40" in refused(good + [(40, [cis[k][0]])])
    assert "takes 1 to 8" in refused(good + [(k, [])]) and "takes 1 to 8" in refused([(k, list(range(9)))])
    assert "variant 40 of 40" in refused([(k, [40])])
    assert "twice" in refused([(k, [cis[k][0], cis[k][1], cis[k][0]])])
    far = [v for v in range(c.V) if c.var_tid[v] != c.regions[k, 0]]
    assert "not cis" in refused([(k, [far[0]])])
    assert "1 to 65535" in refused(good, n_perm=0)
    refused(good, var_pos=c.var_pos[::-1].copy())
    # noticed by the device and reported through its flag word
    usable = set(x for l in cis for x in l)
    near = [(kk, v) for v in range(c.V) if v not in usable for kk in range(c.K) if c.var_tid[v] == c.regions[kk, 0]
            and int(c.regions[kk, 1]) - c.window <= int(c.var_pos[v]) <= int(c.regions[kk, 2]) + c.window]
    assert near
    assert "constant or explained" in refused(good + [(near[0][0], [near[0][1]])])
    d = c.dosage.copy()
    d[0, 0] = 3
    assert "dosage" in refused(good, dosage=d)
    # the cohort is none the worse for it
    _check(co, c, good)


def test_too_few_samples_for_the_set(co):
    from regtools_amd import RegtoolsError, cohort
    c = pcs.rows_with(9, 12, 16, seed=99)                                # n_cov = 0: S = 9 carries m <= 6
    cis = _cis(c)
    _check(co, c, [(0, cis[0][:6])])
    with pytest.raises(RegtoolsError) as e:
        co.qtl_permute_conditional(cohort.pheno_table_from_rank2(c.rank2), c.regions, *cohort.qtl_series([(0, cis[0][:7])]), c.var_tid, c.var_pos,
                                   c.dosage, c.cov, c.window, n_perm=5)
    assert e.value.code == RGX_ERR_ARG and "no degree of freedom" in str(e.value)


# ---- the forward-backward pass -------------------------------------------------------------------------------------------------------------------
def _indep(co, c, **kw):
    """Device == twin, every array."""
    from regtools_amd import cohort
    P = cc.INDEP
    a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window, n_perm=P["B"],
             seed=P["perm_seed"], p_threshold=P["p_threshold"], max_signals=P["max_signals"])
    a.update(kw)
    ph = cohort.pheno_table_from_rank2(c.rank2)
    dev, twin = co.qtl_independent(ph, **a), cohort.qtl_independent_host(ph, **a)
    cref.same_indep_result(dev, twin)
    return dev, twin


def test_the_planted_signals_on_the_device(co):
    c = cc.indep_case()
    dev, _ = _indep(co, c)
    for k, planted in c.two:
        s = slice(int(dev.sig_begin[k]), int(dev.sig_begin[k + 1]))
        assert sorted(int(v) for v in dev.variant[s]) == planted and list(dev.rank[s]) == [1, 2]
    assert dev.n_entered == len(c.two) + len(c.one) + len(c.tag) and dev.n_forward_rounds == 3
    assert any(list(dev.rank[dev.sig_begin[k]:dev.sig_begin[k + 1]]) == [2, 3] for k, _ in c.tag)
    # the cap, and a threshold that lets every fit in
    dev, _ = _indep(co, c, max_signals=1)
    assert dev.n_forward_rounds == 0 and dev.n_capped == dev.n_entered == dev.n_signals
    dev, _ = _indep(co, cc.indep_case(n_two=3, n_one=3, n_null=3, n_tag=2, per_row=10), max_signals=8, p_threshold=1.0)
    assert dev.n_capped > 0 and dev.n_cond.max() == 7 and dev.n_forward_rounds == 7


def test_independent_signals_of_a_larger_run(co):
    """2,000 rows x 3,000 variants x 64 samples, 99 permutations; every third row carries a planted effect."""
    c = qc.planted(64, 2000, 3000, 3, seed=2064, window=60000, span=3_000_000)
    dev, twin = _indep(co, c, n_perm=99, seed=17, p_threshold=0.05, max_signals=8)
    assert dev.n_entered > 300 and dev.n_forward_rounds >= 1 and dev.n_signals >= dev.n_entered - 50
    print("independent signals on 2000 x 3000 x 64, B = 99: %d rows entered, %d forward rounds, %d series, %d signals; %.3f ms (round 0 %.3f ms, "
          "forward %.3f ms, backward %.3f ms); twin %.3f ms" % (dev.n_entered, dev.n_forward_rounds, dev.n_series_total, dev.n_signals,
                                                              dev.ms_indep, dev.ms_round0, dev.ms_forward, dev.ms_backward, twin.ms_indep))


def test_full_path_with_the_text_of_the_signals(gpu_ctx):
    """finish -> refine -> phenotypes -> pheno_pcs -> qtl_independent with the matrix still in HBM, and the text."""
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
    a = c.qtl_independent(ph, regions, tid, pos, dosage, comp.component, qc.WINDOW, n_perm=70, seed=4, p_threshold=0.3, max_signals=3)
    h = cohort.merge_host([cluster_cases.Sample(t) for t in tables], pc.names(S))
    clh = cohort.refine_host(h, **refine)
    pht = cohort.phenotypes_host(h, clh, **kw)
    comp_t = cohort.pheno_pcs_host(pht, 3)
    twin = cohort.qtl_independent_host(pht, cohort.pheno_regions(h, pht), tid, pos, dosage, comp_t.component, qc.WINDOW, n_perm=70, seed=4,
                                       p_threshold=0.3, max_signals=3)
    assert twin.n_entered > 20 and twin.n_forward_rounds >= 1
    cref.same_indep_result(a, twin)
    pheno_ids = [line.split(b"\t")[3].decode() for line in pht.text(h, clh).split(b"\n")[1:-1]]
    want = cref.indep_text(pheno_ids, ids, pos, regions[:, 1], twin, cohort.qtl_tstat, cohort.qtl_pvalue)
    assert a.text(m, cl, ph, pos, ids) == twin.text(h, clh, pht, pos, ids) == want and want.count(b"\n") == twin.n_signals + 1
    c.close()
    cluster_cases.free_tables(tables)


def test_errors_of_the_forward_backward_pass(co):
    from regtools_amd import RegtoolsError, cohort
    c = cc.indep_case(n_two=2, n_one=2, n_null=2, n_tag=1)
    ph = cohort.pheno_table_from_rank2(c.rank2)
    d = c.dosage.copy()
    d[3, 3] = 7
    for kw, word in ((dict(p_threshold=0.0), "(0, 1]"), (dict(max_signals=9), "1 to 8"), (dict(n_perm=0), "1 to 65535"), (dict(dosage=d), "dosage")):
        a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window, n_perm=20)
        a.update(kw)
        with pytest.raises(RegtoolsError) as e:
            co.qtl_independent(ph, **a)
        assert e.value.code == RGX_ERR_ARG and word in str(e.value), kw
    _indep(co, c, n_perm=50)                                             # the cohort is none the worse for it


# (seed, reads): the six files over ONE gene model of tests/test_gpu_cohort_pheno.py, whose clusters have several rows
GENE_FILES = [(5, 20000), (5, 30000), (5, 45000), (5, 60000), (5, 25000), (5, 52000)]


def test_the_tool_writes_the_signals(gpu_ctx, tmp_path):
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
    regions = cohort.pheno_regions(m, ph)
    vcf, bed, perm, out = (str(tmp_path / n) for n in ("v.vcf", "x.bed", "x.perm", "x.indep"))
    tid, pos, dosage, ids, _ = qc.write_vcf(vcf, m, regions, 330, seed=6, samples=["g0", "g5", "other", "g3", "g1", "g4", "g2"])

    def run(*args):
        return subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-o", bed] + list(args) + paths, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, env=dict(os.environ, REGTOOLS_AMD_STATS="1"))
    # -I beside -R with -F, -B, -e, -C and -w: one covariate, so that the six samples leave room for a second signal
    comp = cohort.pheno_pcs_host(ph, 1)
    twin = cohort.qtl_independent_host(ph, regions, tid, pos, dosage, comp.component, 500, n_perm=99, seed=7, p_threshold=0.5, max_signals=8)
    r = run("-g", vcf, "-I", out, "-R", perm, "-F", "0.5", "-B", "99", "-e", "7", "-C", "1", "-w", "500")
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    text = open(out, "rb").read()
    assert text == twin.text(m, cl, ph, pos, ids) and twin.n_signals > 10 and twin.n_forward_rounds >= 1
    assert b"indep: %d rows entered, %d forward rounds, %d conditional series, %d signals written" % (
        twin.n_entered, twin.n_forward_rounds, twin.n_series_total, twin.n_signals) in r.stderr
    # every rank-1 line of a row with one signal is that row's -R line and "\t1\t0"
    perm_lines = dict((l.split(b"\t")[0], l) for l in open(perm, "rb").read().split(b"\n")[1:-1])
    lines = text.split(b"\n")[1:-1]
    per_row = {}
    for l in lines:
        per_row.setdefault(l.split(b"\t")[0], []).append(l)
    singles = [ls[0] for ls in per_row.values() if len(ls) == 1 and ls[0].endswith(b"\t1\t0")]
    assert len(singles) > 5 and all(l == perm_lines[l.split(b"\t")[0]] + b"\t1\t0" for l in singles)
    # -I alone: the defaults (1000 permutations from seed 0, three covariates, p <= 0.05)
    comp3 = cohort.pheno_pcs_host(ph, 3)
    twin = cohort.qtl_independent_host(ph, regions, tid, pos, dosage, comp3.component, 100000, n_perm=1000, seed=0, p_threshold=0.05, max_signals=8)
    os.remove(perm)
    r = run("-g", vcf, "-I", out)
    assert r.returncode == 0 and open(out, "rb").read() == twin.text(m, cl, ph, pos, ids) and not os.path.exists(perm), r.stderr[-2000:]
    # a table without rows: the file is its header line
    r = run("-g", vcf, "-I", out, "-d", "9")
    assert r.returncode == 0 and open(out, "rb").read() == cref.indep_text([], [], [], [], None, None, None)
    for f in (bed, out):
        os.remove(f)
    c.close()
