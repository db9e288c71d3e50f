"""The trans-sQTL scan on the device (rgx_cohort_qtl_trans: csrc/qtl_trans_kernels.hip, csrc/cohort_qtl_trans.cpp): the nominal scan's residual
stages, then every tile of 64 rows x 64 usable variants counted, the tiles with hits computed again and ranked, the hits sorted by row.
Expectations: the library's host twin in every array of the result as bit patterns, and the restatement of tests/qtl_trans_ref.py (exact fused
multiply-adds) where that is affordable."""
import os
import subprocess

import numpy as np
import pytest

import cluster_cases
import pheno_cases as pc
import qtl_cases as qc
import qtl_trans_cases as tc
import qtl_trans_ref as tref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "regtools-amd")
RGX_ERR_ARG = 7
FULL = 0xffffffff


@pytest.fixture(scope="module")
def co(gpu_ctx):
    import regtools_amd
    c = regtools_amd.Cohort(ctx=gpu_ctx)
    yield c
    c.close()


def _args(c, **kw):
    a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, pval=tc.PVAL, exclude_window=qc.WINDOW)
    a.update(kw)
    return a


def _check(co, c, **kw):
    """Device == twin in every array.  Returns both (the arrays are views: the results must outlive what is read from them)."""
    from regtools_amd import cohort
    a = _args(c, **kw)
    ph = cohort.pheno_table_from_rank2(c.rank2)
    dev, twin = co.qtl_trans(ph, **a), cohort.qtl_trans_host(ph, **a)
    assert (dev.n_rows, dev.n_samples, dev.n_variants, dev.n_cov, dev.dof) == (twin.n_rows, twin.n_samples, twin.n_variants, twin.n_cov, twin.dof)
    assert (dev.n_constant, dev.n_explained, dev.n_flat_rows) == (twin.n_constant, twin.n_explained, twin.n_flat_rows)
    tref.same_result(dev, twin)
    assert dev.n_tiles == (dev.n_rows + 63) // 64 * ((dev.n_variants + 63) // 64) and dev.n_hit_tiles <= dev.n_tiles and (dev.n_hit_tiles > 0) == (dev.n_hits > 0)
    return dev, twin


S_SWEEP = [(S, n) for S in (4, 15, 16, 17, 63, 64, 65, 129) for n in sorted({0, 1, S - 3} if S <= 17 else {0, 1})]


@pytest.mark.parametrize("S, n_cov", S_SWEEP)
def test_sample_counts_around_the_slab_and_the_partials(co, S, n_cov):
    """One slab short of a sample, full, one sample over; the 64 partials likewise; every degree of freedom down to 1."""
    c = tc.planted(S, 9, 9, n_cov, seed=S * 100 + n_cov)
    dev, _ = _check(co, c, r_min=0.0)
    assert dev.n_hits == dev.n_tested > 0 and dev.dof == S - n_cov - 2
    _check(co, c, pval=0.3)


@pytest.mark.parametrize("K", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 200])
def test_row_blocks_and_variant_tiles(co, K, V):
    """One and several row blocks against one and several tiles of usable variants.  With r_min = 0 every pair is a hit and every tile full: the
    edge of the rank arithmetic.  (A table of ONE row has one rank, so one quantile in every sample: the row is flat and meets nothing.)"""
    c = qc.simple(9, K, V, 1, seed=K * 1000 + V, span=4 * qc.WINDOW, contigs=1)
    dev, _ = _check(co, c, r_min=0.0, exclude_window=None)
    assert (dev.variant_verdict == 0).all()
    assert dev.n_hits == dev.n_tested == (K * V if K > 1 else 0) and dev.n_hit_tiles == (dev.n_tiles if K > 1 else 0)
    if K > 1:
        assert np.array_equal(dev.hit_variant, np.tile(np.arange(V, dtype=np.uint32), K))
    sparse, _ = _check(co, c, pval=0.01, exclude_window=None)
    assert sparse.n_hits < sparse.n_tested // 4 + 1


def test_tiles_without_hits_between_tiles_with_hits(co):
    """Three row blocks x four variant tiles with six hits: the compaction of the tiles and the offsets of their hits."""
    c = qc.simple(30, 130, 200, 0, seed=31, contigs=1)
    every, _ = _check(co, c, r_min=0.0, exclude_window=None)
    r_min = float(np.sort(np.abs(every.r))[-6])
    dev, _ = _check(co, c, r_min=r_min, exclude_window=None)
    assert dev.n_hits == 6 and dev.n_tiles == 12 and 2 <= dev.n_hit_tiles <= 6
    tiles = sorted({k // 64 * 4 + v // 64 for k, v in tc.hit_pairs(dev)})
    assert len(tiles) == dev.n_hit_tiles and tiles[-1] - tiles[0] + 1 > len(tiles)          # (a tile without hits lies between two with hits)


def test_unusable_variants_between_usable_ones(co):
    """Every other variant is constant: 100 usable of 200, so the second tile of usable variants is partial and the last two return at once."""
    c = qc.simple(9, 70, 200, 0, seed=41, contigs=1)
    d = c.dosage.copy()
    d[1::2] = 1
    dev, _ = _check(co, c, dosage=d, r_min=0.0, exclude_window=None)
    assert dev.n_constant == 100 and dev.n_tiles == 8 and dev.n_hit_tiles == 4 and dev.n_hits == 70 * 100
    assert np.array_equal(dev.hit_variant, np.tile(np.arange(0, 200, 2, dtype=np.uint32), 70))
    _check(co, c, dosage=d, pval=0.05)


def test_a_row_block_that_spans_a_contig_boundary(co):
    c = qc.simple(9, 64, 130, 0, seed=77, span=4 * qc.WINDOW, contigs=2)
    assert len(set(c.regions[:, 0])) == 2                               # (the one block has rows of both contigs)
    dev, _ = _check(co, c, r_min=0.0)
    assert dev.n_hits == dev.n_tested and 64 * 130 // 2 < dev.n_tested < 64 * 130
    # what a row does not meet lies on its own contig, inside the window
    met = np.zeros((64, 130), bool)
    for k, v in tc.hit_pairs(dev):
        met[k, v] = True
    k, v = np.nonzero(~met)
    assert (c.var_tid[v] == c.regions[k, 0]).all()
    assert (c.var_pos[v].astype(np.int64) >= c.regions[k, 1].astype(np.int64) - qc.WINDOW).all()
    assert (c.var_pos[v].astype(np.int64) <= c.regions[k, 2].astype(np.int64) + qc.WINDOW).all()


@pytest.mark.parametrize("window", [0, FULL])
def test_the_narrowest_and_the_widest_exclusion(co, window):
    c = tc.case(65, 40, 40, 3)
    dev, _ = _check(co, c, r_min=0.0, exclude_window=window)
    usable = dev.variant_verdict == 0
    if window:
        other = [int((usable & (c.var_tid != t)).sum()) for t in c.regions[:, 0]]
        assert list(np.diff(dev.hit_begin.astype(np.int64))) == other and dev.n_hits > 0
    else:
        assert 40 * int(usable.sum()) - 40 <= dev.n_hits <= 40 * int(usable.sum())


@pytest.mark.parametrize("S, K, V, n_cov", tc.PLANTED)
def test_planted_cases(co, S, K, V, n_cov):
    from regtools_amd import cohort
    c = tc.case(S, K, V, n_cov)
    dev, _ = _check(co, c)
    tc.check_conditions(c, dev)
    tref.same_result(dev, tref.restate(c, cohort.quantile, cohort.qtl_r_threshold(tc.PVAL, c.dof), qc.WINDOW))


def test_refusals_and_tables_without_hits(co):
    from regtools_amd import RegtoolsError, cohort
    c = tc.case(65, 40, 40, 3)
    dev, _ = _check(co, c)
    H = dev.n_hits
    assert H > 1

    def refused(**kw):
        a = _args(c, rank2=c.rank2)
        a.update(kw)
        rank2 = a.pop("rank2")
        with pytest.raises(RegtoolsError) as e:
            co.qtl_trans(cohort.pheno_table_from_rank2(rank2), **a)
        assert e.value.code == RGX_ERR_ARG, kw.keys()
        return str(e.value)
    # known behind the counting pass
    assert "%d pairs" % H in refused(max_hits=H - 1) and "%d pairs" % H in refused(max_hits=1)
    assert _check(co, c, max_hits=H)[0].n_hits == H
    # judged on the host, before any launch
    assert "r_min" in refused(r_min=float("nan")) and "r_min" in refused(r_min=1.5)
    refused(var_pos=c.var_pos[::-1].copy())
    # noticed by the device and reported through its flag words: the first and the last entry
    for at, bad in (((0, 0), 3), ((39, 64), -2)):
        d = c.dosage.copy()
        d[at] = bad
        assert "dosage" in refused(dosage=d)
    for at, bad in (((0, 0), 1), ((39, 64), 81)):
        r2 = c.rank2.copy()
        r2[at] = bad
        assert "rank2" in refused(rank2=r2)
    # the cohort is none the worse for it; no hits, no variants, none usable, a flat row
    none, _ = _check(co, c, r_min=1.0)
    assert none.n_hits == 0 and none.n_tested == dev.n_tested and not none.hit_begin.any()
    none, _ = _check(co, c, var_tid=np.zeros(0, np.uint32), var_pos=np.zeros(0, np.uint32), dosage=np.zeros((0, 65), np.int8), r_min=0.0)
    assert (none.n_hits, none.n_tested, none.n_tiles) == (0, 0, 0)
    none, _ = _check(co, c, dosage=np.where(np.arange(40)[:, None] % 2, -1, 2) * np.ones((40, 65), np.int8), r_min=0.0)
    assert (none.n_hits, none.n_tested, none.n_constant) == (0, 0, 40)
    r2 = c.rank2.copy()
    r2[3] = 40
    flat, _ = _check(co, qc.Case(**dict(c.__dict__, rank2=r2)), r_min=0.0)
    assert flat.n_flat_rows == 1 and flat.hit_begin[4] == flat.hit_begin[3] and flat.n_hits > 0


def test_larger_run(co):
    """4,000 rows x 6,000 variants x 64 samples at p = 1e-5: 63 row blocks x 94 variant tiles, a few percent of them with hits."""
    from regtools_amd import cohort
    c = tc.planted(64, 4000, 6000, 3, seed=4064, window=20000, span=3_000_000)
    dev, _ = _check(co, c, pval=1e-5, exclude_window=20000)
    print("4000 x 6000 x 64: %d hits of %d pairs, %d of %d tiles, %.3f ms, residuals %.3f ms, count %.3f ms, emit %.3f ms" % (
        dev.n_hits, dev.n_tested, dev.n_hit_tiles, dev.n_tiles, dev.ms_trans, dev.ms_residual, dev.ms_count, dev.ms_emit))
    pairs = tc.hit_pairs(dev)
    assert dev.n_hits >= 500 and 2 * len(set(pairs) & set(c.trans)) >= len(c.trans) and dev.n_hit_tiles < dev.n_tiles
    Q = tref.ref.basis(c.S, c.cov)
    c._T = tref.ref.quantile_table(c.K, cohort.quantile)
    for p in np.random.default_rng(1).integers(0, dev.n_hits, 24):
        k, v = pairs[p]
        tref.ref.same_bits([dev.yy[k], dev.gg[v], dev.r[p], dev.slope[p]], list(tref.ref.restate_pair(c, cohort.quantile, k, v, Q)))


def test_full_path_with_the_text(gpu_ctx):
    """finish -> refine -> phenotypes -> pheno_pcs -> qtl_trans with the matrix still in HBM, against the twin on the twin's table."""
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
    a = c.qtl_trans(ph, regions, tid, pos, dosage, pcs.component, pval=0.01, exclude_window=qc.WINDOW)
    h = cohort.merge_host([cluster_cases.Sample(t) for t in tables], pc.names(S))
    clh = cohort.refine_host(h, **refine)
    pht = cohort.phenotypes_host(h, clh, **kw)
    pcs_t = cohort.pheno_pcs_host(pht, 3)                              # (component is a view: the object must outlive the call)
    twin = cohort.qtl_trans_host(pht, cohort.pheno_regions(h, pht), tid, pos, dosage, pcs_t.component, pval=0.01, exclude_window=qc.WINDOW)
    assert twin.n_rows == ph.n_rows >= 250 and 100 < twin.n_hits < twin.n_tested // 4
    tref.same_result(a, twin)
    pheno_ids = [line.split(b"\t")[3].decode() for line in pht.text(h, clh).split(b"\n")[1:-1]]
    want = tref.text(pheno_ids, ids, twin, cohort.qtl_tstat, cohort.qtl_pvalue)
    assert a.text(m, cl, ph, pos, ids) == twin.text(h, clh, pht, pos, ids) == want
    c.close()
    cluster_cases.free_tables(tables)


# (seed, reads): the six files over ONE gene model of tests/test_gpu_cohort_qtl.py
GENE_FILES = [(5, 20000), (5, 30000), (5, 45000), (5, 60000), (5, 25000), (5, 52000)]


def test_the_tool_scans_every_variant_of_a_vcf(gpu_ctx, tmp_path):
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
    vcf, bed, q, pcs, out = (str(tmp_path / n) for n in ("v.vcf", "x.bed", "x.pheno", "x.PCs", "x.trans"))
    tid, pos, dosage, ids, skipped = qc.write_vcf(vcf, m, regions, 330, seed=6, samples=["g0", "g5", "other", "g3", "g1", "g4", "g2"])

    def run(*args):
        return subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-o", bed] + list(args) + paths, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, env=dict(os.environ, REGTOOLS_AMD_STATS="1"))

    def expected(n_cov, pval, window):
        pcs_t = cohort.pheno_pcs_host(ph, n_cov) if n_cov else None    # (component is a view: the object must outlive the call)
        twin = cohort.qtl_trans_host(ph, regions, tid, pos, dosage, pcs_t.component if n_cov else None, pval=pval, exclude_window=window)
        assert twin.n_hits > 100
        text = twin.text(m, cl, ph, pos, ids)
        pheno_ids = [line.split(b"\t")[3].decode() for line in ph.text(m, cl).split(b"\n")[1:-1]]
        assert text == tref.text(pheno_ids, ids, twin, cohort.qtl_tstat, cohort.qtl_pvalue)
        return text, twin
    header = tref.text([], [], None, None, None)
    # -X alone computes the table and the components and writes neither; ten components clipped to the six samples less three
    want, twin = expected(3, 0.2, 100)
    r = run("-g", vcf, "-X", out, "-u", "0.2", "-W", "100")
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert open(out, "rb").read() == want and not os.path.exists(q) and not os.path.exists(pcs)
    assert b"trans: p <= 0.2, exclusion 100, %d variants, 3 covariates, %d pairs tested, %d hits written" % (
        len(pos), twin.n_tested, twin.n_hits) in r.stderr
    # the defaults: p <= 1e-5 with one degree of freedom, five million bases left out
    r = run("-g", vcf, "-X", out)
    twin = cohort.qtl_trans_host(ph, regions, tid, pos, dosage, cohort.pheno_pcs_host(ph, 3).component)
    assert r.returncode == 0 and open(out, "rb").read() == twin.text(m, cl, ph, pos, ids)
    assert b"trans: p <= 1e-05, exclusion 5000000, " in r.stderr
    # beside -q and -P with -C, the cis pairs kept
    want, twin = expected(1, 0.01, None)
    r = run("-g", vcf, "-X", out, "-P", pcs, "-q", q, "-C", "1", "-u", "1e-2", "-W", "off")
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert open(out, "rb").read() == want and open(q, "rb").read() == ph.text(m, cl) and open(pcs, "rb").read() == cohort.pheno_pcs_host(ph, 1).text(m)
    assert b"exclusion off" in r.stderr
    # a table without rows: the file is its header line
    r = run("-g", vcf, "-X", out, "-d", "9")
    assert r.returncode == 0 and open(out, "rb").read() == header
    for f in (bed, q, pcs, out):
        os.remove(f)
    # -X without -g, and values that do not parse
    r = run("-X", out)
    assert r.returncode == 1 and b"Please supply the genotypes with '-g' option!" in r.stderr and not os.path.exists(out)
    for bad in ("0", "-0.1", "1.5", "small", "", "nan", "1e-5x"):
        r = run("-g", vcf, "-X", out, "-u", bad)
        assert r.returncode == 1 and b"Unrecognized threshold argument!" in r.stderr, bad
        assert not os.path.exists(out) and not os.path.exists(bed)
    for bad in ("-1", "1.5", "wide", "", "4294967296", "OFF"):
        r = run("-g", vcf, "-X", out, "-W", bad)
        assert r.returncode == 1 and b"Unrecognized exclusion argument!" in r.stderr, bad
        assert not os.path.exists(out) and not os.path.exists(bed)
    c.close()
