"""The grouped permutation pass of the cis-sQTL scan on the device (rgx_cohort_qtl_permute_grouped: k_qtl_perm of csrc/qtl_perm_kernels.hip with
member lists, csrc/cohort_qtl_group.cpp): a workgroup per (group, 64 permutations) that walks the group's members, each member's residual in LDS in turn, the
running maximum per permutation in registers across members.  Expectations: the library's host twin in every array of the result as bit patterns;
the device's own ungrouped pass (singleton groups reproduce it, every group is the maximum of its members) -- the same kernel without its lists, so
that comparison checks the two ways into it against each other and is no independent evidence; the device's nominal scan at the best pair; and the
restatement of tests/qtl_group_ref.py (exact fused multiply-adds) at sampled (group, permutation)."""
import os
import subprocess

import numpy as np
import pytest

import cluster_cases
import pheno_cases as pc
import qtl_cases as qc
import qtl_group_cases as gc
import qtl_group_ref as gref
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


def _args(c, n_perm=5, seed=1, **kw):
    a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window, n_perm=n_perm, seed=seed)
    a.update(kw)
    return a


def _check(co, c, groups, G, **kw):
    """Device == twin in every array.  Returns both (the arrays are views: the results must outlive what is read from them)."""
    from regtools_amd import cohort
    a = _args(c, **kw)
    ph = cohort.pheno_table_from_rank2(a.pop("rank2", c.rank2))
    dev = co.qtl_permute_grouped(ph, groups=groups, n_groups=G, **a)
    twin = cohort.qtl_permute_grouped_host(ph, groups=groups, n_groups=G, **a)
    assert (dev.n_rows, dev.n_samples, dev.n_variants, dev.n_cov) == (twin.n_rows, twin.n_samples, twin.n_variants, twin.n_cov)
    assert (dev.n_constant, dev.n_explained, dev.n_flat_rows) == (twin.n_constant, twin.n_explained, twin.n_flat_rows)
    gref.same_group_result(dev, twin)
    tiles = (-(-(dev.n_perm + 1) // 64)) * int((-(-dev.n_cis[dev.grp_row].astype(np.int64) // 64)).sum())
    assert dev.n_tiles == tiles and twin.n_tiles == 0
    return dev, twin


def _ungrouped(co, c, **kw):
    from regtools_amd import cohort
    a = _args(c, **kw)
    return co.qtl_permute(cohort.pheno_table_from_rank2(a.pop("rank2", c.rank2)), **a)


def _nominal_best(co, c, dev, **kw):
    """best_r and best_slope are the device's nominal scan's r and slope at (best_row, best_variant), bit for bit, and no pair of the group's
    members has larger bits."""
    from regtools_amd import cohort
    a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window)
    a.update(kw)
    nom = co.qtl_nominal(cohort.pheno_table_from_rank2(a.pop("rank2", c.rank2)), **a)
    bits = np.abs(nom.r).view(np.uint64)
    n = 0
    for g in range(dev.n_groups):
        if not dev.group_n_cis[g]:
            continue
        k, v = int(dev.best_row[g]), int(dev.best_variant[g])
        lo, hi = int(nom.pair_begin[k]), int(nom.pair_begin[k + 1])
        at = lo + int(np.nonzero(nom.pair_variant[lo:hi] == v)[0][0])
        ref.same_bits([dev.best_r[g], dev.best_slope[g], dev.perm_r[g, 0]], [nom.r[at], nom.slope[at], abs(nom.r[at])])
        for m in dev.grp_row[dev.grp_begin[g]:dev.grp_begin[g + 1]]:
            assert not (bits[nom.pair_begin[m]:nom.pair_begin[m + 1]] > bits[at]).any()
        n += 1
    assert n
    return nom


S_SWEEP = [(S, n) for S in (4, 15, 16, 17, 63, 64, 65, 129) for n in (0, 1)]


@pytest.mark.parametrize("S, n_cov", S_SWEEP)
def test_sample_counts_around_the_slab(co, S, n_cov):
    """One slab short of a sample, full, one sample over, several slabs with a partial one; two groups of 7 and 13 rows."""
    groups = np.where(np.arange(20) < 7, 0, 1).astype(np.uint32)
    dev, _ = _check(co, qc.planted(S, 20, 24, n_cov, seed=S * 100 + n_cov), groups, 2, n_perm=5, seed=S)
    assert (dev.group_n_cis > 0).all() and dev.dof == S - n_cov - 2 and (dev.perm_r[:, 1:] != dev.perm_r[:, :1]).any()


@pytest.mark.parametrize("B1", [2, 63, 64, 65, 130])
@pytest.mark.parametrize("n_cis", [(1, 65), (63, 64), (64, 1), (200, 0)])
def test_permutation_tiles_and_members_variant_tiles(co, B1, n_cis):
    """One and several blocks of 64 permutations against a group of two members whose cis variants fill a part of a tile, a whole tile, a tile and
    one variant, several tiles, or nothing; the other three rows are a second group."""
    c = gc.two_rows_with(9, n_cis[0], n_cis[1], seed=B1 * 1000 + n_cis[0])
    groups = np.array([0, 0, 1, 1, 1], np.uint32)
    dev, _ = _check(co, c, groups, 2, n_perm=B1 - 1, seed=B1)
    assert (dev.variant_verdict == 0).all() and (dev.n_cis[0], dev.n_cis[1]) == n_cis and dev.group_n_cis[0] == sum(n_cis)
    gref.max_identity(dev, _ungrouped(co, c, n_perm=B1 - 1, seed=B1), groups, 2)
    _nominal_best(co, c, dev)


def test_groups_of_one_two_and_seventeen_members(co):
    c = qc.planted(30, 20, 24, 1, seed=117)
    groups = np.array([0, 1, 1] + [2] * 17, np.uint32)
    dev, _ = _check(co, c, groups, 3, n_perm=70)
    assert np.diff(dev.grp_begin).tolist() == [1, 2, 17] and (dev.group_n_cis > 0).all()
    gref.max_identity(dev, _ungrouped(co, c, n_perm=70), groups, 3)
    _nominal_best(co, c, dev)


def test_groups_whose_members_interleave(co):
    c = qc.case(65, 40, 40, 3)
    groups = (np.arange(40) % 2).astype(np.uint32)
    dev, _ = _check(co, c, groups, 2, n_perm=9)
    assert dev.grp_row[:20].tolist() == list(range(0, 40, 2)) and dev.grp_row[20:].tolist() == list(range(1, 40, 2))
    gref.max_identity(dev, _ungrouped(co, c, n_perm=9), groups, 2)
    _nominal_best(co, c, dev)


def test_the_most_samples(co):
    """S = 2048, the contract's limit: the 16 KiB LDS row loaded for the first member and reloaded for the second."""
    c = qc.planted(2048, 6, 9, 2, seed=2048)
    groups = np.array([0, 0] + [gc.NO_GROUP] * 4, np.uint32)
    dev, _ = _check(co, c, groups, 1, n_perm=3, seed=2)
    assert dev.n_cis[0] > 0 and dev.n_cis[1] > 0 and dev.dof == 2044 and dev.grp_row.tolist() == [0, 1]
    gref.max_identity(dev, _ungrouped(co, c, n_perm=3, seed=2), groups, 1)
    _nominal_best(co, c, dev)


def test_groups_without_pairs_and_members_without_cis_variants(co):
    c, groups, G, empty = gc.degenerate()
    dev, _ = _check(co, c, groups, G)
    for g in empty:
        gref.no_pairs(dev, g)
    assert (dev.group_n_cis[:3] > 0).all() and np.signbit(dev.perm_r).sum() == 0 and dev.n_flat_rows == 2
    gref.max_identity(dev, _ungrouped(co, c), groups, G)
    dev, _ = _check(co, c, np.full(20, gc.NO_GROUP, np.uint32), 2)
    assert dev.n_pairs == 0 and dev.n_tiles == 0
    # no variants at all
    dev, _ = _check(co, c, groups, G, var_tid=np.zeros(0, np.uint32), var_pos=np.zeros(0, np.uint32), dosage=np.zeros((0, 30), np.int8))
    assert dev.n_pairs == 0 and not dev.perm_r.any() and (dev.best_row == gc.NO_PAIR).all()


def test_ties_go_to_the_lowest_row_and_then_to_the_earliest_variant(co):
    groups, G = gc.one_group(8)
    for c, want in ((gc.tie_rows(), (1, 3)), (gc.tie_variants(5), (1, 3)), (gc.tie_variants(0), (1, 0)), (gc.tie_across(), (1, 5))):
        dev, _ = _check(co, c, groups, G, n_perm=7, seed=11)
        assert (dev.best_row[0], dev.best_variant[0]) == want
        _nominal_best(co, c, dev)
    # the equal rows far apart inside a group of 17 members, the equal variants in different tiles of the members' 150
    c, groups = gc.tie_wide()
    dev, _ = _check(co, c, groups, 2, n_perm=7)
    assert (dev.best_row[0], dev.best_variant[0]) == (2, 7) and dev.n_cis[2] == 150 and np.diff(dev.grp_begin).tolist() == [17, 3]
    ung = _ungrouped(co, c, n_perm=7)
    gref.max_identity(dev, ung, groups, 2)
    ref.same_bits(ung.perm_r[2], ung.perm_r[18])
    _nominal_best(co, c, dev)


def test_a_contig_boundary_inside_a_group(co):
    c = qc.simple(9, 64, 130, 0, seed=77, span=4 * qc.WINDOW, contigs=2)
    groups = (np.arange(64) // 8).astype(np.uint32)
    assert any(len(set(c.regions[8 * g:8 * g + 8, 0])) == 2 for g in range(8))
    dev, _ = _check(co, c, groups, 8, n_perm=9)
    assert (dev.group_n_cis > 0).all() and (c.var_tid[dev.best_variant] == c.regions[dev.best_row, 0]).all()
    gref.max_identity(dev, _ungrouped(co, c, n_perm=9), groups, 8)
    _nominal_best(co, c, dev)


@pytest.mark.parametrize("window", [0, 0xffffffff])
def test_the_narrowest_and_the_widest_window(co, window):
    c = qc.case(65, 40, 40, 3)
    groups, G = gc.round_robin(40)
    dev, _ = _check(co, c, groups, G, window=window)
    assert dev.n_pairs > 0 and 1 not in dev.grp_row
    gref.max_identity(dev, _ungrouped(co, c, window=window), groups, G)
    if window:
        assert list(dev.n_cis) == [int(((c.var_tid == t) & (dev.variant_verdict == 0)).sum()) for t in c.regions[:, 0]]


@pytest.mark.parametrize("S, K, V, n_cov", qc.PLANTED)
def test_device_against_device(co, S, K, V, n_cov):
    """Singleton groups are Cohort.qtl_permute in every array; round-robin groups (one row in none) are the maxima of its rows; the best pair is
    the device's nominal scan's."""
    c = qc.case(S, K, V, n_cov)
    ung = _ungrouped(co, c, n_perm=7, seed=11)
    groups, G = gc.singletons(K)
    dev, _ = _check(co, c, groups, G, n_perm=7, seed=11)
    gref.same_as_ungrouped(dev, ung)
    assert dev.n_tiles == ung.n_tiles
    groups, G = gc.round_robin(K)
    dev, _ = _check(co, c, groups, G, n_perm=7, seed=11)
    gref.max_identity(dev, ung, groups, G)
    _nominal_best(co, c, dev)


def test_the_kernel_without_lists_and_with_singleton_lists(co):
    """One kernel behind both passes: S = 17 (the slab's tail), five rows of 0, 1, 65, 0 and 64 cis variants (a variant-tile edge; members
    without pairs between members with pairs), B + 1 = 65 (a second tile of permutations), through Cohort.qtl_permute -- no lists on the device
    -- and through singleton groups -- the lists -- and both against the host twins."""
    from regtools_amd import cohort
    c = gc.merged_case()
    groups, G = gc.singletons(5)
    dev, twin = _check(co, c, groups, G, n_perm=64, seed=3)
    ung = _ungrouped(co, c, n_perm=64, seed=3)
    assert tuple(ung.n_cis) == gc.MERGED_COUNTS and (ung.variant_verdict == 0).all() and ung.perm_r.shape == (5, 65)
    gref.same_as_ungrouped(dev, ung)
    assert dev.best_row.tolist() == [gc.NO_PAIR, 1, 2, gc.NO_PAIR, 4] and dev.n_tiles == ung.n_tiles == 2 * (1 + 2 + 1)
    ung_twin = cohort.qtl_permute_host(cohort.pheno_table_from_rank2(c.rank2), **_args(c, n_perm=64, seed=3))
    gref.same_as_ungrouped(twin, ung_twin)
    gref.same_as_ungrouped(dev, ung_twin)
    assert ung.n_pairs == ung_twin.n_pairs == 130 and ung_twin.n_tiles == 0
    assert (ung.n_constant, ung.n_explained, ung.n_flat_rows) == (ung_twin.n_constant, ung_twin.n_explained, ung_twin.n_flat_rows)
    for g in (0, 3):
        gref.no_pairs(dev, g)
    assert (dev.perm_r[[1, 2, 4], 1:] != dev.perm_r[[1, 2, 4], :1]).any()


def test_larger_run_against_the_ungrouped_pass_and_the_restatement(co):
    """2,000 rows x 3,000 variants x 64 samples, 99 permutations, the rows grouped in runs of 1 .. 8: two blocks of permutations per group, members
    of one and of several variant tiles."""
    from regtools_amd import cohort
    c = qc.planted(64, 2000, 3000, 3, seed=2064, window=60000, span=3_000_000)
    B, seed = 99, 17
    groups, G = gc.runs(2000, seed=3)
    dev, _ = _check(co, c, groups, G, n_perm=B, seed=seed)
    assert dev.n_pairs > 100_000 and dev.n_cis.max() > 64 and sorted(set(np.diff(dev.grp_begin))) == list(range(1, 9))
    print("2000 x 3000 x 64 in %d groups, B = 99: %d pairs, %d tiles, %.3f ms, residuals %.3f ms, products %.3f ms, beta %.3f ms" % (
        G, dev.n_pairs, dev.n_tiles, dev.ms_perm, dev.ms_residual, dev.ms_products, dev.ms_beta))
    ung = _ungrouped(co, c, n_perm=B, seed=seed)
    gref.max_identity(dev, ung, groups, G)
    print("ungrouped: products %.3f ms, beta %.3f ms" % (ung.ms_products, ung.ms_beta))
    # 24 (group, permutation): four permutations of six groups of at most three members with pairs, one of three members among them
    rng = np.random.default_rng(1)
    size = np.diff(dev.grp_begin)
    some = [int(np.nonzero((size == 3) & (dev.group_n_cis > 0))[0][0])] + [int(g) for g in rng.choice(np.nonzero((size <= 2) & (dev.group_n_cis > 0))[0],
                                                                                                 5, replace=False)]
    only = set((g, int(b)) for g in some for b in rng.choice(B + 1, 4, replace=False))
    assert len(only) == 24
    want, rows = gref.restate_sampled(c, cohort.quantile, pref.permutations(64, B, seed), groups, G, only, dev.variant_verdict)
    for g, b in only:
        ref.same_bits([dev.perm_r[g, b]], [want[(g, b)]])
        for k in gc.members(groups, g):
            assert dev.n_cis[k] == rows.n_cis[k]
            ref.same_bits([dev.yy[k]], [rows.yy[k]])


def test_full_path_with_the_text(gpu_ctx):
    """finish -> refine -> phenotypes -> pheno_pcs -> pheno_groups -> qtl_permute_grouped with the matrix still in HBM."""
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
    groups, G = cohort.pheno_groups(cl, ph)
    tid, pos, dosage = qc.variants_near(regions, S, 400, seed=12)
    ids = ["v%d" % i for i in range(400)]
    a = c.qtl_permute_grouped(ph, regions, groups, G, tid, pos, dosage, comp.component, qc.WINDOW, n_perm=70, seed=4)
    h = cohort.merge_host([cluster_cases.Sample(t) for t in tables], pc.names(S))
    clh = cohort.refine_host(h, **refine)
    pht = cohort.phenotypes_host(h, clh, **kw)
    comp_t = cohort.pheno_pcs_host(pht, 3)
    groups_t, G_t = cohort.pheno_groups(clh, pht)
    assert G_t == G and np.array_equal(groups, groups_t) and 1 < G < ph.n_rows and np.diff(np.bincount(groups)).any()
    twin = cohort.qtl_permute_grouped_host(pht, cohort.pheno_regions(h, pht), groups_t, G_t, tid, pos, dosage, comp_t.component, qc.WINDOW, n_perm=70,
                                           seed=4)
    assert twin.n_rows == ph.n_rows >= 250 and twin.n_pairs > 1000
    gref.same_group_result(a, twin)
    pheno_ids = [line.split(b"\t")[3].decode() for line in pht.text(h, clh).split(b"\n")[1:-1]]
    want = gref.text(pheno_ids, ids, pos, regions[:, 1], twin, cohort.qtl_tstat, cohort.qtl_pvalue)
    assert a.text(m, cl, ph, pos, ids) == twin.text(h, clh, pht, pos, ids) == want and want.count(b"\n") == int((twin.group_n_cis > 0).sum()) + 1
    gref.max_identity(a, c.qtl_permute(ph, regions, tid, pos, dosage, comp.component, qc.WINDOW, n_perm=70, seed=4), groups, G)
    c.close()
    cluster_cases.free_tables(tables)


def test_errors(co):
    from regtools_amd import RegtoolsError, cohort
    c = qc.case(65, 40, 40, 3)
    groups, G = gc.round_robin(40)

    def refused(**kw):
        a = _args(c, rank2=c.rank2, groups=groups, n_groups=G)
        a.update(kw)
        rank2 = a.pop("rank2")
        with pytest.raises(RegtoolsError) as e:
            co.qtl_permute_grouped(cohort.pheno_table_from_rank2(rank2), **a)
        assert e.value.code == RGX_ERR_ARG, kw.keys()
        return str(e.value)
    # judged on the host, before any launch
    refused(var_pos=c.var_pos[::-1].copy())
    assert "1 to 65535" in refused(n_perm=0)
    bad = groups.copy()
    bad[39] = 3
    assert "row 39 is of group 3" in refused(groups=bad)
    assert "1 to 2^31 - 1 groups" in refused(n_groups=0)
    assert "65537 groups" in refused(n_groups=65537, n_perm=65535)
    perms = pref.permutations(65, 3, 1)
    perms[2, 0] = perms[2, 1]
    assert "row 2" in refused(perms=perms)
    # noticed by the device and reported through its flag words
    for at, val in (((0, 0), 3), ((39, 64), -2)):
        d = c.dosage.copy()
        d[at] = val
        assert "dosage" in refused(dosage=d)
    for at, val in (((0, 0), 1), ((39, 64), 81)):
        r2 = c.rank2.copy()
        r2[at] = val
        assert "rank2" in refused(rank2=r2)
    # the cohort is none the worse for it
    _check(co, c, groups, G)


# (seed, reads): the six files over ONE gene model of tests/test_gpu_cohort_pheno.py, whose clusters have several rows
GENE_FILES = [(5, 20000), (5, 30000), (5, 45000), (5, 60000), (5, 25000), (5, 52000)]


def test_the_tool_runs_the_grouped_pass(gpu_ctx, tmp_path):
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
    groups, G = cohort.pheno_groups(cl, ph)
    assert 1 < G < ph.n_rows
    vcf, bed, nominal, perm, out = (str(tmp_path / n) for n in ("v.vcf", "x.bed", "x.qtl", "x.perm", "x.group"))
    tid, pos, dosage, ids, skipped = qc.write_vcf(vcf, m, regions, 330, seed=6, samples=["g0", "g5", "other", "g3", "g1", "g4", "g2"])

    def run(*args):
        return subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-o", bed] + list(args) + paths, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, env=dict(os.environ, REGTOOLS_AMD_STATS="1"))

    def expected(n_cov, window, n_perm, seed):
        comp = cohort.pheno_pcs_host(ph, n_cov) if n_cov else None     # (component is a view: the object must outlive the call)
        twin = cohort.qtl_permute_grouped_host(ph, regions, groups, G, tid, pos, dosage, comp.component if n_cov else None, window, n_perm=n_perm,
                                               seed=seed)
        assert twin.n_pairs > 100
        text = twin.text(m, cl, ph, pos, ids)
        pheno_ids = [line.split(b"\t")[3].decode() for line in ph.text(m, cl).split(b"\n")[1:-1]]
        assert text == gref.text(pheno_ids, ids, pos, regions[:, 1], twin, cohort.qtl_tstat, cohort.qtl_pvalue)
        return text, twin
    # -G alone: the defaults of -R
    want, twin = expected(3, 100000, 1000, 0)
    r = run("-g", vcf, "-G", out)
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert open(out, "rb").read() == want and not os.path.exists(nominal) and not os.path.exists(perm)
    assert b"group: 1000 permutations from seed 0, %d variants, 3 covariates, %d groups, %d pairs, %d groups written" % (
        len(pos), G, twin.n_pairs, int((twin.group_n_cis > 0).sum())) in r.stderr
    # beside -R and -Q, with -B, -e, -C and -w
    want, twin = expected(1, 500, 37, 12345678901234567890)
    r = run("-g", vcf, "-G", out, "-R", perm, "-Q", nominal, "-B", "37", "-e", "12345678901234567890", "-C", "1", "-w", "500")
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    comp = cohort.pheno_pcs_host(ph, 1)
    assert open(out, "rb").read() == want
    assert open(perm, "rb").read() == cohort.qtl_permute_host(ph, regions, tid, pos, dosage, comp.component, 500, n_perm=37,
                                                              seed=12345678901234567890).text(m, cl, ph, pos, ids)
    assert open(nominal, "rb").read() == cohort.qtl_nominal_host(ph, regions, tid, pos, dosage, comp.component, 500).text(m, cl, ph, pos, ids)
    # a table without rows: the file is its header line
    r = run("-g", vcf, "-G", out, "-d", "9")
    assert r.returncode == 0 and open(out, "rb").read() == gref.HEAD.encode()
    for f in (bed, nominal, perm, out):
        os.remove(f)
    # -G without -g
    r = run("-G", out)
    assert r.returncode == 1 and b"Please supply the genotypes with '-g' option!" in r.stderr and not os.path.exists(out)
    r = run("-g", vcf, "-G", out, "-B", "0")
    assert r.returncode == 1 and b"Unrecognized permutations argument!" in r.stderr and not os.path.exists(out) and not os.path.exists(bed)
    c.close()
