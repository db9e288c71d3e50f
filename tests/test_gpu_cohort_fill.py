"""The cohort calls on workspaces filled with NaN, ones and guard bytes (REGTOOLS_AMD_FILL: CohortRun::carved, csrc/cohort_internal.h).

Device memory is cleared when it is handed out, and the host twins build their results in zeroed memory: a workspace word that no kernel
wrote reads as 0 on first use and as whatever the call before left on later ones, so a result word the device never wrote equals the twin's 0 by
luck.  With the fill mode on, every floating-point array of every cohort workspace starts as a quiet NaN, every integer array as ones, and
everything behind a workspace's last array as the guard byte 0xA5, whose first 256 bytes come back with the results: a changed byte fails the
call.  Every comparison here is the one the call's own GPU test makes -- the device equals the host twin in every array, as bit patterns -- and
the twin never sees the fill.  (a) each call at the edges where its kernels leave words unwritten, (b) a large, a small and the large call again
on one cohort, mode on and off, (d) the trans scan's map from workgroups to tiles at every band.  (c): every call of these tests returns
success, so no workspace's tail was touched; the guard's failure path is tested on the CPU (tests/test_hostemu.py).

With the mode on the library found nothing: no word read before it was written, no tail touched.

That these tests can fail was shown once, on scratch builds with one-line faults (the unwritten word a value or a flag, never an index):
  (i) the conditional run without its hipMemsetAsync(cflag, 0, 8, st): 19 tests here fail, each call refused ("a variant a series is conditioned on is constant or
      explained by the covariates") by the flag word's 1 -- test_qtl_permute_conditional_under_the_fill (all 14 cases), test_qtl_independent_under_the_fill[planted_signals, every_fit_enters,
      S17] (the two cases without a conditional round pass), test_history_of_qtl_permute_conditional and test_history_of_qtl_independent.  The
      existing suite catches it too, with the mode off: 45 tests of test_gpu_cohort_qtl_cond.py fail, the first of the module among them -- inside one process a new allocation is memory an earlier cohort freed, not zeros.
  (ii) k_qtl_cond_best without the stores of best_r and best_slope in its no-place branch: test_qtl_permute_conditional_under_the_fill
      [K130_V200_alternating] (a collinear series) and [mixed_list] fail here, the NaN against the twin's +0.0.  The existing suite catches it in
      test_gpu_cohort_qtl_cond.py::test_a_mixed_list_of_series and ::test_the_narrowest_and_the_widest_window[0], by what the series before left.
  (iii) k_qtl_trans_count without the three stores of a tile behind the last usable variant: test_qtl_trans_under_the_fill[K63_V65_alternating,
      K130_V130_alternating, K130_V200_alternating, all_constant, unusable_between] and test_history_of_qtl_trans fail here, by n_hits and
      n_tested, which count the ones of such tiles -- wrong results, no more.  With the mode OFF the same fault is not a value any longer: in
      test_gpu_cohort_qtl_trans.py::test_unusable_variants_between_usable_ones the stale flag and count of such a tile (left by the call before,
      whose tiles were all full) made hits of slots the emit kernel never wrote, k_qtl_trans_gather took the bits a nominal-sized layout had
      left there as hit_u, and u_var[hit_u] was an illegal memory access, after which every later test of the process failed.  That run is not
      to be repeated; under the fill the unwritten words are 1 and stay inside the arrays, which is what the mode is for.
No fault was caught under the fill alone: (i) and (ii) also fail the existing suite, by the luck of what the calls before left; (iii) fails it
by a memory fault instead of a wrong count.
"""
import contextlib
import os

import numpy as np
import pytest

import cluster_cases
import cluster_ref
import pca_cases as pca
import pheno_cases as pc
import pheno_ref
import qtl_cases as qc
import qtl_cond_cases as cc
import qtl_group_cases as gc
import qtl_perm_cases as pcs
import refine_ref
import test_gpu_cohort_clusters as t_clusters
import test_gpu_cohort_edges as t_edges
import test_gpu_cohort_pcs as t_pcs
import test_gpu_cohort_pheno as t_pheno
import test_gpu_cohort_qtl as t_nom
import test_gpu_cohort_qtl_cond as t_cond
import test_gpu_cohort_qtl_group as t_group
import test_gpu_cohort_qtl_perm as t_perm
import test_gpu_cohort_qtl_trans as t_trans
import test_gpu_cohort_refine as t_refine

pytestmark = pytest.mark.gpu

FILL, BAND = "REGTOOLS_AMD_FILL", "REGTOOLS_AMD_TRANS_BAND"


@contextlib.contextmanager
def env(**kw):
    """The library reads both switches per call: set for the block, then as before."""
    was = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in was.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def filled():
    return env(**{FILL: 1})


@pytest.fixture(scope="module")
def co(gpu_ctx):
    """One cohort without samples for the whole module: every workspace of a call holds what the calls before it left."""
    import regtools_amd
    c = regtools_amd.Cohort(ctx=gpu_ctx)
    yield c
    c.close()


# ---- (a) the matrix, the clusters, the table and its components ------------------------------------------------------------------------------
# (samples, rows): a wave's trips and the eight-lane forms at S = 8, 9, 17, 65; one and several blocks of rows
SHAPES = [(8, 63), (9, 65), (17, 130), (65, 130), (9, 1)]


def _counts(S, n_rows):
    """A third of the entries absent, sample 1 without a read anywhere (its column of the table is one tie), equal rows."""
    empty = [(1, 0, 1)] if S > 1 else []
    return pc.counts(S, n_rows, seed=S * 1000 + n_rows, absent=0.3, empty_clusters=empty, duplicates=2 if n_rows >= 24 else 0)


@contextlib.contextmanager
def _chain(gpu_ctx, S, n_rows, **cohort_kw):
    """(the cohort of the shape's tables, the twin's matrix of the same samples)"""
    import regtools_amd
    from regtools_amd import cohort
    tables = pc.tables(_counts(S, n_rows))
    own = regtools_amd.Cohort(ctx=gpu_ctx, **cohort_kw)
    try:
        for t, nm in zip(tables, pc.names(S)):
            own.add(cluster_cases.Sample(t), nm)
        yield own, cohort.merge_host([cluster_cases.Sample(t) for t in tables], pc.names(S), **cohort_kw)
    finally:
        own.close()
        cluster_cases.free_tables(tables)


def _drop_some(h):
    """A min_total that takes about half of the clusters: their rows are rows without a cluster."""
    from regtools_amd import cohort
    every = cohort.cluster_host(h)
    return dict(min_total=int(np.median(every.cl_total))) if every.n_clusters > 1 else dict()


@pytest.mark.parametrize("S, n_rows", SHAPES)
def test_finish_under_the_fill(gpu_ctx, S, n_rows):
    """The key sort, the heads, the row reduction with rows that the filters drop (min_samples: keep = 0 between kept rows) and the image."""
    for kw in (dict(), dict(min_samples=max(2, 3 * S // 4), min_total=S * 10)):
        with filled(), _chain(gpu_ctx, S, n_rows, **kw) as (own, h):
            m = own.finish()
            t_edges._same_matrix(m, h)
            assert kw == {} or m.n < n_rows or n_rows == 1
            again = own.finish()                                         # (a second finish cuts both workspaces anew over what the first left)
            t_edges._same_matrix(again, h)


@pytest.mark.parametrize("S, n_rows", SHAPES)
def test_cluster_under_the_fill(gpu_ctx, co, S, n_rows):
    """Both matrix paths, without filters and with a min_total that leaves rows without a cluster and clusters without denominators."""
    from regtools_amd import cohort
    with filled(), _chain(gpu_ctx, S, n_rows) as (own, h):
        m = own.finish()
        for kw in (dict(), _drop_some(h), dict(min_rows=4)):             # (min_rows = 4: no cluster stays, no entry workspace)
            twin = cohort.cluster_host(h, **kw)
            for who, mat, path in ((own, m, 1), (co, h, 0)):
                cl = who.cluster(mat, **kw)
                assert who.cluster_paths[-1] == path
                cluster_ref.same_clusters(cl, twin)
                assert cl.counts_text(mat) == twin.counts_text(h)
    if n_rows == 130:
        with filled():
            t_clusters.test_hand_made_cohort_on_both_paths(gpu_ctx)
            t_clusters.test_filters_that_keep_no_cluster(gpu_ctx)


@pytest.mark.parametrize("S, n_rows", SHAPES)
def test_refine_under_the_fill(gpu_ctx, co, S, n_rows):
    """Rows that are not eligible, rows that are weak (both compactions, the second search) and parameters that remove nothing."""
    from regtools_amd import cohort
    with filled(), _chain(gpu_ctx, S, n_rows) as (own, h):
        m = own.finish()
        reads = int(np.median(h.total)) if n_rows > 1 else 1
        for kw in (dict(), dict(min_reads=reads), dict(max_intron=43, min_reads=reads, min_ratio=(1, 3)), dict(max_intron=1)):
            twin = cohort.refine_host(h, **kw)
            for who, mat, path in ((own, m, 1), (co, h, 0)):
                rf = who.refine(mat, **kw)
                assert who.cluster_paths[-1] == path
                refine_ref.same_clusters(rf, twin)
                assert (rf.n_ineligible, rf.n_weak) == (twin.n_ineligible, twin.n_weak) and rf.counts_text(mat) == twin.counts_text(h)
            if kw.get("max_intron") == 43 and n_rows > 2:
                assert twin.n_ineligible > 0 and twin.n_weak > 0
    if n_rows == 130:
        with filled():
            t_refine.test_hand_made_cohort_on_both_paths(gpu_ctx)
            t_refine.test_the_ratio_test_is_made_on_the_whole_products(gpu_ctx)


@pytest.mark.parametrize("S, n_rows", SHAPES)
def test_phenotypes_under_the_fill(gpu_ctx, co, S, n_rows):
    """Rows without a cluster between clustered ones (k_pheno_row_stats leaves their n_na, mean and sd), rows the filters drop, a column that
    is one tie; both matrix paths."""
    from regtools_amd import cohort
    with filled(), _chain(gpu_ctx, S, n_rows) as (own, h):
        m = own.finish()
        for ckw in (dict(), _drop_some(h)):
            clh = cohort.cluster_host(h, **ckw)
            cl = own.cluster(m, **ckw)
            for kw in (dict(), dict(max_missing=(1, 1), min_sd=0.0)):
                twin = cohort.phenotypes_host(h, clh, **kw)
                for ph in (own.phenotypes(m, cl, **kw), co.phenotypes(h, clh, **kw)):
                    pheno_ref.same_tables(ph, twin)
                if ckw and n_rows >= 63:
                    assert (clh.cluster == 0xffffffff).any() and 0 < twin.n_clustered < n_rows
                if kw and n_rows >= 63:
                    assert twin.n_rows == twin.n_clustered and (twin.rank2[:, 1] == twin.n_rows + 1).all()       # (sample 1: one tie)
    if n_rows == 130:
        with filled():
            t_pheno.test_sample_counts_around_the_wave(gpu_ctx, S)
            t_pheno.test_one_row_kept_and_no_row_kept(gpu_ctx)


@pytest.mark.parametrize("S", [8, 9, 17, 65])
@pytest.mark.parametrize("K", [2, 63, 65, 130])             # (the call takes no table of one row)
def test_pheno_pcs_under_the_fill(co, K, S):
    """One tile and three (six tile pairs with their mirrored halves), slabs with a partial last one, the pad columns of the column sums."""
    with filled():
        t_pcs._check(co, pca.random_rank2(K, S, seed=K * 100 + S))


# ---- (a) the five sQTL passes --------------------------------------------------------------------------------------------------------------
def _alternating(c):
    """Every other variant constant: half of the tiles of usable variants are partial or behind the last usable one."""
    d = c.dosage.copy()
    d[1::2] = 1
    return qc.Case(**dict(c.__dict__, dosage=d))


def _flat_row(c, k=3):
    r2 = c.rank2.copy()
    r2[k] = c.K + 1
    return qc.Case(**dict(c.__dict__, rank2=r2))


def _no_variants(c):
    return qc.Case(**dict(c.__dict__, var_tid=np.zeros(0, np.uint32), var_pos=np.zeros(0, np.uint32), dosage=np.zeros((0, c.S), np.int8)))


def _all_constant(c):
    return qc.Case(**dict(c.__dict__, dosage=(np.where(np.arange(c.V)[:, None] % 2, -1, 2) * np.ones((c.V, c.S))).astype(np.int8)))


def _qtl_cases():
    """name -> a thunk: planted tables with constant and explained variants between usable ones and a flat row, tables without pairs, and the
    sample, row and variant counts at the waves', blocks' and tiles' edges."""
    out = {"planted_flat_row": lambda: _flat_row(qc.case(30, 20, 24, 2)),
           "no_variants": lambda: _no_variants(qc.case(30, 20, 24, 2)),
           "all_constant": lambda: _all_constant(qc.case(30, 20, 24, 2))}
    for S in (8, 9, 17, 65):
        out["S%d" % S] = lambda S=S: qc.planted(S, 20, 24, 1, seed=S * 100 + 1)
    for K, V in ((1, 1), (63, 65), (65, 63), (130, 130), (130, 200)):
        out["K%d_V%d" % (K, V)] = lambda K=K, V=V: qc.simple(9, K, V, 1, seed=K * 1000 + V, span=4 * qc.WINDOW, contigs=1)
        if V > 1:
            out["K%d_V%d_alternating" % (K, V)] = lambda K=K, V=V: _alternating(qc.simple(9, K, V, 1, seed=K * 1000 + V, span=4 * qc.WINDOW, contigs=1))
    return out


QTL = _qtl_cases()


@pytest.mark.parametrize("name", sorted(QTL))
def test_qtl_nominal_under_the_fill(co, name):
    with filled():
        dev, _ = t_nom._check(co, QTL[name]())
        if name == "planted_flat_row":
            assert dev.n_flat_rows == 1 and dev.n_constant > 0 and dev.n_explained > 0 and dev.n_pairs > 0
        if name.endswith("alternating"):
            assert dev.n_constant == dev.n_variants // 2


@pytest.mark.parametrize("name", sorted(QTL))
def test_qtl_permute_under_the_fill(co, name):
    """5 permutations, and 129: one block of 64 with its pad columns, and three with a partial last one."""
    with filled():
        c = QTL[name]()
        t_perm._check(co, c, n_perm=5, seed=3)
        if c.K <= 65:
            t_perm._check(co, c, n_perm=129, seed=4)


@pytest.mark.parametrize("name", sorted(QTL) + ["degenerate"])
def test_qtl_permute_grouped_under_the_fill(co, name):
    """Runs of one to eight rows, rows in no group, and the groups without pairs and members without cis variants of qtl_group_cases."""
    with filled():
        if name == "degenerate":
            t_group.test_groups_without_pairs_and_members_without_cis_variants(co)
            return
        c = QTL[name]()
        groups, G = gc.runs(c.K, seed=c.K + c.V)
        t_group._check(co, c, groups, G, n_perm=5, seed=3)
        if c.K >= 3:
            groups, G = gc.round_robin(c.K)
            t_group._check(co, c, groups, G + 2, n_perm=66, seed=5)       # (two empty groups behind the three)


@pytest.mark.parametrize("name", sorted(QTL) + ["six_hits", "unusable_between"])
def test_qtl_trans_under_the_fill(co, name):
    """Every pair a hit (every tile full) and few hits (tiles without hits between tiles with hits); tiles behind the last usable variant."""
    with filled():
        if name == "six_hits":
            t_trans.test_tiles_without_hits_between_tiles_with_hits(co)
        elif name == "unusable_between":
            t_trans.test_unusable_variants_between_usable_ones(co)
        else:
            c = QTL[name]()
            t_trans._check(co, c, r_min=0.0, exclude_window=None)
            t_trans._check(co, c, pval=0.05)


def _series_of(c, seed):
    from regtools_amd import cohort
    return cc.draw(cc.cis_lists(c, cohort), (1, 2, 3), seed=seed, per_size=6)


# (a series needs a row with two cis variants: the tables without usable variants and the table of one row have none)
@pytest.mark.parametrize("name", sorted(set(QTL) - {"no_variants", "all_constant", "K1_V1"}) + ["mixed_list"])
def test_qtl_permute_conditional_under_the_fill(co, name):
    """Series of one to three conditioning variants; the mixed list: collinear sets (yc left), flat rows, series that lose every variant (beta
    and gg' left)."""
    with filled():
        if name == "mixed_list":
            t_cond.test_a_mixed_list_of_series(co)
            return
        c = QTL[name]()
        series = _series_of(c, seed=c.K + c.V)
        assert len(series) >= 3
        t_cond._check(co, c, series, n_perm=5, seed=3)
        t_cond._check(co, c, series[:3], n_perm=129, seed=4)


def _indep_small():
    return cc.indep_case(n_two=6, n_one=6, n_null=8, n_tag=4)            # 24 rows x 168 variants x 120 samples


def _indep(co, c, **kw):
    a = dict(n_perm=129, p_threshold=0.01)
    a.update(kw)
    return t_cond._indep(co, c, **a)


@pytest.mark.parametrize("name", ["planted_signals", "capped", "every_fit_enters", "S17", "no_variants"])
def test_qtl_independent_under_the_fill(co, name):
    """Round 0 and every later round cut the conditional workspace anew over what the round before left; 129 permutations."""
    with filled():
        if name == "planted_signals":
            dev, _ = _indep(co, _indep_small())
            assert dev.n_entered > 0 and dev.n_forward_rounds >= 2 and (dev.rank > 1).any()
        elif name == "capped":
            dev, _ = _indep(co, _indep_small(), max_signals=1)
            assert dev.n_forward_rounds == 0 and dev.n_capped == dev.n_entered == dev.n_signals
        elif name == "every_fit_enters":
            dev, _ = _indep(co, cc.indep_case(n_two=3, n_one=3, n_null=3, n_tag=2, per_row=10), max_signals=8, p_threshold=1.0)
            assert dev.n_capped > 0 and dev.n_forward_rounds == 7
        elif name == "S17":
            _indep(co, qc.planted(17, 20, 24, 1, seed=1701), n_perm=99, seed=2, p_threshold=0.5, max_signals=3)
        else:
            dev, _ = _indep(co, _no_variants(qc.case(30, 20, 24, 2)), n_perm=9, seed=1)
            assert dev.n_signals == 0 and dev.n_forward_rounds == 0


# ---- (b) call history: large, small, large on one cohort, mode on and then off -----------------------------------------------------------------
def _large():
    """130 rows (three blocks) x 200 variants (every other one constant: two tiles of usable ones) x 17 samples."""
    return _alternating(qc.simple(17, 130, 200, 1, seed=130200, span=4 * qc.WINDOW, contigs=1))


def _small():
    """Two rows, one variant, four samples: the least the scans take (one row alone is flat).  One block, one tile, leading dimensions of 64."""
    return qc.simple(4, 2, 1, 0, seed=421, span=4 * qc.WINDOW, contigs=1)


def _small_wide():
    """Five rows of nine samples, the first with three cis variants: the least the conditional passes take a series of."""
    return pcs.rows_with(9, 3, 8, seed=938)


def _history(call):
    """call(which) with which = 'large', 'small', 'large': under the fill, then without it; every one of the six compares with its twin."""
    for mode in (1, None):
        with env(**{FILL: mode}):
            for which in ("large", "small", "large"):
                call(which)


def test_history_of_qtl_nominal(co):
    c = {"large": _large(), "small": _small()}
    _history(lambda w: t_nom._check(co, c[w]))


def test_history_of_qtl_permute(co):
    c = {"large": _large(), "small": _small()}
    _history(lambda w: t_perm._check(co, c[w], n_perm=129 if w == "large" else 1, seed=7))


def test_history_of_qtl_permute_grouped(co):
    c = {"large": _large(), "small": _small()}
    g = {"large": gc.runs(130, seed=13), "small": (np.zeros(2, np.uint32), 1)}
    _history(lambda w: t_group._check(co, c[w], g[w][0], g[w][1], n_perm=129 if w == "large" else 1, seed=7))


def test_history_of_qtl_trans(co):
    c = {"large": _large(), "small": _small()}

    def call(w):
        t_trans._check(co, c[w], r_min=0.0, exclude_window=None)
        t_trans._check(co, c[w], pval=0.05, exclude_window=None)
    _history(call)


def test_history_of_qtl_permute_conditional(co):
    c = {"large": _large(), "small": _small_wide()}
    from regtools_amd import cohort
    series = {"large": _series_of(c["large"], seed=5), "small": [(0, cc.cis_lists(c["small"], cohort)[0][:1])]}
    assert len(series["large"]) >= 12 and len(series["small"][0][1]) == 1
    _history(lambda w: t_cond._check(co, c[w], series[w], n_perm=129 if w == "large" else 1, seed=7))


def test_history_of_qtl_independent(co):
    c = {"large": _indep_small(), "small": _small_wide()}
    kw = {"large": dict(), "small": dict(n_perm=5, p_threshold=1.0, max_signals=2)}
    _history(lambda w: _indep(co, c[w], **kw[w]))


def test_history_of_cluster_and_phenotypes(co):
    """The uploaded path on the module's cohort: 130 rows of 65 samples, then four rows of three samples (two clusters, every row kept), then
    the 130 again."""
    from regtools_amd import cohort
    made = {}
    try:
        for w, count in (("large", _counts(65, 130)), ("small", pc.counts(3, 4, seed=34))):
            S = count.shape[1]
            tables = pc.tables(count)
            made[w] = (tables, cohort.merge_host([cluster_cases.Sample(t) for t in tables], pc.names(S)))
        ckw = {"large": _drop_some(made["large"][1]), "small": dict()}

        def call(w):
            h = made[w][1]
            cl, twin = co.cluster(h, **ckw[w]), cohort.cluster_host(h, **ckw[w])
            cluster_ref.same_clusters(cl, twin)
            rf, rtwin = co.refine(h, min_reads=1, min_ratio=(1, 50)), cohort.refine_host(h, min_reads=1, min_ratio=(1, 50))
            refine_ref.same_clusters(rf, rtwin)
            kw = dict(max_missing=(1, 1), min_sd=0.0)
            pheno_ref.same_tables(co.phenotypes(h, twin, **kw), cohort.phenotypes_host(h, twin, **kw))
        _history(call)
    finally:
        for tables, _ in made.values():
            cluster_cases.free_tables(tables)


# ---- (d) which workgroup runs which trans tile ---------------------------------------------------------------------------------------------
# (rows, variants) -> row blocks x variant tiles: 1 x 1, 3 x 4, 5 x 3, 9 x 2 and 4 x 4 -- 1, 12, 15, 18 and 16 tiles, so that the eight runs of
# places are equal (16) and unequal, and the row blocks are and are not a multiple of the band.  (5 x 3 and 9 x 2 take 260 and 520 rows.)
TILES = {(20, 24): (1, 1), (130, 200): (3, 4), (260, 130): (5, 3), (520, 70): (9, 2), (200, 200): (4, 4)}
GRIDS = sorted(TILES)
BANDS = [0, 1, 2, 3, 4, 5, 64]


@pytest.mark.parametrize("K, V", GRIDS)
def test_every_band_visits_every_trans_tile_once(co, K, V):
    """trans_tile_of is a bijection from workgroups to tiles at every band: with the per-tile words filled with ones, a tile no workgroup visits
    counts one hit and one tested pair, and a tile visited twice leaves another without a visit.  Every pair a hit, then six hits."""
    c = qc.simple(30, K, V, 0, seed=31 if (K, V) == (130, 200) else K + V, contigs=1)       # (130 x 200: the case of the six hits in test_gpu_cohort_qtl_trans.py)
    n_blocks, n_vt = TILES[(K, V)]
    with filled():
        with env(**{BAND: None}):
            every, _ = t_trans._check(co, c, r_min=0.0, exclude_window=None)
        r_min = float(np.sort(np.abs(every.r))[-6])
        n_few = int((np.abs(every.r) >= r_min).sum())
        assert 6 <= n_few <= 8
        for band in BANDS:
            with env(**{BAND: band}):
                dev, _ = t_trans._check(co, c, r_min=0.0, exclude_window=None)
                assert dev.n_tiles == n_blocks * n_vt == dev.n_hit_tiles and dev.n_hits == dev.n_tested == K * V
                few, _ = t_trans._check(co, c, r_min=r_min, exclude_window=None)
                assert few.n_hits == n_few and few.n_tested == K * V and few.n_hit_tiles <= min(n_few, few.n_tiles)
