"""The grouped permutation pass of the cis-sQTL scan without a device: the contract of rgx_cohort_qtl_permute_grouped in include/regtools_amd.h as
rgx_cohort_qtl_permute_grouped_host (the library's plain C++ twin) keeps it, rgx_cohort_pheno_groups and the text.  Expectations: the restatement
of tests/qtl_group_ref.py -- the permuted chains with exact fused multiply-adds in the contract's order, the maxima over a group's members in
Python integers --, the ungrouped twin of the same input (singleton groups reproduce it; every group is the maximum of its members), and expected
indices written out where the tie rule decides.

The null case, measured with the twin before its condition was fixed: of the ten groups of two null rows of the strong case, B = 199,
seed 5, ten have n_ge >= B / 10 (n_ge = 50, 85, 177, 55, 189, 198, 107, 87, 81, 72); the condition is at least half of them."""
import functools
import math

import numpy as np
import pytest

import cluster_cases
import pheno_cases as pc
import qtl_cases as qc
import qtl_group_cases as gc
import qtl_group_ref as gref
import qtl_perm_cases as pcs
import qtl_perm_ref as pref
import qtl_ref as ref

RGX_ERR_ARG = 7
B_SMALL, S_SEED = 7, 11
GROUPINGS = {"singletons": gc.singletons, "one": gc.one_group, "round_robin": gc.round_robin}


def _args(c, **kw):
    a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window, rank2=c.rank2,
             n_perm=B_SMALL, seed=S_SEED)
    a.update(kw)
    return a


def _twin(c, groups, G, **kw):
    from regtools_amd import cohort
    a = _args(c, **kw)
    return cohort.qtl_permute_grouped_host(cohort.pheno_table_from_rank2(a.pop("rank2")), groups=groups, n_groups=G, **a)


def _ungrouped(c, **kw):
    from regtools_amd import cohort
    a = _args(c, **kw)
    return cohort.qtl_permute_host(cohort.pheno_table_from_rank2(a.pop("rank2")), **a)


@functools.lru_cache(maxsize=None)
def _rows_restated(S, K, V, n_cov):
    """qtl_perm_ref.restate of a planted case, once for its three groupings."""
    from regtools_amd import cohort
    return pref.restate(qc.case(S, K, V, n_cov), cohort.quantile, pref.permutations(S, B_SMALL, S_SEED))


@pytest.mark.parametrize("grouping", sorted(GROUPINGS))
@pytest.mark.parametrize("S, K, V, n_cov", qc.PLANTED)
def test_planted_cases_are_the_contract_s_bits(S, K, V, n_cov, grouping):
    c = qc.case(S, K, V, n_cov)
    groups, G = GROUPINGS[grouping](K)
    want = gref.restate(_rows_restated(S, K, V, n_cov), groups, G)
    q = _twin(c, groups, G)
    assert (q.n_rows, q.n_samples, q.n_variants, q.n_cov, q.dof, q.n_perm, q.n_groups) == (K, S, V, n_cov, S - n_cov - 2, B_SMALL, G)
    assert q.perm_r.shape == (G, B_SMALL + 1) and q.n_tiles == 0
    for f in ("perm_r", "best_r", "best_slope"):
        ref.same_bits(getattr(q, f), getattr(want, f))
    for f in ("n_ge", "group_n_cis", "best_row", "best_variant", "grp_begin", "grp_row"):
        assert np.array_equal(getattr(q, f), getattr(want, f)), f
    for f in ("yy", "gg"):
        ref.same_bits(getattr(q, f), getattr(want.rows, f))
    assert np.array_equal(q.n_cis, want.rows.n_cis) and np.array_equal(q.variant_verdict, want.rows.variant_verdict)
    assert q.n_pairs == want.n_pairs > 0 and np.array_equal(q.p_perm, (q.n_ge + 1.0) / (B_SMALL + 1.0))
    assert (q.perm_r[:, 1:] != q.perm_r[:, :1]).any()
    ung = _ungrouped(c)
    gref.max_identity(q, ung, groups, G)
    gref.max_identity(q, want.rows, groups, G)
    if grouping == "round_robin":                               # (row 1 is in no group; the groups are not contiguous)
        assert 1 not in q.grp_row and q.n_pairs == ung.n_pairs - ung.n_cis[1] and (np.diff(q.grp_row[q.grp_begin[0]:q.grp_begin[1]]) == 3).all()
    if grouping == "singletons":
        gref.same_as_ungrouped(q, ung)
        gref.no_pairs(q, K - 1)                                 # (the planted row that no variant reaches)


@pytest.mark.parametrize("S, K, V, n_cov", qc.PLANTED + [pcs.STRONG])
def test_singleton_groups_reproduce_the_ungrouped_pass(S, K, V, n_cov):
    """Every array, NaN included: the beta approximation goes through one function."""
    strong = (S, K, V, n_cov) == pcs.STRONG
    c = pcs.strong_case() if strong else qc.case(S, K, V, n_cov)
    kw = dict(n_perm=pcs.STRONG_B, seed=5) if strong else {}
    groups, G = gc.singletons(K)
    q, ung = _twin(c, groups, G, **kw), _ungrouped(c, **kw)
    gref.same_as_ungrouped(q, ung)
    assert (q.n_constant, q.n_explained, q.n_flat_rows) == (ung.n_constant, ung.n_explained, ung.n_flat_rows)
    if strong:
        assert (q.beta_status == 0).all()
    else:
        assert np.isnan(q.p_beta).any() and (q.beta_status != 2).any()


def test_the_ungrouped_twin_is_the_grouped_twin_of_singleton_groups():
    """One product loop and one finish behind both twins: S = 17, five rows of 0, 1, 65, 0 and 64 cis variants, B = 64, group[k] = k."""
    c = gc.merged_case()
    groups, G = gc.singletons(5)
    q, ung = _twin(c, groups, G, n_perm=64), _ungrouped(c, n_perm=64)
    assert tuple(ung.n_cis) == gc.MERGED_COUNTS and (ung.variant_verdict == 0).all() and ung.n_samples == 17
    assert q.perm_r.shape == ung.perm_r.shape == (5, 65) and q.n_ge.shape == ung.n_ge.shape == (5,)
    gref.same_as_ungrouped(q, ung)                              # (perm_r, best_*, n_ge, p_perm, the shapes and p_beta as bit patterns; best_row)
    assert q.best_row.tolist() == [gc.NO_PAIR, 1, 2, gc.NO_PAIR, 4]
    assert (q.n_constant, q.n_explained, q.n_flat_rows, q.n_tiles) == (ung.n_constant, ung.n_explained, ung.n_flat_rows, ung.n_tiles)
    for g in (0, 3):
        gref.no_pairs(q, g)
    assert (q.perm_r[[1, 2, 4], 1:] != q.perm_r[[1, 2, 4], :1]).any() and (q.beta_status[[1, 2, 4]] != 2).all()


def _nominal_top(c):
    """(row, variant) of the largest |r| of the whole table by the nominal twin, with the rows and variants that reach the same bits."""
    from regtools_amd import cohort
    nom = cohort.qtl_nominal_host(cohort.pheno_table_from_rank2(c.rank2), *c.args())
    bits = np.abs(nom.r).view(np.uint64)
    at = np.nonzero(bits == bits.max())[0]
    row_of = np.searchsorted(nom.pair_begin, at, side="right") - 1
    return sorted(zip(row_of.tolist(), nom.pair_variant[at].tolist()))


def test_ties_go_to_the_lowest_row_and_then_to_the_earliest_variant():
    groups, G = gc.one_group(8)
    # two members with the same rank2 row
    c = gc.tie_rows()
    assert _nominal_top(c) == [(1, 3), (4, 3)]
    q = _twin(c, groups, G)
    assert (q.best_row[0], q.best_variant[0]) == (1, 3)
    # two variants with the same dosages, the other one behind and in front of the best
    c = gc.tie_variants(5)
    assert _nominal_top(c) == [(1, 3), (1, 5)]
    q = _twin(c, groups, G)
    assert (q.best_row[0], q.best_variant[0]) == (1, 3)
    c = gc.tie_variants(0)
    assert _nominal_top(c) == [(1, 0), (1, 3)]
    q = _twin(c, groups, G)
    assert (q.best_row[0], q.best_variant[0]) == (1, 0)
    # a later variant of an earlier row against an earlier variant of a later row
    c = gc.tie_across()
    assert _nominal_top(c) == [(1, 5), (4, 3)]
    q = _twin(c, groups, G)
    assert (q.best_row[0], q.best_variant[0]) == (1, 5)
    gref.max_identity(q, _ungrouped(c), groups, G)
    # ... and with the two rows in different groups each group has its own
    two = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.uint32)
    q = _twin(c, two, 2)
    assert q.best_row.tolist() == [1, 4] and q.best_variant.tolist() == [5, 3]
    ref.same_bits(q.perm_r[0, :1], q.perm_r[1, :1])


def test_groups_without_pairs_and_members_without_cis_variants():
    """An empty group, a group of flat rows alone and a lone row that no variant reaches have no pairs: +0.0, RGX_NO_PAIR, status 2 (and no
    text line: test_a_cohort_s_table_and_the_text).  A member without cis variants -- the first, a middle or the last of its group -- adds
    nothing: its group is the group of the other members."""
    c, groups, G, empty = gc.degenerate()
    q, ung = _twin(c, groups, G), _ungrouped(c)
    assert q.n_flat_rows == 2 and [int(ung.n_cis[k]) for k in (0, 3, 7, 12, 13, 19)] == [0] * 6
    for g in empty:
        gref.no_pairs(q, g)
    assert q.grp_begin.tolist() == [0, 3, 6, 9, 11, 11, 12]
    gref.max_identity(q, ung, groups, G)
    assert np.signbit(q.perm_r).sum() == 0
    without = groups.copy()
    without[[0, 7, 19]] = gc.NO_GROUP
    q2 = _twin(c, without, G)
    for g in (0, 1, 2):
        assert q.group_n_cis[g] > 0 and q.beta_status[g] != 2 and q.best_row[g] in gc.members(without, g)
        ref.same_bits(q.perm_r[g], q2.perm_r[g])
        assert (q.best_row[g], q.best_variant[g], q.n_ge[g], q.group_n_cis[g]) == (q2.best_row[g], q2.best_variant[g], q2.n_ge[g], q2.group_n_cis[g])
        ref.same_bits([q.p_beta[g], q.beta_shape1[g], q.beta_shape2[g]], [q2.p_beta[g], q2.beta_shape1[g], q2.beta_shape2[g]])
    # no row in any group at all
    q = _twin(c, np.full(20, gc.NO_GROUP, np.uint32), 2)
    assert q.n_pairs == 0 and len(q.grp_row) == 0 and ung.n_pairs > 0 and np.array_equal(q.n_cis, ung.n_cis)
    for g in (0, 1):
        gref.no_pairs(q, g)


def test_bad_groups_are_refused():
    from regtools_amd import RegtoolsError
    c = qc.case(30, 20, 24, 2)
    groups, G = gc.round_robin(20)

    def refused(groups, G, **kw):
        with pytest.raises(RegtoolsError) as e:
            _twin(c, groups, G, **kw)
        assert e.value.code == RGX_ERR_ARG
        return str(e.value)
    assert _twin(c, groups, G).n_groups == 3
    bad = groups.copy()
    bad[7] = 3
    assert "row 7 is of group 3" in refused(bad, 3)
    bad[7] = 0xfffffffe
    assert "row 7" in refused(bad, 3)
    assert "1 to 2^31 - 1 groups" in refused(groups, 0) and "1 to 2^31 - 1 groups" in refused(groups, 2 ** 31)
    # the ungrouped call's errors
    assert "1 to 65535" in refused(groups, G, n_perm=0)
    d = c.dosage.copy()
    d[0, 0] = 3
    assert "dosage" in refused(groups, G, dosage=d)
    shifted = pref.permutations(30, 4, 3)
    shifted[0, [4, 5]] = shifted[0, [5, 4]]
    assert "identity" in refused(groups, G, perms=shifted)
    with pytest.raises(ValueError):
        _twin(c, groups[:-1], G)


def test_more_groups_times_permutations_than_the_result_can_index():
    """65,537 groups x (65,535 permutations + the identity) = 2^32 + 2^16, judged before anything is computed -- whatever the rows: 9 rows here, for
    which the ungrouped limit K (B + 1) is far away."""
    from regtools_amd import RegtoolsError
    c = qc.case(12, 9, 16, 0)
    groups = np.zeros(9, np.uint32)
    with pytest.raises(RegtoolsError) as e:
        _twin(c, groups, 65537, n_perm=65535)
    assert e.value.code == RGX_ERR_ARG and "65537 groups" in str(e.value) and "2^32 - 2^16" in str(e.value)
    assert _ungrouped(c, n_perm=3).n_perm == 3


def test_strong_effects_stand_out_in_their_groups_and_null_groups_do_not():
    """S = 64, K = 30, V = 40, B = 199; rows grouped in threes, so that each group holds one planted row; then the planted rows in groups of their
    own behind ten groups of two null rows."""
    c = pcs.strong_case()
    B = pcs.STRONG_B
    threes = (np.arange(c.K) // 3).astype(np.uint32)
    q = _twin(c, threes, 10, n_perm=B, seed=5)
    print("grouped in threes: n_ge", q.n_ge.tolist(), "best_row", q.best_row.tolist())
    assert (q.n_ge == 0).all() and q.best_row.tolist() == list(range(0, 30, 3))
    assert np.array_equal(q.best_variant, c.anchor[::3]) and (q.p_perm == 1.0 / (B + 1)).all()
    assert (q.beta_status == 0).all() and (q.p_beta < 1e-6).all()
    ung = _ungrouped(c, n_perm=B, seed=5)
    gref.max_identity(q, ung, threes, 10)
    apart = threes.copy()
    apart[::3] = 10 + np.arange(10)
    q = _twin(c, apart, 20, n_perm=B, seed=5)
    null = q.n_ge[:10]
    print("null groups: n_ge", null.tolist(), "pairs", q.group_n_cis[:10].tolist())
    assert (q.group_n_cis[:10] > 0).all() and 2 * int((null >= B / 10).sum()) >= 10
    assert (q.n_ge[10:] == 0).all() and q.best_row[10:].tolist() == list(range(0, 30, 3))
    gref.max_identity(q, ung, apart, 20)
    assert (np.abs(q.p_beta[:10] - q.p_perm[:10]) < 0.1).all()


def _cohort_table(**kw):
    from regtools_amd import cohort
    tables = pc.tables(pc.counts(9, 41, seed=9, absent=0.2))
    m = cohort.merge_host([cluster_cases.Sample(t) for t in tables], pc.names(9))
    cl = cohort.cluster_host(m)
    return tables, m, cl, cohort.phenotypes_host(m, cl, **kw)


def test_pheno_groups():
    from regtools_amd import RegtoolsError, cohort
    # 41 rows in 20 clusters: 19 pairs of rows and one cluster of three
    tables, m, cl, ph = _cohort_table(max_missing=(1, 1), min_sd=0.0)
    groups, G = cohort.pheno_groups(cl, ph)
    assert groups.dtype == np.uint32 and G == 20 and groups.tolist() == [k // 2 for k in range(40)] + [19]
    # with the rows that miss a sample left out, 27 rows of 13 clusters stay: the clusters' numbers have gaps, the groups' have none
    ph2 = cohort.phenotypes_host(m, cl, max_missing=(1, 10), min_sd=0.0)
    assert cl.cluster[ph2.row].tolist() == [0, 0, 2, 2, 3, 3, 5, 5, 7, 7, 8, 8, 9, 9, 11, 11, 14, 14, 15, 15, 16, 16, 17, 17, 19, 19, 19]
    groups, G = cohort.pheno_groups(cl, ph2)
    assert G == 13 and groups.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 12]
    # a clustering that dropped the table's clusters
    big = cohort.cluster_host(m, min_rows=3)
    assert big.n_clusters == 1
    with pytest.raises(RegtoolsError) as e:
        cohort.pheno_groups(big, ph)
    assert e.value.code == RGX_ERR_ARG and "not clustered" in str(e.value)
    cluster_cases.free_tables(tables)


def test_a_cohort_s_table_and_the_text():
    from regtools_amd import cohort
    tables, m, cl, ph = _cohort_table(max_missing=(1, 1), min_sd=0.0)
    regions = cohort.pheno_regions(m, ph)
    tid, pos, dosage = qc.variants_near(regions, 9, 30, seed=4)
    pcs_ = cohort.pheno_pcs_host(ph, 2)
    B = 40
    groups, G = cohort.pheno_groups(cl, ph)
    q = cohort.qtl_permute_grouped_host(ph, regions, groups, G, tid, pos, dosage, pcs_.component, qc.WINDOW, n_perm=B, seed=3)
    c = qc.Case(rank2=ph.rank2, regions=regions, var_tid=tid, var_pos=pos, dosage=dosage, cov=pcs_.component, window=qc.WINDOW)
    want = gref.restate(pref.restate(c, cohort.quantile, pref.permutations(9, B, 3)), groups, G)
    ref.same_bits(q.perm_r, want.perm_r)
    for f in ("n_ge", "best_row", "best_variant", "group_n_cis"):
        assert np.array_equal(getattr(q, f), getattr(want, f)), f
    ung = cohort.qtl_permute_host(ph, regions, tid, pos, dosage, pcs_.component, qc.WINDOW, n_perm=B, seed=3)
    gref.max_identity(q, ung, groups, G)
    ids = [b"v%d" % i if i % 3 else b"%s:%d:A:T" % (m.ref_name[tid[i]].encode(), pos[i]) for i in range(30)]
    sids = [i.decode() for i in ids]
    pheno_ids = [line.split(b"\t")[3].decode() for line in ph.text(m, cl).split(b"\n")[1:-1]]
    text = q.text(m, cl, ph, pos, ids)
    assert text == gref.text(pheno_ids, sids, pos, regions[:, 1], q, cohort.qtl_tstat, cohort.qtl_pvalue)
    n_lines = int((q.group_n_cis > 0).sum())
    assert text.count(b"\n") == n_lines + 1 and 0 < n_lines
    lines = [x.split(b"\t") for x in text.split(b"\n")[:-1]]
    assert lines[0][:4] == [b"group_id", b"group_size", b"phenotype_id", b"num_var"] and lines[0][-3:] == [b"pval_nominal", b"pval_perm", b"pval_beta"]
    assert all(len(x) == 16 for x in lines) and all(x[2].endswith(b":" + x[0]) and x[0].startswith(b"clu_") for x in lines[1:])
    assert lines[-1][:2] == [b"clu_20_+", b"3"] or q.group_n_cis[19] == 0
    # groups without pairs have no line: an empty group in front, a group of flat rows alone (rows 4 and 5), rows in no group
    r2 = ph.rank2.copy()
    r2[4] = r2[5] = 12
    g2 = groups + 1
    g2[[8, 9]] = gc.NO_GROUP
    flat = cohort.qtl_permute_grouped_host(cohort.pheno_table_from_rank2(r2), regions, g2, G + 1, tid, pos, dosage, pcs_.component, qc.WINDOW, n_perm=B,
                                           seed=3)
    gref.no_pairs(flat, 0)
    gref.no_pairs(flat, 3)
    gref.no_pairs(flat, 5)
    t2 = flat.text(m, cl, ph, pos, ids)
    assert t2 == gref.text(pheno_ids, sids, pos, regions[:, 1], flat, cohort.qtl_tstat, cohort.qtl_pvalue)
    assert t2.count(b"\n") == int((flat.group_n_cis > 0).sum()) + 1 and b"clu_3_" not in t2 and b"clu_5_" not in t2 and flat.n_flat_rows == 2
    # NaN is written as nan: a result of one permutation has no fit
    one = cohort.qtl_permute_grouped_host(ph, regions, groups, G, tid, pos, dosage, pcs_.component, qc.WINDOW, n_perm=1, seed=3)
    t1 = one.text(m, cl, ph, pos, ids)
    assert t1 == gref.text(pheno_ids, sids, pos, regions[:, 1], one, cohort.qtl_tstat, cohort.qtl_pvalue)
    assert b"\tnan\tnan\t" in t1 and t1.endswith(b"\tnan\n") and b"-nan" not in t1
    # the header alone; the buffer protocol; a result of another table
    import ctypes as C
    from regtools_amd import _ffi
    fn = _ffi.lib().rgx_cohort_format_qtl_group
    arr = (C.c_char_p * 30)(*ids)
    n = fn(m._h, cl._h, ph._h, None, None, None, None, 0)
    buf = C.create_string_buffer(n + 1)
    assert fn(m._h, cl._h, ph._h, None, None, None, buf, n) == n and buf.raw[:n] == gref.HEAD.encode() == text.split(b"\n")[0] + b"\n"
    small = C.create_string_buffer(b"\x7f" * 8, 8)
    assert fn(m._h, cl._h, ph._h, q._h, pos.ctypes.data, arr, small, 8) == len(text) and small.raw == b"\x7f" * 8
    other = qc.case(12, 9, 16, 0)
    assert _twin(other, *gc.one_group(9)).text(m, cl, ph, np.zeros(16, np.uint32), [b"x"] * 16) == b""
    cluster_cases.free_tables(tables)


def test_one_permutation_has_no_fit():
    c = qc.case(12, 9, 16, 0)
    q = _twin(c, *gc.round_robin(9), n_perm=1)
    assert (q.beta_status == 2).all() and np.isnan(q.p_beta).all() and set(q.p_perm) <= {0.5, 1.0} and not math.isnan(q.best_r[0])
