"""The permutation pass of the cis-sQTL scan without a device: the contract of rgx_cohort_qtl_permute in include/regtools_amd.h as
rgx_cohort_qtl_permute_host (the library's plain C++ twin) keeps it, the permutation generator, the digamma, trigamma and incomplete beta functions,
the beta fit and the text.  Expectations: the restatement of tests/qtl_perm_ref.py -- perm_r as bit patterns against exact fused multiply-adds in
the contract's order --, the nominal twin's best pair, mpmath and scipy.

Tolerances, each four times what two references differ by (neither the code under test; measured by the tests themselves, printed, and recorded in
DESIGN 4.5h): scipy.special against mpmath at 50 digits over the points of qtl_perm_ref -- digamma 8.28e-17, trigamma 2.77e-16, betainc 3.47e-13
relative (this code: 7.75e-17, 6.35e-17, 1.35e-15); scipy.stats.beta.fit against mpmath.findroot on the digamma equations over the 30 rows of
the strong case: 5.25e-10 relative in the shapes (this code against scipy: 5.25e-10)."""
import math

import numpy as np
import pytest

import cluster_cases
import pheno_cases as pc
import qtl_cases as qc
import qtl_perm_cases as pcs
import qtl_perm_ref as pref
import qtl_ref as ref

RGX_ERR_ARG = 7
B_SMALL, S_SEED = 7, 11


def _table(c):
    from regtools_amd import cohort
    return cohort.pheno_table_from_rank2(c.rank2)


def _twin(c, **kw):
    from regtools_amd import cohort
    a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window, rank2=c.rank2,
             n_perm=B_SMALL, seed=S_SEED)
    a.update(kw)
    return cohort.qtl_permute_host(cohort.pheno_table_from_rank2(a.pop("rank2")), **a)


def test_the_generator():
    from regtools_amd import RegtoolsError, cohort
    assert next(pref.splitmix64(0)) == 0xe220a8397b1dcdaf
    p = cohort.qtl_permutations(8, 3, 1)
    assert p.dtype == np.uint16 and p.tolist() == [[0, 1, 2, 3, 4, 5, 6, 7], [0, 3, 7, 1, 2, 6, 5, 4], [0, 3, 6, 5, 2, 7, 1, 4], [6, 0, 5, 2, 4, 7, 1, 3]]
    for S, B, seed in ((1, 2, 0), (3, 5, 2 ** 64 - 1), (64, 9, 7), (2048, 2, 123456789012345)):
        got = cohort.qtl_permutations(S, B, seed)
        assert np.array_equal(got, pref.permutations(S, B, seed)), (S, B, seed)
        assert (np.sort(got, axis=1) == np.arange(S)).all()
    assert not np.array_equal(cohort.qtl_permutations(64, 1, 1), cohort.qtl_permutations(64, 1, 2))
    for S, B in ((0, 1), (65537, 1), (4, 65536)):
        with pytest.raises(RegtoolsError) as e:
            cohort.qtl_permutations(S, B, 0)
        assert e.value.code == RGX_ERR_ARG


def test_bad_permutations_are_refused():
    from regtools_amd import RegtoolsError
    c = qc.case(30, 20, 24, 2)
    good = pref.permutations(30, 4, 3)

    def refused(**kw):
        with pytest.raises(RegtoolsError) as e:
            _twin(c, **kw)
        assert e.value.code == RGX_ERR_ARG, kw.keys()
        return str(e.value)
    assert _twin(c, perms=good).n_perm == 4
    again = good.copy()
    again[3, 7] = again[3, 8]                                   # a repeated index
    assert "row 3" in refused(perms=again)
    out = good.copy()
    out[2, 0] = 30                                              # an index that is no sample
    assert "row 2" in refused(perms=out)
    shifted = good.copy()
    shifted[0, [4, 5]] = shifted[0, [5, 4]]                     # row 0 a permutation, not the identity
    assert "identity" in refused(perms=shifted)
    assert "identity" in refused(perms=good[1:])
    assert "1 to 65535" in refused(n_perm=0) and "1 to 65535" in refused(perms=good[:1])
    assert "1 to 65535" in refused(n_perm=65536)
    # the nominal scan's errors come first
    d = c.dosage.copy()
    d[0, 0] = 3
    assert "dosage" in refused(dosage=d)


def test_more_rows_times_permutations_than_the_result_can_index():
    """65,537 rows x (65,535 permutations + the identity) = 2^32 + 2^16, judged before anything is computed."""
    from regtools_amd import RegtoolsError
    K, S = 65537, 3
    rank2 = (2 * (np.argsort(np.random.default_rng(8).random((K, S)), axis=0) + 1)).astype(np.uint32)
    c = qc.Case(rank2=rank2, regions=np.tile(np.array([[0, 5, 9]], np.uint32), (K, 1)), var_tid=np.zeros(1, np.uint32),
                var_pos=np.ones(1, np.uint32), dosage=np.array([[0, 1, 2]], np.int8), cov=np.zeros((0, S)), window=10)
    with pytest.raises(RegtoolsError) as e:
        _twin(c, n_perm=65535)
    assert e.value.code == RGX_ERR_ARG and "2^32 - 2^16" in str(e.value)


@pytest.mark.parametrize("S, K, V, n_cov", qc.PLANTED)
def test_planted_cases_are_the_contract_s_bits(S, K, V, n_cov):
    from regtools_amd import cohort
    c = qc.case(S, K, V, n_cov)
    perms = pref.permutations(S, B_SMALL, S_SEED)
    want = pref.restate(c, cohort.quantile, perms)
    q = _twin(c)
    assert (q.n_rows, q.n_samples, q.n_variants, q.n_cov, q.dof, q.n_perm) == (K, S, V, n_cov, S - n_cov - 2, B_SMALL)
    assert q.perm_r.shape == (K, B_SMALL + 1)
    ref.same_bits(q.perm_r, want.perm_r)
    for f in ("n_ge", "n_cis", "best_variant", "variant_verdict"):
        assert np.array_equal(getattr(q, f), getattr(want, f)), f
    for f in ("yy", "gg", "best_r", "best_slope"):
        ref.same_bits(getattr(q, f), getattr(want, f))
    assert q.n_pairs == want.n_pairs > 0 and 4 * int((q.n_cis == 0).sum()) <= K
    assert np.array_equal(q.p_perm, (q.n_ge + 1.0) / (B_SMALL + 1.0))
    # the permutations took part: some row's largest |r| differs between the identity and a permutation, and n_ge counts in both directions
    assert (q.perm_r[:, 1:] != q.perm_r[:, :1]).any() and q.n_ge.max() > 0 and q.n_ge[q.n_cis > 0].min() < B_SMALL
    # explicit permutations are the seeded ones
    pref.same_perm_result(q, _twin(c, perms=perms))
    # a row without pairs
    assert q.n_cis[K - 1] == 0 and q.best_variant[K - 1] == pref.NO_PAIR and not q.perm_r[K - 1].any() and q.n_ge[K - 1] == B_SMALL
    assert q.beta_status[K - 1] == 2 and math.isnan(q.p_beta[K - 1]) and math.isnan(q.beta_shape1[K - 1])


@pytest.mark.parametrize("S, K, V, n_cov", qc.PLANTED + [pcs.STRONG])
def test_the_best_pair_is_the_nominal_scan_s(S, K, V, n_cov):
    from regtools_amd import cohort
    c = qc.case(S, K, V, n_cov) if (S, K, V, n_cov) != pcs.STRONG else pcs.strong_case()
    q, nom = _twin(c), cohort.qtl_nominal_host(_table(c), *c.args())
    has = nom.best != ref.NO_PAIR
    assert np.array_equal(q.n_cis, np.diff(nom.pair_begin.astype(np.int64))) and np.array_equal(q.n_cis > 0, has) and has.any()
    assert (q.best_variant[~has] == pref.NO_PAIR).all()
    assert np.array_equal(q.best_variant[has], nom.pair_variant[nom.best[has]])
    ref.same_bits(q.best_r[has], nom.r[nom.best[has]])
    ref.same_bits(q.best_slope[has], nom.slope[nom.best[has]])
    ref.same_bits(q.perm_r[:, 0][has], np.abs(nom.r[nom.best[has]]))
    for f in ("yy", "gg"):
        ref.same_bits(getattr(q, f), getattr(nom, f))
    assert np.array_equal(q.variant_verdict, nom.variant_verdict)
    assert (q.n_constant, q.n_explained, q.n_flat_rows, q.n_pairs, q.n_tiles) == (nom.n_constant, nom.n_explained, nom.n_flat_rows, nom.n_pairs, 0)


def test_identity_permutations_change_nothing():
    c = qc.case(65, 40, 40, 3)
    B = 5
    q = _twin(c, perms=np.tile(np.arange(65, dtype=np.uint16), (B + 1, 1)))
    assert np.array_equal(q.perm_r.view(np.uint64), np.repeat(q.perm_r[:, :1], B + 1, axis=1).view(np.uint64))
    assert (q.n_ge == B).all() and (q.p_perm == 1.0).all() and q.perm_r.any()
    assert (q.beta_status == 2).all()                           # (no variance among the permutations' p)


def test_strong_effects_stand_out_and_null_rows_do_not():
    """S = 64, K = 30, V = 40, B = 199; every third row carries 3 x the dosage of a variant inside its window."""
    c = pcs.strong_case()
    B = pcs.STRONG_B
    q = _twin(c, n_perm=B, seed=5)
    planted = np.arange(c.K) % 3 == 0
    print("n_cis", q.n_cis.tolist(), "n_ge", q.n_ge.tolist())
    assert 4 * int((q.n_cis == 0).sum()) <= c.K
    assert (q.n_cis[planted] > 0).all() and (q.n_ge[planted] == 0).all()
    assert np.array_equal(q.best_variant[planted], c.anchor[planted])
    null = ~planted & (q.n_cis > 0)
    assert 2 * int((q.n_ge[null] >= B / 10).sum()) >= int(null.sum()) > 0
    assert np.array_equal(q.p_perm, (q.n_ge + 1.0) / (B + 1.0)) and (q.p_perm[planted] == 1.0 / (B + 1)).all()
    # the beta approximation says the same: planted rows far below every permutation's reach, the others near their empirical p
    assert (q.beta_status == 0).all() and (q.p_beta[planted] < 1e-6).all()
    assert (np.abs(q.p_beta[null] - q.p_perm[null]) < 0.1).all()


def test_digamma_trigamma_and_the_incomplete_beta_function():
    import mpmath
    from regtools_amd import cohort
    sd, st, si = pref.measure_special(*pref.scipy_special())
    md, mt, mi = pref.measure_special(cohort.qtl_digamma, cohort.qtl_trigamma, cohort.qtl_betainc)
    print("largest relative error against mpmath: digamma scipy %.3g, this %.3g; trigamma %.3g, %.3g; betainc %.3g, %.3g" % (sd, md, st, mt, si, mi))
    assert 0 < sd and 0 < st and 0 < si
    assert md <= 4 * sd and mt <= 4 * st and mi <= 4 * si
    with mpmath.workdps(50):                                    # (point by point, so that a failure names its point)
        for x in pref.PSI_X:
            assert pref.rel(cohort.qtl_digamma(x), mpmath.digamma(mpmath.mpf(x))) <= 4 * sd, x
            assert pref.rel(cohort.qtl_trigamma(x), mpmath.polygamma(1, mpmath.mpf(x))) <= 4 * st, x
        for a in pref.BETA_AB:
            for b in pref.BETA_AB:
                for x in pref.BETA_X:
                    want = mpmath.betainc(mpmath.mpf(a), mpmath.mpf(b), 0, mpmath.mpf(x), regularized=True)
                    assert pref.rel(cohort.qtl_betainc(x, a, b), want) <= 4 * si, (x, a, b)
    assert cohort.qtl_betainc(0.0, 2.0, 3.0) == 0.0 and cohort.qtl_betainc(1.0, 2.0, 3.0) == 1.0
    for bad in ((-0.1, 1, 1), (1.1, 1, 1), (0.5, 0, 1), (0.5, 1, -2), (math.nan, 1, 1)):
        assert math.isnan(cohort.qtl_betainc(*bad))
    assert math.isnan(cohort.qtl_digamma(0.0)) and math.isnan(cohort.qtl_trigamma(-1.0))
    # I_x(dof / 2, 1 / 2) at x = dof / (dof + t^2) is the two-sided p of Student's t
    for dof, t in ((10, 2.0), (997, 4.5), (3, 0.5)):
        assert abs(cohort.qtl_betainc(dof / (dof + t * t), dof / 2.0, 0.5) - cohort.qtl_pvalue(t, dof)) <= ref.P_TOL * cohort.qtl_pvalue(t, dof)


def test_the_fit_against_a_reference_maximiser():
    from scipy.special import betainc
    from regtools_amd import cohort
    c = pcs.strong_case()
    q = _twin(c, n_perm=pcs.STRONG_B, seed=5)
    si = pref.measure_special(*pref.scipy_special())[2]
    between, mine, rows = 0.0, 0.0, []
    for k in range(c.K):
        if not q.n_cis[k]:
            continue
        p = pref.perm_pvalues(q, k, cohort.qtl_tstat, cohort.qtl_pvalue)
        assert cohort.qtl_beta_fit(p) == (int(q.beta_status[k]), q.beta_shape1[k], q.beta_shape2[k]) and q.beta_status[k] == 0
        a_s, b_s = pref.fit_reference(p)
        a_m, b_m = pref.fit_mpmath(p)
        between = max(between, abs(a_s - a_m) / a_m, abs(b_s - b_m) / b_m)
        rows.append((k, a_s, b_s))
        mine = max(mine, abs(q.beta_shape1[k] - a_s) / a_s, abs(q.beta_shape2[k] - b_s) / b_s)
        x = cohort.qtl_pvalue(cohort.qtl_tstat(float(q.best_r[k]), q.dof), q.dof)
        want = betainc(q.beta_shape1[k], q.beta_shape2[k], x)
        assert abs(q.p_beta[k] - want) <= 4 * si * want, (k, q.p_beta[k], want)
    print("shapes over %d rows: scipy.stats.beta.fit against mpmath.findroot %.3g relative, this code against scipy %.3g" % (len(rows), between, mine))
    assert len(rows) >= 20 and between > 0
    for k, a_s, b_s in rows:
        assert abs(q.beta_shape1[k] - a_s) <= 4 * between * a_s and abs(q.beta_shape2[k] - b_s) <= 4 * between * b_s, k
    # what cannot be fitted
    assert cohort.qtl_beta_fit([0.3])[0] == 2 and cohort.qtl_beta_fit([0.3, 0.3, 0.3])[0] == 2 and cohort.qtl_beta_fit([0.5, 1.0])[0] == 2
    assert all(math.isnan(x) for x in cohort.qtl_beta_fit([0.3])[1:])


def test_one_permutation_has_no_fit():
    c = qc.case(12, 9, 16, 0)
    q = _twin(c, n_perm=1)
    assert (q.beta_status == 2).all() and np.isnan(q.p_beta).all() and set(q.p_perm[q.n_cis > 0]) <= {0.5, 1.0}


def _cohort_table():
    from regtools_amd import cohort
    tables = pc.tables(pc.counts(9, 41, seed=9, absent=0.2))
    m = cohort.merge_host([cluster_cases.Sample(t) for t in tables], pc.names(9))
    cl = cohort.cluster_host(m)
    return tables, m, cl, cohort.phenotypes_host(m, cl, max_missing=(1, 1), min_sd=0.0)


def test_a_cohort_s_table_and_the_text():
    from regtools_amd import cohort
    tables, m, cl, ph = _cohort_table()
    regions = cohort.pheno_regions(m, ph)
    tid, pos, dosage = qc.variants_near(regions, 9, 30, seed=4)
    pcs_ = cohort.pheno_pcs_host(ph, 2)
    B = 40
    q = cohort.qtl_permute_host(ph, regions, tid, pos, dosage, pcs_.component, qc.WINDOW, n_perm=B, seed=3)
    c = qc.Case(rank2=ph.rank2, regions=regions, var_tid=tid, var_pos=pos, dosage=dosage, cov=pcs_.component, window=qc.WINDOW)
    want = pref.restate(c, cohort.quantile, pref.permutations(9, B, 3))
    ref.same_bits(q.perm_r, want.perm_r)
    assert np.array_equal(q.n_ge, want.n_ge) and np.array_equal(q.best_variant, want.best_variant) and 0 < int((q.n_cis > 0).sum())
    ids = [b"v%d" % i if i % 3 else b"%s:%d:A:T" % (m.ref_name[tid[i]].encode(), pos[i]) for i in range(30)]
    pheno_ids = [line.split(b"\t")[3].decode() for line in ph.text(m, cl).split(b"\n")[1:-1]]
    text = q.text(m, cl, ph, pos, ids)
    assert text == pref.text(pheno_ids, [i.decode() for i in ids], pos, regions[:, 1], q, cohort.qtl_tstat, cohort.qtl_pvalue)
    assert text.count(b"\n") == int((q.n_cis > 0).sum()) + 1
    head = text.split(b"\n")[0].split(b"\t")
    assert head[0] == b"phenotype_id" and head[-3:] == [b"pval_nominal", b"pval_perm", b"pval_beta"] and len(head) == 14
    # NaN is written as nan: a result of one permutation has no fit
    one = cohort.qtl_permute_host(ph, regions, tid, pos, dosage, pcs_.component, qc.WINDOW, n_perm=1, seed=3)
    t1 = one.text(m, cl, ph, pos, ids)
    assert t1 == pref.text(pheno_ids, [i.decode() for i in ids], pos, regions[:, 1], one, cohort.qtl_tstat, cohort.qtl_pvalue)
    assert b"\tnan\tnan\t" in t1 and t1.endswith(b"\tnan\n") and b"-nan" not in t1
    # the header alone; the buffer protocol; a result of another table
    import ctypes as C
    from regtools_amd import _ffi
    fn = _ffi.lib().rgx_cohort_format_qtl_perm
    arr = (C.c_char_p * 30)(*ids)
    n = fn(m._h, cl._h, ph._h, None, None, None, None, 0)
    buf = C.create_string_buffer(n + 1)
    assert fn(m._h, cl._h, ph._h, None, None, None, buf, n) == n and buf.raw[:n] == text.split(b"\n")[0] + b"\n"
    small = C.create_string_buffer(b"\x7f" * 8, 8)
    assert fn(m._h, cl._h, ph._h, q._h, pos.ctypes.data, arr, small, 8) == len(text) and small.raw == b"\x7f" * 8
    assert _twin(qc.case(12, 9, 16, 0)).text(m, cl, ph, np.zeros(16, np.uint32), [b"x"] * 16) == b""
    cluster_cases.free_tables(tables)
