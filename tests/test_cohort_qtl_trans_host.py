"""The trans-sQTL scan without a device: the contract of rgx_cohort_qtl_trans in include/regtools_amd.h as rgx_cohort_qtl_trans_host (the library's
plain C++ twin) keeps it, rgx_qtl_r_threshold, and the text.  Expectations: the restatement of tests/qtl_trans_ref.py -- yy, gg, r and slope as
bit patterns against exact fused multiply-adds in the contract's order, verdicts, hits and n_tested exactly --, the nominal scan's twin for the
pairs both see, and scipy's Student distribution for the threshold.  The tolerance constant: tests/qtl_trans_ref.py."""
import math

import numpy as np
import pytest

import cluster_cases
import pheno_cases as pc
import qtl_cases as qc
import qtl_trans_cases as tc
import qtl_trans_ref as tref

RGX_ERR_ARG = 7
FULL = 0xffffffff


def _twin(c, **kw):
    from regtools_amd import cohort
    a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, rank2=c.rank2, pval=tc.PVAL,
             exclude_window=qc.WINDOW)
    a.update(kw)
    rank2 = a.pop("rank2")
    return cohort.qtl_trans_host(cohort.pheno_table_from_rank2(rank2), **a)


@pytest.mark.parametrize("S, K, V, n_cov", tc.PLANTED)
def test_planted_cases_are_the_contract_s_bits(S, K, V, n_cov):
    from regtools_amd import cohort
    c = tc.case(S, K, V, n_cov)
    r_min = cohort.qtl_r_threshold(tc.PVAL, c.dof)
    want = tref.restate(c, cohort.quantile, r_min, qc.WINDOW)
    tc.check_conditions(c, want)
    q = _twin(c)
    tc.check_conditions(c, q)
    print("(%d, %d, %d, %d): %d hits of %d pairs, %d planted" % (S, K, V, n_cov, q.n_hits, q.n_tested, len(c.trans)))
    assert (q.n_rows, q.n_samples, q.n_variants, q.n_cov, q.dof) == (K, S, V, n_cov, S - n_cov - 2)
    tref.same_result(q, want)
    assert (q.n_tiles, q.n_hit_tiles) == (0, 0)
    # constant and explained variants lie between the usable ones: a hit's variant is not its place among the usable
    assert q.n_constant == c.n_constant and q.n_explained == (1 if n_cov else 0) and q.n_flat_rows == 0
    place = np.cumsum(q.variant_verdict == 0) - 1
    assert not np.isin(q.hit_variant, np.nonzero(q.variant_verdict)[0]).any() and (place[q.hit_variant] != q.hit_variant).any()
    # a row's hits ascend, every hit reaches the threshold, r has both signs somewhere among the cases' hits
    for k in range(K):
        assert (np.diff(q.hit_variant[q.hit_begin[k]:q.hit_begin[k + 1]].astype(np.int64)) > 0).all()
    assert (np.abs(q.r) >= r_min).all()
    # r_min given is the same call as pval given
    tref.same_result(_twin(c, r_min=r_min, pval=None), want)


def test_pairs_both_scans_see_have_the_same_bits():
    """No exclusion, r_min = 0, one contig: the hits are the nominal scan's pairs with the widest window, array for array."""
    from regtools_amd import cohort
    c = qc.simple(21, 13, 30, 2, seed=5, contigs=1)
    q = _twin(c, r_min=0.0, exclude_window=None)
    n = cohort.qtl_nominal_host(cohort.pheno_table_from_rank2(c.rank2), c.regions, c.var_tid, c.var_pos, c.dosage, c.cov, FULL)
    assert q.n_hits == n.n_pairs == q.n_tested == 13 * 30 and (q.variant_verdict == 0).all()
    assert np.array_equal(q.hit_begin, n.pair_begin) and np.array_equal(q.hit_variant, n.pair_variant)
    for f in ("r", "slope", "yy", "gg"):
        tref.ref.same_bits(getattr(q, f), getattr(n, f))
    assert (q.r < 0).any() and (q.r > 0).any()


def test_the_threshold_is_a_comparison_of_bits():
    c = tc.case(30, 20, 24, 2)
    every = _twin(c, r_min=0.0, exclude_window=None)
    neg = int(np.nonzero(every.r < 0)[0][len(np.nonzero(every.r < 0)[0]) // 2])        # a pair with a negative r somewhere in the middle
    for p in (neg, int(np.argmax(every.r)), int(np.argmin(np.abs(every.r)))):
        own = abs(float(every.r[p]))
        k = int(np.searchsorted(every.hit_begin, p, side="right")) - 1
        pair = (k, int(every.hit_variant[p]))
        kept = _twin(c, r_min=own, exclude_window=None)
        assert pair in tc.hit_pairs(kept) and kept.n_hits == int((np.abs(every.r) >= own).sum()) and kept.n_tested == every.n_tested
        dropped = _twin(c, r_min=math.nextafter(own, 2.0), exclude_window=None)
        assert pair not in tc.hit_pairs(dropped) and dropped.n_hits == int((np.abs(every.r) > own).sum())
        at = tc.hit_pairs(kept).index(pair)
        assert kept.r[at] == every.r[p] and kept.slope[at] == every.slope[p]
    assert every.r[neg] < 0
    # -0.0 is +0.0, and 1.0 keeps nothing here
    assert _twin(c, r_min=-0.0, exclude_window=None).n_hits == every.n_hits and _twin(c, r_min=1.0, exclude_window=None).n_hits == 0


def _edge_case(regions, variants, S=8, seed=2):
    """Rows with the given regions (tid, start, end) and variants (tid, pos), ascending; every variant usable, no row flat."""
    rng = np.random.default_rng(seed)
    K, V = len(regions), len(variants)
    dosage = rng.integers(0, 3, (V, S)).astype(np.int8)
    dosage[:, 0], dosage[:, 1] = 0, 2
    var = np.array(variants, np.uint32).reshape(-1, 2)
    return qc.Case(rank2=qc.rank2_of(rng.standard_normal((K, S))), regions=np.array(regions, np.uint32), var_tid=var[:, 0].copy(),
                   var_pos=var[:, 1].copy(), dosage=dosage, cov=np.zeros((0, S)), window=0)


def test_the_exclusion_s_edges():
    from regtools_amd import cohort
    start, end = 5000, 5200

    def met(region, variants, W):
        """The variants row 0 meets (r_min = 0: every pair that met is a hit), checked against the restatement."""
        c = _edge_case([region, (0, 1, 2), (1, 7, 9)], variants)
        q = _twin(c, r_min=0.0, exclude_window=W)
        tref.same_result(q, tref.restate(c, cohort.quantile, 0.0, W))
        assert (q.variant_verdict == 0).all() and q.n_flat_rows == 0
        return q.hit_variant[q.hit_begin[0]:q.hit_begin[1]].tolist()
    for W in (300, 0, 1):
        variants = [(0, start), (1, start - W - 1), (1, start - W), (1, end + W), (1, end + W + 1), (2, start)]
        assert met((1, start, end), variants, W) == [0, 1, 4, 5], W
        assert met((1, start, end), variants, None) == [0, 1, 2, 3, 4, 5]
    # the left side stops at 0, the right side at 2^32 - 1
    assert met((1, 5, 9), [(0, 0), (1, 0), (1, 1), (1, 19), (1, 20), (2, 0)], 10) == [0, 4, 5]
    assert met((1, FULL - 20, FULL - 10), [(0, FULL), (1, FULL - 121), (1, FULL - 120), (1, FULL), (2, FULL)], 100) == [0, 1, 4]
    assert met((1, 5, FULL - 10), [(0, 7), (1, 0), (1, FULL), (2, 7)], FULL) == [0, 3]
    # the other rows of those cases lie on their own contigs: the same position on another tid is not cis
    c = _edge_case([(1, start, end), (0, start, end)], [(0, start), (1, start)])
    assert tc.hit_pairs(_twin(c, r_min=0.0, exclude_window=5)) == [(0, 0), (1, 1)]


def test_max_hits_flat_rows_and_tables_without_hits():
    from regtools_amd import RegtoolsError
    c = tc.case(30, 20, 24, 2)
    q = _twin(c)
    H = q.n_hits
    assert H > 1 and _twin(c, max_hits=H).n_hits == H and _twin(c, max_hits=H + 1).n_hits == H and _twin(c, max_hits=2 ** 63).n_hits == H
    with pytest.raises(RegtoolsError) as e:
        _twin(c, max_hits=H - 1)
    assert e.value.code == RGX_ERR_ARG and "%d pairs" % H in str(e.value) and "at most %d" % (H - 1) in str(e.value)
    # a flat row: every sample the same rank
    r2 = c.rank2.copy()
    r2[4] = 20
    flat = _twin(c, rank2=r2, r_min=0.0)
    assert flat.n_flat_rows == 1 and flat.hit_begin[5] == flat.hit_begin[4] and flat.n_hits == flat.n_tested > 0
    from regtools_amd import cohort
    tref.same_result(flat, tref.restate(qc.Case(**dict(c.__dict__, rank2=r2)), cohort.quantile, 0.0, qc.WINDOW))
    # no variants at all, and none usable
    none = _twin(c, var_tid=np.zeros(0, np.uint32), var_pos=np.zeros(0, np.uint32), dosage=np.zeros((0, 30), np.int8), r_min=0.0)
    assert (none.n_hits, none.n_tested, none.n_variants) == (0, 0, 0) and not none.hit_begin.any() and len(none.hit_begin) == 21
    tref.ref.same_bits(none.yy, q.yy)
    none = _twin(c, dosage=np.where(np.arange(24)[:, None] % 2, -1, 2) * np.ones((24, 30), np.int8), r_min=0.0)
    assert (none.n_hits, none.n_tested, none.n_constant) == (0, 0, 24) and not none.hit_begin.any()
    # everything excluded: one contig, the widest window
    one = qc.simple(9, 5, 7, 0, seed=3, contigs=1)
    none = _twin(one, r_min=0.0, exclude_window=FULL)
    assert (none.n_hits, none.n_tested) == (0, 0)


def test_argument_errors():
    from regtools_amd import RegtoolsError
    c = tc.case(30, 20, 24, 2)

    def refused(**kw):
        with pytest.raises(RegtoolsError) as e:
            _twin(c, **kw)
        assert e.value.code == RGX_ERR_ARG, kw.keys()
        return e.value
    for bad in (math.nan, -1e-300, math.nextafter(1.0, 2.0), math.inf, -math.inf):
        assert "r_min" in str(refused(r_min=bad))
    refused(rank2=np.zeros((0, 30), np.uint32), regions=np.zeros((0, 3), np.uint32), r_min=0.5)                    # K == 0
    refused(covariates=np.random.default_rng(1).standard_normal((28, 30)), r_min=0.5)                          # S < n_cov + 3
    x = c.var_pos.copy()
    x[[0, 23]] = x[[23, 0]]
    refused(var_pos=x)                                                                                         # variants out of order
    assert "covariate 1" in str(refused(covariates=np.full((1, 30), 3.0)))
    for at in ((0, 0), (23, 29)):                                                                              # met by the twin
        d = c.dosage.copy()
        d[at] = 3
        assert "dosage" in str(refused(dosage=d))
        r2 = c.rank2.copy()
        r2[(0, 0) if at == (0, 0) else (19, 29)] = 41
        assert "rank2" in str(refused(rank2=r2))
    with pytest.raises(ValueError):
        _twin(c, exclude_window=2 ** 32)


def test_a_cohort_s_table_and_the_text():
    from regtools_amd import _ffi, cohort
    tables = pc.tables(pc.counts(9, 41, seed=9, absent=0.2))
    m = cohort.merge_host([cluster_cases.Sample(t) for t in tables], pc.names(9))
    cl = cohort.cluster_host(m)
    ph = cohort.phenotypes_host(m, cl, max_missing=(1, 1), min_sd=0.0)
    regions = cohort.pheno_regions(m, ph)
    tid, pos, dosage = qc.variants_near(regions, 9, 30, seed=4)
    pcs = cohort.pheno_pcs_host(ph, 2)
    q = cohort.qtl_trans_host(ph, regions, tid, pos, dosage, pcs.component, pval=0.05, exclude_window=50)
    c = qc.Case(rank2=ph.rank2, regions=regions, var_tid=tid, var_pos=pos, dosage=dosage, cov=pcs.component, window=0)
    tref.same_result(q, tref.restate(c, cohort.quantile, cohort.qtl_r_threshold(0.05, 9 - 2 - 2), 50))
    assert 1 < q.n_hits < q.n_tested < 41 * 30
    ids = [b"v%d" % i if i % 3 else b"%s:%d:A:T" % (m.ref_name[tid[i]].encode(), pos[i]) for i in range(30)]
    pheno_ids = [line.split(b"\t")[3].decode() for line in ph.text(m, cl).split(b"\n")[1:-1]]
    text = q.text(m, cl, ph, pos, ids)
    assert text == tref.text(pheno_ids, [i.decode() for i in ids], q, cohort.qtl_tstat, cohort.qtl_pvalue)
    assert text.count(b"\n") == q.n_hits + 1
    assert all(float(line.split(b"\t")[6]) <= 0.05 for line in text.split(b"\n")[1:-1])
    # a null result: the header line alone; a result of another table: nothing
    fn = _ffi.lib().rgx_cohort_format_qtl_trans
    assert cohort._text(fn, m._h, cl._h, ph._h, None, None, None) == b"phenotype_id\tvariant_id\tr\tslope\tslope_se\ttstat\tpval\n"
    assert _twin(tc.case(12, 9, 16, 0)).text(m, cl, ph, np.zeros(16, np.uint32), [b"x"] * 16) == b""
    cluster_cases.free_tables(tables)


def test_r_threshold_is_its_definition():
    from regtools_amd import cohort
    worst = 0.0
    for dof in tref.R_DOFS:
        for p in tref.R_PS:
            r = cohort.qtl_r_threshold(p, dof)
            assert 0.0 < r <= 1.0
            assert cohort.qtl_pvalue(cohort.qtl_tstat(r, dof), dof) <= p, (dof, p)
            assert cohort.qtl_pvalue(cohort.qtl_tstat(math.nextafter(r, 0.0), dof), dof) > p, (dof, p)
            want = tref.r_from_t_isf(p, dof)
            worst = max(worst, abs(r - want) / want)
            assert abs(r - want) <= tref.R_TOL * want, (dof, p, r, want)
    print("r_threshold against t.isf: off by %.3g relative (the two references: %.3g)" % (worst, tref.measure_r()))
    for dof in (1, 997):
        assert cohort.qtl_r_threshold(1.0, dof) == 0.0 and math.copysign(1.0, cohort.qtl_r_threshold(1.0, dof)) == 1.0
        assert cohort.qtl_r_threshold(2.5, dof) == 0.0 and cohort.qtl_r_threshold(math.inf, dof) == 0.0
        assert math.isnan(cohort.qtl_r_threshold(-1e-9, dof)) and math.isnan(cohort.qtl_r_threshold(math.nan, dof))
        assert cohort.qtl_r_threshold(0.0, dof) <= 1.0 and cohort.qtl_pvalue(cohort.qtl_tstat(cohort.qtl_r_threshold(0.0, dof), dof), dof) == 0.0
    assert math.isnan(cohort.qtl_r_threshold(0.5, 0))


def test_the_two_threshold_references_agree_within_the_tolerance():
    """The measurement behind R_MEASURED, repeated: neither reference is the code under test."""
    worst = tref.measure_r()
    print("t.isf against betaincinv: %.3g relative" % worst)
    assert worst <= tref.R_TOL
