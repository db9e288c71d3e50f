"""The nominal cis-sQTL scan without a device: the contract of rgx_cohort_qtl_nominal in include/regtools_amd.h as rgx_cohort_qtl_nominal_host (the
library's plain C++ twin) keeps it, the t and p functions, and the text.  Expectations: the restatement of tests/qtl_ref.py -- yy, gg, r and slope as
bit patterns against exact fused multiply-adds in the contract's order, verdicts and pairs exactly --, ordinary least squares of the full model
(numpy.linalg.lstsq) for slope and t, and scipy's Student distribution for p.  The tolerance constants: tests/qtl_ref.py."""
import math

import numpy as np
import pytest

import cluster_cases
import pheno_cases as pc
import qtl_cases as qc
import qtl_ref as ref

RGX_ERR_ARG = 7
C_TOL, P_TOL = ref.C_TOL, ref.P_TOL


def _twin(c, **kw):
    from regtools_amd import cohort
    a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window, rank2=c.rank2)
    a.update(kw)
    rank2 = a.pop("rank2")
    return cohort.qtl_nominal_host(cohort.pheno_table_from_rank2(rank2), **a)


@pytest.mark.parametrize("S, K, V, n_cov", qc.PLANTED)
def test_planted_cases_are_the_contract_s_bits(S, K, V, n_cov):
    from regtools_amd import cohort
    c = qc.case(S, K, V, n_cov)
    want = ref.restate(c, cohort.quantile)
    qc.check_conditions(c, want)
    q = _twin(c)
    qc.check_conditions(c, q)
    assert (q.n_rows, q.n_samples, q.n_variants, q.n_cov, q.dof) == (K, S, V, n_cov, S - n_cov - 2)
    ref.same_result(q, want)
    # what was planted is there: constant variants, the explained one, equal positions, two contigs, a row out of reach
    assert q.n_constant == c.n_constant == int((q.variant_verdict == 1).sum()) and (q.gg[q.variant_verdict == 1] == 0).all()
    assert q.n_explained == (1 if n_cov else 0) and q.n_flat_rows == 0
    if n_cov:
        assert q.variant_verdict[c.special[c.n_constant]] == 2
    assert (np.diff(c.var_pos.astype(np.int64))[np.diff(c.var_tid.astype(np.int64)) == 0] == 0).any() and len(set(c.var_tid)) == 2
    assert q.pair_begin[K] == q.pair_begin[K - 1] and q.best[K - 1] == ref.NO_PAIR
    assert not np.isin(q.pair_variant, np.nonzero(q.variant_verdict)[0]).any()


@pytest.mark.parametrize("S, K, V, n_cov", qc.PLANTED)
def test_slope_and_t_against_least_squares_of_the_full_model(S, K, V, n_cov):
    from regtools_amd import cohort
    c = qc.case(S, K, V, n_cov)
    q = _twin(c)
    rows = np.array(ref.quantile_table(K, cohort.quantile))[c.rank2.astype(np.int64) - 2]
    worst, strongest = [0.0, 0.0], 0.0
    for k in range(K):
        for p in range(q.pair_begin[k], q.pair_begin[k + 1]):
            y, g, Z = ref.model(c, k, int(q.pair_variant[p]), rows)
            b, se, t = ref.ols(y, g, Z)
            u_slope, u_t = ref.bounds(c, q.r[p], q.yy[k], q.gg[q.pair_variant[p]], g)
            mine_t = cohort.qtl_tstat(q.r[p], q.dof)
            worst = [max(worst[0], abs(q.slope[p] - b) / u_slope), max(worst[1], abs(mine_t - t) / u_t)]
            assert abs(q.slope[p] - b) <= C_TOL * u_slope and abs(mine_t - t) <= C_TOL * u_t, (k, p)
            # slope_se = slope / t is the fit's standard error (relative: both errors and a few roundings)
            assert abs(q.slope[p] / mine_t - se) <= (C_TOL * (u_slope / abs(b) + u_t / abs(t)) + 8 * ref.EPS) * se
            strongest = max(strongest, abs(mine_t))
    print("(%d, %d, %d, %d): slope off by %.3f, t by %.3f units of S eps scale" % (S, K, V, n_cov, worst[0], worst[1]))
    assert strongest > 4 or S < 30                               # (a planted effect was found, where the samples can show one)


def test_the_two_references_agree_within_the_tolerance():
    """The measurement behind C_MEASURED and P_MEASURED, repeated: neither reference is the code under test."""
    from regtools_amd import cohort
    worst, n = ref.measure_c(cohort.quantile, [qc.case(*s) for s in qc.PLANTED])
    print("lstsq against QR residuals over %d pairs: slope %.4f, t %.4f; t.sf against betainc: %.3g" % (n, worst[0], worst[1], ref.measure_p()))
    assert n >= 300 and max(worst) <= C_TOL and ref.measure_p() <= P_TOL


def test_t_and_p():
    from regtools_amd import cohort
    for dof in ref.P_DOFS:
        assert cohort.qtl_pvalue(0.0, dof) == 1.0 and cohort.qtl_pvalue(-0.0, dof) == 1.0
        assert cohort.qtl_pvalue(math.inf, dof) == 0.0 and cohort.qtl_pvalue(-math.inf, dof) == 0.0
        assert math.isnan(cohort.qtl_pvalue(math.nan, dof))
        worst = 0.0
        for t in ref.P_TS[1:]:
            want, got = ref.t_sf_p(t, dof), cohort.qtl_pvalue(t, dof)
            assert got == cohort.qtl_pvalue(-t, dof)
            worst = max(worst, abs(got - want) / want)
            assert abs(got - want) <= P_TOL * want, (dof, t, got, want)
        print("dof %d: p off by %.3g relative" % (dof, worst))
    assert cohort.qtl_tstat(1.0, 5) == math.inf and cohort.qtl_tstat(-1.0, 5) == -math.inf
    assert cohort.qtl_tstat(0.0, 5) == 0.0
    for r, dof in ((0.5, 10), (-0.25, 3), (0.999, 997)):
        assert cohort.qtl_tstat(r, dof) == r * math.sqrt(dof / (1.0 - r * r))


def test_windows_and_tables_without_pairs():
    from regtools_amd import cohort
    c = qc.case(30, 20, 24, 2)
    for window in (0, 1, 0xffffffff):
        want = ref.restate(qc.Case(**dict(c.__dict__, window=window)), cohort.quantile)
        ref.same_result(_twin(c, window=window), want)
        if window == 0xffffffff:                                 # every usable variant of the row's contig
            usable_on = [int(((c.var_tid == t) & (want.variant_verdict == 0)).sum()) for t in c.regions[:, 0]]
            assert list(np.diff(want.pair_begin.astype(np.int64))) == usable_on
    # no variants at all, and none usable
    q = _twin(c, var_tid=np.zeros(0, np.uint32), var_pos=np.zeros(0, np.uint32), dosage=np.zeros((0, 30), np.int8))
    assert q.n_pairs == 0 and q.n_variants == 0 and (q.best == ref.NO_PAIR).all() and not q.pair_begin.any()
    whole = _twin(c)                                             # (the arrays are views: the result must outlive the comparison)
    ref.same_bits(q.yy, whole.yy)
    q = _twin(c, dosage=np.where(np.arange(24)[:, None] % 2, -1, 2) * np.ones((24, 30), np.int8))
    assert q.n_pairs == 0 and q.n_constant == 24 and (q.variant_verdict == 1).all()
    # a flat row: every sample the same rank
    r2 = c.rank2.copy()
    r2[3] = 20
    q = _twin(c, rank2=r2)
    assert q.n_flat_rows == 1 and q.pair_begin[4] == q.pair_begin[3] and q.best[3] == ref.NO_PAIR
    ref.same_result(q, ref.restate(qc.Case(**dict(c.__dict__, rank2=r2)), cohort.quantile))


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
    assert regions.shape == (41, 3)
    assert np.array_equal(regions, np.stack([m.tid[ph.row], m.start[ph.row], m.end[ph.row]], axis=1))
    tid, pos, dosage = qc.variants_near(regions, 9, 30, seed=4)
    pcs = cohort.pheno_pcs_host(ph, 2)
    q = cohort.qtl_nominal_host(ph, regions, tid, pos, dosage, pcs.component, qc.WINDOW)
    c = qc.Case(rank2=ph.rank2, regions=regions, var_tid=tid, var_pos=pos, dosage=dosage, cov=pcs.component, window=qc.WINDOW)
    qc.check_conditions(c, q)
    ref.same_result(q, ref.restate(c, cohort.quantile))
    ids = [b"v%d" % i if i % 3 else b"%s:%d:A:T" % (m.ref_name[tid[i]].encode(), pos[i]) for i in range(30)]
    pheno_ids = [line.split(b"\t")[3].decode() for line in ph.text(m, cl).split(b"\n")[1:-1]]
    text = q.text(m, cl, ph, pos, ids)
    assert text == ref.text(pheno_ids, [i.decode() for i in ids], pos, regions[:, 1], q, cohort.qtl_tstat, cohort.qtl_pvalue)
    assert text.count(b"\n") == q.n_pairs + 1 and text.count(b"\t1\n") == int((q.best != ref.NO_PAIR).sum())
    # the buffer protocol: the size without a buffer, nothing written into one that is too small
    import ctypes as C
    from regtools_amd import _ffi
    fn = _ffi.lib().rgx_cohort_format_qtl
    arr = (C.c_char_p * 30)(*ids)
    small = C.create_string_buffer(b"\x7f" * 8, 8)
    assert fn(m._h, cl._h, ph._h, q._h, pos.ctypes.data, arr, small, 8) == len(text) and small.raw == b"\x7f" * 8
    # a result of another table
    assert _twin(qc.case(12, 9, 16, 0)).text(m, cl, ph, np.zeros(16, np.uint32), [b"x"] * 16) == b""
    cluster_cases.free_tables(tables)


def test_genotypes_from_a_vcf(tmp_path):
    """Samples by name, dosages from GT, the three kinds of records left out, the stable order, the made-up identifiers; plain and gzip."""
    import gzip
    from regtools_amd import RegtoolsError, cohort
    tables, m, cl, ph = _cohort_table()
    regions = cohort.pheno_regions(m, ph)
    names = list(m.sample_name)
    vcf = str(tmp_path / "v.vcf")
    tid, pos, dosage, ids, skipped = qc.write_vcf(vcf, m, regions, 220, seed=3, samples=names[::-1][:4] + ["other"] + names[::-1][4:])
    with open(vcf, "rb") as f, gzip.open(vcf + ".gz", "wb") as z:
        z.write(f.read())
    for path in (vcf, vcf + ".gz"):
        g = cohort.genotypes(path, m)
        assert np.array_equal(g.tid, tid) and np.array_equal(g.pos, pos) and np.array_equal(g.dosage, dosage)
        assert [i.decode() for i in g.ids] == ids
        assert (g.n_records, [g.n_multiallelic, g.n_no_gt, g.n_unknown_contig]) == (220, skipped) and min(skipped) > 0
    assert set(np.unique(dosage)) == {-1, 0, 1, 2} and (np.diff(pos.astype(np.int64))[np.diff(tid.astype(np.int64)) == 0] == 0).any()
    qc.write_vcf(vcf, m, regions, 20, seed=3, samples=names[1:])
    with pytest.raises(RegtoolsError) as e:
        cohort.genotypes(vcf, m)
    assert e.value.code == RGX_ERR_ARG and "Sample %s has no genotypes in %s" % (names[0], vcf) in str(e.value)
    with pytest.raises(RegtoolsError):
        cohort.genotypes(str(tmp_path / "absent.vcf"), m)
    cluster_cases.free_tables(tables)


def test_argument_errors():
    from regtools_amd import RegtoolsError
    c = qc.case(30, 20, 24, 2)

    def refused(**kw):
        with pytest.raises(RegtoolsError) as e:
            _twin(c, **kw)
        assert e.value.code == RGX_ERR_ARG, kw.keys()
        return e.value
    refused(rank2=np.zeros((0, 30), np.uint32), regions=np.zeros((0, 3), np.uint32))                     # K == 0
    refused(rank2=np.full((1, 2049), 2, np.uint32), regions=c.regions[:1], dosage=np.zeros((24, 2049), np.int8),
            covariates=None)                                                                             # S > 2048
    # K > 2^31 - 1, judged before anything is read: the table's row count alone says so
    import ctypes as C
    from regtools_amd import _ffi, cohort
    ph = cohort.pheno_table_from_rank2(c.rank2)
    ph._table.n_rows = 2 ** 31
    out, err = C.POINTER(_ffi.QtlResult)(), C.create_string_buffer(512)
    assert _ffi.lib().rgx_cohort_qtl_nominal_host(ph._h, c.regions.ctypes.data, 0, None, None, None, 0, None, 0, C.byref(out), err, len(err)) == RGX_ERR_ARG
    assert b"2147483648" in err.value and not out
    refused(covariates=np.random.default_rng(1).standard_normal((28, 30)))                              # S < n_cov + 3
    assert _twin(c, covariates=np.random.default_rng(1).standard_normal((27, 30))).dof == 1
    for a, b in ((5, 4), (0, 23)):                                                                       # variants out of order
        for f in ("var_pos", "var_tid"):
            x = getattr(c, f).copy()
            x[[a, b]] = x[[b, a]]
            if not np.array_equal(x, getattr(c, f)):
                refused(**{f: x})
    # a covariate that the intercept and those before it explain
    assert "covariate 2" in str(refused(covariates=np.stack([c.cov[0], c.cov[0] * 2 + 1])))
    assert "covariate 1" in str(refused(covariates=np.full((1, 30), 3.0)))
    assert "covariate 3" in str(refused(covariates=np.stack([c.cov[0], c.cov[1], c.cov[0] - c.cov[1] * (1 + 1e-12)])))
    # met by the twin: a dosage outside the four values, a rank2 outside [2, 2 K], at the first and the last entry
    for at in ((0, 0), (23, 29)):
        for bad in (3, -2, 127, -128):
            d = c.dosage.copy()
            d[at] = bad
            assert "dosage" in str(refused(dosage=d))
    for at in ((0, 0), (19, 29)):
        for bad in (0, 1, 41, 0xffffffff):
            r2 = c.rank2.copy()
            r2[at] = bad
            assert "rank2" in str(refused(rank2=r2))
        for edge in (2, 40):
            r2 = c.rank2.copy()
            r2[at] = edge
            assert _twin(c, rank2=r2).n_rows == 20


def test_more_pairs_than_the_result_can_index():
    """65,537 rows x 65,536 usable variants on one contig under the widest window: 2^32 + 2^16 pairs."""
    from regtools_amd import RegtoolsError
    K, V, S = 65537, 65536, 3
    rng = np.random.default_rng(8)
    rank2 = (2 * (np.argsort(rng.random((K, S)), axis=0) + 1)).astype(np.uint32)
    regions = np.tile(np.array([[0, 5, 9]], np.uint32), (K, 1))
    dosage = np.tile(np.array([[0, 1, 2]], np.int8), (V, 1))
    c = qc.Case(rank2=rank2, regions=regions, var_tid=np.zeros(V, np.uint32), var_pos=np.arange(1, V + 1, dtype=np.uint32), dosage=dosage,
                cov=np.zeros((0, S)), window=0xffffffff)
    with pytest.raises(RegtoolsError) as e:
        _twin(c)
    assert e.value.code == RGX_ERR_ARG and "4295032832 pairs" in str(e.value)
