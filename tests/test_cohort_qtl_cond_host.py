"""The conditional permutation pass without a device: the contract of rgx_cohort_qtl_permute_conditional in include/regtools_amd.h as
rgx_cohort_qtl_permute_conditional_host (the library's plain C++ twin) keeps it.  Expectations: the restatement of tests/qtl_cond_ref.py -- every
array as bit patterns against exact fused multiply-adds in the contract's order --, ordinary least squares of the FULL model y ~ 1 + covariates +
conditioning variants + g, and the unconditional permutation pass where the two must meet.

The tolerance of the least-squares check is qtl_ref's form with the constant measured between two references (numpy lstsq against a QR
residualisation of the same full model; qtl_cond_ref.C_MEASURED), four times over; the measurement is repeated below."""
import numpy as np
import pytest

import qtl_cases as qc
import qtl_cond_cases as cc
import qtl_cond_ref as cref
import qtl_perm_cases as pcs
import qtl_perm_ref as pref
import qtl_ref as ref

RGX_ERR_ARG = 7
B_SMALL, S_SEED = 3, 11


def _twin(c, series, **kw):
    from regtools_amd import cohort
    a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window, rank2=c.rank2,
             n_perm=B_SMALL, seed=S_SEED)
    a.update(kw)
    rows, begin, var = cohort.qtl_series(series)
    return cohort.qtl_permute_conditional_host(cohort.pheno_table_from_rank2(a.pop("rank2")), a.pop("regions"), rows, begin, var, **a)


def _cis(c, **kw):
    from regtools_amd import cohort
    return cc.cis_lists(c, cohort, **kw)


@pytest.mark.parametrize("S, K, V, n_cov", qc.PLANTED)
def test_the_twin_is_the_restatement(S, K, V, n_cov):
    """Every array of the result, m = 1, 2, 3, on the planted cases: bases, rows, beta, gg', alpha and the conditioned chains in exact rationals."""
    from regtools_amd import cohort
    c = qc.case(S, K, V, n_cov)
    series = cc.draw(_cis(c), (1, 2, 3), seed=S, per_size=2)
    assert len(series) >= 5 and set(len(cv) for _, cv in series) == {1, 2, 3}
    q = _twin(c, series)
    want = cref.restate(c, cohort.quantile, pref.permutations(S, B_SMALL, S_SEED), series)
    cref.same_as_restated(q, want)
    assert q.n_pairs > 0 and q.n_tiles == 0 and (q.cond_status == 0).all()
    assert np.array_equal(q.dof, [S - n_cov - 2 - len(cv) for _, cv in series])
    assert np.array_equal(q.p_perm, (q.n_ge + 1.0) / (B_SMALL + 1))


def _best_pairs(c, series, q):
    return [(k, cv, int(q.best_variant[n])) for n, (k, cv) in enumerate(series) if q.n_cis[n]]


def test_least_squares_of_the_full_model():
    """r, slope and t of every series' best pair at b = 0 against numpy.linalg.lstsq of y ~ 1 + cov + x_c1 .. x_cm + g, mean-imputed dosages."""
    from regtools_amd import cohort
    c = cc.lstsq_case()
    series = cc.lstsq_series(_cis(c))
    q = _twin(c, series, n_perm=2)
    rows = np.array(ref.quantile_table(c.K, cohort.quantile))[c.rank2.astype(np.int64) - 2]
    worst, n_checked, strongest = [0.0, 0.0], 0, 0.0
    for n, (k, cv) in enumerate(series):
        if not q.n_cis[n]:
            continue
        v, dof = int(q.best_variant[n]), int(q.dof[n])
        y, g, Z = cref.full_model(c, k, cv, v, rows)
        b, se, t = ref.ols(y, g, Z)
        _, _, _, _, gg = ref.qr_stats(y, g, Z)
        r = float(q.best_r[n])
        u_slope, u_t = cref.bounds(c.S, dof, r, float(q.yy_cond[n]), gg, g)
        mine_t = cohort.qtl_tstat(r, dof)
        worst = [max(worst[0], abs(q.best_slope[n] - b) / u_slope), max(worst[1], abs(mine_t - t) / u_t)]
        assert dof == c.S - Z.shape[1] - 1
        assert abs(q.best_slope[n] - b) <= cref.C_TOL * u_slope and abs(mine_t - t) <= cref.C_TOL * u_t, (n, k, cv, v)
        assert abs(q.best_slope[n] / mine_t - se) <= (cref.C_TOL * (u_slope / abs(b) + u_t / abs(t)) + 8 * ref.EPS) * se
        n_checked += 1
        strongest = max(strongest, abs(mine_t))
    print("%d series: slope off by %.3f, t by %.3f units of S eps scale" % (n_checked, worst[0], worst[1]))
    assert n_checked >= 30 and strongest > 3


def test_the_two_references_agree_within_the_tolerance():
    """The measurement behind C_MEASURED, repeated: lstsq against a QR residualisation of the full model, neither the code under test."""
    from regtools_amd import cohort
    c = cc.lstsq_case()
    series = cc.lstsq_series(_cis(c))
    pairs = _best_pairs(c, series, _twin(c, series, n_perm=2))
    worst = cref.measure_c(c, cohort.quantile, pairs)
    print("lstsq against QR residuals over %d pairs: slope %.4f, t %.4f" % (len(pairs), worst[0], worst[1]))
    assert len(pairs) >= 30 and max(worst) <= cref.C_TOL


def test_a_duplicate_of_a_conditioning_variant_drops_out():
    """The partner with equal dosages takes no part, and n_cis drops accordingly; both in one set are collinear: no pairs, no fit."""
    c = qc.case(64, 16, 20, 1)
    cis = _cis(c)
    k = int(np.argmax([len(x) for x in cis]))
    a, b, other = cis[k][0], cis[k][-1], cis[k][1]
    assert len(cis[k]) >= 4
    before = _twin(c, [(k, [a])])
    d = c.dosage.copy()
    d[b] = d[a]
    q = _twin(c, [(k, [a]), (k, [b]), (k, [a, b]), (k, [other, b, a]), (k, [other])], dosage=d)
    assert before.n_cis[0] == before.n_window[0] - 1
    assert list(q.n_window) == [len(cis[k])] * 5 and list(q.n_cis[:2]) == [len(cis[k]) - 2] * 2 and q.n_cis[4] == len(cis[k]) - 1
    assert list(q.cond_status) == [0, 0, 1, 1, 0] and q.n_collinear == 2
    for n in (2, 3):
        assert q.n_cis[n] == 0 and q.best_variant[n] == cref.NO_PAIR and not q.perm_r[n].any() and q.beta_status[n] == 2
        assert np.isnan(q.p_beta[n]) and q.yy_cond[n] == 0 and q.n_ge[n] == B_SMALL
    # conditioned on either of the two the row and the places are the same numbers
    ref.same_bits(q.perm_r[0], q.perm_r[1])
    ref.same_bits([q.yy_cond[0], q.best_r[0]], [q.yy_cond[1], q.best_r[1]])


def test_eight_variants_and_a_row_in_three_series():
    from regtools_amd import cohort
    c = pcs.rows_with(30, 14, 20, seed=8)
    cis = _cis(c)
    series = [(0, cis[0][:8]), (0, cis[0][3:11][::-1]), (0, cis[0][13:14])]
    q = _twin(c, series)
    assert list(q.dof) == [20, 20, 27] and list(q.n_cis) == [6, 6, 13] and (q.cond_status == 0).all() and q.n_cond == 17
    assert np.array_equal(q.series_row, [0, 0, 0]) and np.array_equal(q.cond_begin, [0, 8, 16, 17])
    want = cref.restate(c, cohort.quantile, pref.permutations(30, B_SMALL, S_SEED), series, only={(0, 0), (1, 2), (2, 3)})
    cref.same_as_restated(q, want, only={(0, 0), (1, 2), (2, 3)})
    # the variance left shrinks with every variant taken out
    assert q.yy_cond[0] < q.yy[0] and q.yy_cond[2] < q.yy[0] and (q.best_variant != cref.NO_PAIR).all()
    assert not set(q.best_variant[:1]) & set(cis[0][:8])


def test_the_order_of_a_set_does_not_change_what_takes_part():
    """Another order is another basis of the same space: the same variants take part and the statistics agree to rounding, not to the bit."""
    c = qc.case(65, 40, 40, 3)
    cis = _cis(c)
    k = int(np.argmax([len(x) for x in cis]))
    q = _twin(c, [(k, cis[k][:3]), (k, cis[k][:3][::-1])], n_perm=9)
    assert q.n_cis[0] == q.n_cis[1] and q.best_variant[0] == q.best_variant[1]
    assert np.allclose(q.perm_r[0], q.perm_r[1], rtol=0, atol=1e-12) and abs(q.yy_cond[0] - q.yy_cond[1]) < 1e-12 * q.yy[k]


def test_errors():
    from regtools_amd import RegtoolsError
    c = qc.case(65, 40, 40, 3)
    cis = _cis(c)
    good = cc.draw(cis, (1, 2), seed=2, per_size=5)
    k = good[-1][0]

    def refused(series, **kw):
        with pytest.raises(RegtoolsError) as e:
            _twin(c, series, **kw)
        assert e.value.code == RGX_ERR_ARG, series
        return str(e.value)
    assert "at least one series" in refused([])
    assert "names row 40" in refused(good + [(40, [cis[k][0]])])
    assert "takes 1 to 8" in refused(good + [(k, [])]) and "takes 1 to 8" in refused([(k, list(range(9)))])
    assert "variant 40 of 40" in refused([(k, [40])])
    assert "twice" in refused([(k, [cis[k][0], cis[k][1], cis[k][0]])])
    far = [v for v in range(c.V) if c.var_tid[v] != c.regions[k, 0]]
    assert "not cis" in refused([(k, [far[0]])])
    usable = set(x for l in cis for x in l)
    near = [(kk, v) for v in range(c.V) if v not in usable for kk in range(c.K) if c.var_tid[v] == c.regions[kk, 0]
            and int(c.regions[kk, 1]) - c.window <= int(c.var_pos[v]) <= int(c.regions[kk, 2]) + c.window]
    assert "variant %d, which series %d is conditioned on, is constant or explained" % (near[0][1], len(good)) in refused(
        good + [(near[0][0], [near[0][1]])])
    # the permutation pass's and the nominal scan's
    assert "1 to 65535" in refused(good, n_perm=0) and "1 to 65535" in refused(good, n_perm=65536)
    perms = pref.permutations(65, 3, 1)
    perms[2, 0] = perms[2, 1]
    assert "row 2" in refused(good, perms=perms)
    refused(good, var_pos=c.var_pos[::-1].copy())
    d = c.dosage.copy()
    d[0, 0] = 3
    assert "dosage" in refused(good, dosage=d)
    r2 = c.rank2.copy()
    r2[0, 0] = 81
    assert "rank2" in refused(good, rank2=r2)
    # S < n_cov + 3 + m
    small = pcs.rows_with(9, 12, 16, seed=99)
    cs = _cis(small)
    assert _twin(small, [(0, cs[0][:6])]).dof[0] == 1
    with pytest.raises(RegtoolsError) as e:
        _twin(small, [(0, cs[0][:7])])
    assert e.value.code == RGX_ERR_ARG and "no degree of freedom" in str(e.value)


def test_too_many_series_for_the_result():
    """N (B + 1) > 2^32 - 2^16 is refused before anything of that size is touched: 65,536 series x 65,536 values."""
    from regtools_amd import RegtoolsError, cohort
    c = qc.case(12, 9, 16, 0)
    cis = _cis(c)
    k = int(np.argmax([len(x) for x in cis]))
    N = 65536
    rows, begin, var = np.full(N, k, np.uint32), np.arange(N + 1, dtype=np.uint32), np.full(N, cis[k][0], np.uint32)
    perms = np.tile(np.arange(12, dtype=np.uint16), (65536, 1))
    with pytest.raises(RegtoolsError) as e:
        cohort.qtl_permute_conditional_host(cohort.pheno_table_from_rank2(c.rank2), c.regions, rows, begin, var, c.var_tid, c.var_pos, c.dosage, c.cov,
                                            c.window, perms=perms)
    assert e.value.code == RGX_ERR_ARG and "2^32 - 2^16" in str(e.value)


# ---- the forward-backward pass -------------------------------------------------------------------------------------------------------------------
def _indep_args(c, **kw):
    P = cc.INDEP
    a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window, n_perm=P["B"],
             seed=P["perm_seed"], p_threshold=P["p_threshold"], max_signals=P["max_signals"])
    a.update(kw)
    return a


def _loop(c, a):
    """The Python forward-backward loop over the two host twins alone."""
    from regtools_amd import cohort
    ph = cohort.pheno_table_from_rank2(c.rank2)
    shared = {x: a[x] for x in a if x not in ("p_threshold", "max_signals", "regions")}
    keep = []

    def perm_pass():
        keep.append(cohort.qtl_permute_host(ph, a["regions"], **shared))
        return keep[-1]

    def cond_pass(series):
        keep.append(cohort.qtl_permute_conditional_host(ph, a["regions"], *cohort.qtl_series(series), **shared))
        return keep[-1]
    return cref.forward_backward(perm_pass, cond_pass, c.S, c.n_cov, a["p_threshold"], a["max_signals"])


def test_the_planted_signals_are_found():
    """Two-signal rows end with exactly their two planted variants at ranks 1 and 2, one-signal rows with exactly theirs, no null row enters, and
    the tag row of seed 9 drops its forward signal 1 -- the tag min(2, A + B) -- going backward: A and B stay with ranks 2 and 3."""
    from regtools_amd import cohort
    c = cc.indep_case()
    q = cohort.qtl_independent_host(cohort.pheno_table_from_rank2(c.rank2), **_indep_args(c))

    def signals(k):
        s = slice(int(q.sig_begin[k]), int(q.sig_begin[k + 1]))
        return [int(v) for v in q.variant[s]], [int(v) for v in q.rank[s]], [int(v) for v in q.n_cond[s]]
    for k, planted in c.two:
        assert (sorted(signals(k)[0]), signals(k)[1], signals(k)[2]) == (planted, [1, 2], [1, 1]), k
    for k, planted in c.one:
        assert signals(k) == (planted, [1], [0]), k
    for k, _ in c.null:
        assert signals(k) == ([], [], []), k
    dropped = [(k, signals(k)) for k, (a, b, t) in c.tag if signals(k)[1] == [2, 3] and sorted(signals(k)[0]) == sorted([a, b])]
    assert len(dropped) == 1 and dropped[0][1][2] == [2, 2]
    assert q.n_entered == len(c.two) + len(c.one) + len(c.tag) and q.n_forward_rounds == 3 and q.n_capped == 0 and not q.capped.any()
    assert (q.dof == c.S - c.n_cov - 2 - q.n_cond).all() and (q.p_beta <= q.p_threshold).all() and q.max_signals == 4


@pytest.mark.parametrize("max_signals, p_threshold", [(4, 0.01), (1, 0.01), (2, 0.5), (8, 1.0)])
def test_the_driver_is_the_loop_over_the_two_twins(max_signals, p_threshold):
    """Integers exactly, doubles as bits.  max_signals 1 caps every row that enters; a threshold of 1 takes every fit and runs into the cap."""
    from regtools_amd import cohort
    c = cc.indep_case(n_two=3, n_one=3, n_null=3, n_tag=2, per_row=10) if max_signals == 8 else cc.indep_case()
    a = _indep_args(c, max_signals=max_signals, p_threshold=p_threshold)
    q = cohort.qtl_independent_host(cohort.pheno_table_from_rank2(c.rank2), **a)
    loop = _loop(c, a)
    cref.same_as_loop(q, loop)
    if max_signals == 1:
        assert q.n_forward_rounds == 0 and q.n_series_total == 0 and q.n_capped == q.n_entered == q.n_signals > 0 and (q.n_cond == 0).all()
    if p_threshold == 1.0:
        assert q.n_capped > 0 and max(len(f) for f in loop[5]) == 8 and q.n_cond.max() == 7
    if max_signals == 2:
        assert q.n_capped > 0 and q.n_forward_rounds == 1


def test_the_arguments_of_the_forward_backward_pass():
    from regtools_amd import RegtoolsError, cohort
    c = cc.indep_case(n_two=2, n_one=2, n_null=2, n_tag=1)
    ph = cohort.pheno_table_from_rank2(c.rank2)
    for kw, word in ((dict(p_threshold=0.0), "(0, 1]"), (dict(p_threshold=1.5), "(0, 1]"), (dict(p_threshold=float("nan")), "(0, 1]"),
                     (dict(max_signals=0), "1 to 8"), (dict(max_signals=9), "1 to 8"), (dict(n_perm=0), "1 to 65535"),
                     (dict(var_pos=c.var_pos[::-1].copy()), "lies in front")):
        with pytest.raises(RegtoolsError) as e:
            cohort.qtl_independent_host(ph, **_indep_args(c, **kw))
        assert e.value.code == RGX_ERR_ARG and word in str(e.value), kw


def test_the_text_of_the_signals():
    import cluster_cases
    import pheno_cases as pc
    from regtools_amd import cohort
    tables = pc.tables(pc.counts(9, 41, seed=9, absent=0.2))
    m = cohort.merge_host([cluster_cases.Sample(t) for t in tables], pc.names(9))
    cl = cohort.cluster_host(m)
    ph = cohort.phenotypes_host(m, cl, max_missing=(1, 1), min_sd=0.0)
    regions = cohort.pheno_regions(m, ph)
    tid, pos, dosage = qc.variants_near(regions, 9, 30, seed=4)
    a = dict(covariates=cohort.pheno_pcs_host(ph, 1).component.copy(), window=qc.WINDOW, n_perm=40, seed=3)
    q = cohort.qtl_independent_host(ph, regions, tid, pos, dosage, p_threshold=0.6, max_signals=3, **a)
    first = cohort.qtl_permute_host(ph, regions, tid, pos, dosage, **a)
    ids = [b"v%d" % i if i % 3 else b"%s:%d:A:T" % (m.ref_name[tid[i]].encode(), pos[i]) for i in range(30)]
    pheno_ids = [line.split(b"\t")[3].decode() for line in ph.text(m, cl).split(b"\n")[1:-1]]
    text = q.text(m, cl, ph, pos, ids)
    assert text == cref.indep_text(pheno_ids, [i.decode() for i in ids], pos, regions[:, 1], q, cohort.qtl_tstat, cohort.qtl_pvalue)
    n_per_row = np.diff(q.sig_begin.astype(np.int64))
    assert text.count(b"\n") == q.n_signals + 1 and (n_per_row == 1).any() and (n_per_row >= 2).any()
    # every line of a row with one signal is the permutation pass's line of that row and "\t1\t0"
    perm_lines = dict((l.split(b"\t")[0], l) for l in first.text(m, cl, ph, pos, ids).split(b"\n")[1:-1])
    lines = text.split(b"\n")[1:-1]
    singles = [l for l in lines if l.endswith(b"\t1\t0")]
    assert len(singles) == int((n_per_row == 1).sum()) and all(l == perm_lines[l.split(b"\t")[0]] + b"\t1\t0" for l in singles)
    head = text.split(b"\n")[0]
    assert head == first.text(m, cl, ph, pos, ids).split(b"\n")[0] + b"\trank\tn_cond"
    import ctypes as C
    from regtools_amd import _ffi
    fn = _ffi.lib().rgx_cohort_format_qtl_indep
    n = fn(m._h, cl._h, ph._h, None, None, None, None, 0)
    buf = C.create_string_buffer(n + 1)
    assert fn(m._h, cl._h, ph._h, None, None, None, buf, n) == n and buf.raw[:n] == head + b"\n"
    cluster_cases.free_tables(tables)


def test_the_tool_refuses_bad_thresholds():
    """-I without -g and thresholds that do not parse end with status 1 before any file is read or any device touched."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "regtools-amd")

    def run(*args):
        return subprocess.run([exe, "junctions", "cohort", "-s", "XS"] + list(args) + ["none.bam"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    r = run("-I", "none.indep")
    assert r.returncode == 1 and b"Please supply the genotypes with '-g' option!" in r.stderr
    for bad in ("0", "-0.1", "1.5", "nan", "p", "", "0.05x"):
        r = run("-g", "none.vcf", "-I", "none.indep", "-F", bad)
        assert r.returncode == 1 and b"Unrecognized threshold argument!" in r.stderr, bad
    assert b"-I FILE" in run("-h").stdout and b"-F FLOAT" in run("-h").stdout
    assert not os.path.exists("none.indep")
