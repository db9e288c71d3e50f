"""The contract of rgx_cohort_qtl_permute_conditional (include/regtools_amd.h) restated in scalar Python, and the independent references of the
conditional pass tests (tests/test_cohort_qtl_cond_host.py, tests/test_gpu_cohort_qtl_cond.py).  Steps (1)-(6) are tests/qtl_ref.py's.
  restate()       the bases, the rows, beta, gg', alpha and every conditioned chain with qtl_ref's exact rational fma and dot64, the max on bit patterns
  full_model(), ols(), qr_stats(), measure_c()   least squares of y ~ 1 + cov + conditioning variants + g by numpy.linalg.lstsq, the same numbers from
                  a QR residualisation, and the largest ratio between the two in units of the bound
  same_cond_result()   two results of the library, every array
"""
import math
import struct

import numpy as np

import qtl_perm_ref as pref
import qtl_ref as ref

NO_PAIR = ref.NO_PAIR
MAX_COND = 8

# The tolerance of slope and t against ols(): qtl_ref's form, |slope - slope_ols| <= C * S * EPS * sqrt(yy' / gg') * amp and |t - t_ols| <= C * S *
# EPS * sqrt(dof) / (1 - r^2)^1.5 * amp with amp = |g| / sqrt(gg'), g the imputed genotype and gg' what the intercept, the covariates AND the
# conditioning variants leave of it.  C_MEASURED is the largest ratio between TWO references, neither the code under test: ols() against
# qr_stats() over the best pair of every series of qtl_cond_cases.lstsq_series() (measure_c() below; 37 pairs): 0.0469 in the slope, 0.0344 in t.
# C_TOL is four times the larger, the project's usual margin for another machine's libm.
C_MEASURED, C_TOL = 0.0469, 4 * 0.0469


class Restated(object):
    pass


def _variant(c, v, Q):
    d = [int(x) for x in c.dosage[v]]
    present = [x for x in d if x >= 0]
    if not present or min(present) == max(present):
        return None, 0.0, 1
    mean = float(sum(present)) / float(len(present))
    g, gg = ref.residual([float(x) if x >= 0 else mean for x in d], Q)
    return g, gg, (0 if gg > 1e-12 * c.S else 2)


def restate(c, quantile, perms, series, only=None, verdict=None):
    """The whole contract for case c, the (B + 1) x S permutations and the series [(row, [variants])].  only: None for every (series, b), else a
    set of (series, b) whose perm_r is wanted (the others stay NaN; n_ge is then not computed, the best pair only where (series, 0) is wanted).
    verdict: None, or the variants' verdicts from a result checked otherwise, for tables too large to residualise every variant in rationals."""
    K, S, V = c.K, c.S, c.V
    B = len(perms) - 1
    T = ref.quantile_table(K, quantile)
    Q = ref.basis(S, c.cov)
    assert Q is not None
    G = {}

    def variant(v):
        if v not in G:
            G[v] = _variant(c, v, Q)
        return G[v]
    if verdict is None:
        verdict = [variant(v)[2] for v in range(V)]
    usable = [v for v in range(V) if verdict[v] == 0]
    keys = [(int(c.var_tid[v]), int(c.var_pos[v])) for v in usable]
    N = len(series)
    o = Restated()
    o.cond_status, o.yy_cond = np.zeros(N, np.uint8), np.zeros(N)
    o.n_window, o.n_cis = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
    o.perm_r = np.full((N, B + 1), np.nan if only is not None else 0.0)
    o.best_variant, o.best_r, o.best_slope = np.full(N, NO_PAIR, np.uint32), np.zeros(N), np.zeros(N)
    o.n_ge = np.zeros(N, np.uint32)
    o.dof = np.array([S - c.n_cov - 2 - len(cv) for _, cv in series], np.uint32)
    rows = {}
    for n, (k, cv) in enumerate(series):
        if only is not None and not any(s == n for s, _ in only):
            continue
        if k not in rows:
            rows[k] = ref.residual([T[int(r) - 2] for r in c.rank2[k]], Q)
        Yk, yy = rows[k]
        lo, hi = ref.cis_range(keys, c.regions[k], c.window) if yy > 1e-12 * S else (0, 0)
        o.n_window[n] = hi - lo
        if only is not None:
            o.perm_r[n, [b for s, b in only if s == n]] = 0.0
        z = []
        for v in cv:
            assert verdict[v] == 0
            x = list(variant(v)[0])
            for _ in range(2):
                for zi in z:
                    d = ref.dot64(x, zi)
                    x = [ref.fma(-d, zi[s], x[s]) for s in range(S)]
            nn = ref.dot64(x, x)
            if not nn > 1e-12 * S:
                o.cond_status[n] = 1
                break
            root = math.sqrt(nn)
            z.append([a / root for a in x])
        if o.cond_status[n]:
            continue
        y = list(Yk)
        for zj in z:
            d = ref.dot64(y, zj)
            y = [ref.fma(-d, zj[s], y[s]) for s in range(S)]
        y2 = o.yy_cond[n] = ref.dot64(y, y)
        if not y2 > 1e-12 * S:
            o.cond_status[n] = 2
            continue
        part = []
        for u in range(lo, hi):
            v = usable[u]
            x, beta = list(variant(v)[0]), []
            for zj in z:
                d = ref.dot64(x, zj)
                beta.append(d)
                x = [ref.fma(-d, zj[s], x[s]) for s in range(S)]
            g2 = ref.dot64(x, x)
            if g2 > 1e-12 * S:
                part.append((v, beta, g2))
        o.n_cis[n] = len(part)
        for b in range(B + 1):
            if (only is not None and (n, b) not in only) or not part:
                continue
            p = [int(x) for x in perms[b]]
            yp = [y[p[s]] for s in range(S)]
            alpha = []
            for zj in z:
                acc = 0.0
                for s in range(S):
                    acc = ref.fma(yp[s], zj[s], acc)
                alpha.append(acc)
            top, at = 0, None
            for v, beta, g2 in part:
                g = variant(v)[0]
                dot = 0.0
                for s in range(S):
                    dot = ref.fma(yp[s], g[s], dot)
                for a, bt in zip(alpha, beta):
                    dot = ref.fma(-a, bt, dot)
                r = dot / math.sqrt(y2 * g2)
                if at is None or pref.bits(r) > top:
                    top, at = pref.bits(r), (v, r, dot / g2)
            o.perm_r[n, b] = struct.unpack("<d", struct.pack("<Q", top))[0]
            if b == 0:
                o.best_variant[n], o.best_r[n], o.best_slope[n] = at
        if only is None:
            o.n_ge[n] = sum(1 for b in range(1, B + 1) if pref.bits(o.perm_r[n, b]) >= pref.bits(o.perm_r[n, 0]))
    o.n_pairs = int(o.n_cis.sum())
    return o


INTS = ("variant_verdict", "series_row", "cond_begin", "cond_variant", "cond_status", "dof", "n_window", "n_cis", "best_variant", "n_ge", "beta_status")
DOUBLES = ("yy", "gg", "yy_cond", "perm_r", "best_r", "best_slope", "p_perm", "beta_shape1", "beta_shape2", "p_beta")


def same_cond_result(a, b):
    """Every array of two results (library against library): the integers exactly, the doubles as bit patterns, NaN included."""
    assert (a.n_rows, a.n_samples, a.n_variants, a.n_cov) == (b.n_rows, b.n_samples, b.n_variants, b.n_cov)
    assert (a.n_pairs, a.n_perm, a.n_series, a.n_cond) == (b.n_pairs, b.n_perm, b.n_series, b.n_cond)
    assert (a.n_constant, a.n_explained, a.n_flat_rows, a.n_collinear, a.n_flat_series) == (
        b.n_constant, b.n_explained, b.n_flat_rows, b.n_collinear, b.n_flat_series)
    for f in INTS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for f in DOUBLES:
        ref.same_bits(getattr(a, f), getattr(b, f))


def same_as_restated(q, want, only=None):
    """A library result against restate()'s: what the restatement computed, as bit patterns."""
    for f in ("cond_status", "n_window", "n_cis", "dof"):
        got, exp = getattr(q, f), getattr(want, f)
        idx = sorted(set(n for n, _ in only)) if only is not None else slice(None)
        assert np.array_equal(got[idx], exp[idx]), f
    if only is None:
        for f in ("best_variant", "n_ge"):
            assert np.array_equal(getattr(q, f), getattr(want, f)), f
        for f in ("yy_cond", "perm_r", "best_r", "best_slope"):
            ref.same_bits(getattr(q, f), getattr(want, f))
    else:
        for n, b in only:
            ref.same_bits([q.perm_r[n, b], q.yy_cond[n]], [want.perm_r[n, b], want.yy_cond[n]])
            if b == 0:
                assert q.best_variant[n] == want.best_variant[n]
                ref.same_bits([q.best_r[n], q.best_slope[n]], [want.best_r[n], want.best_slope[n]])


# ---- the independent references -----------------------------------------------------------------------------------------------------------------
def imputed(c, v):
    d = c.dosage[v].astype(np.float64)
    return np.where(d >= 0, d, d[d >= 0].mean())


def full_model(c, k, cv, v, quantile_rows):
    """y, the imputed g and the design [1, covariates, conditioning variants] of row k, the set cv and variant v."""
    y = np.asarray(quantile_rows[k], np.float64)
    Z = np.vstack([np.ones(c.S), c.cov.reshape(-1, c.S)] + [imputed(c, x) for x in cv]).T
    return y, imputed(c, v), Z


def bounds(S, dof, r, yy, gg, g):
    """(the slope's, t's) bound per unit of C."""
    amp = math.sqrt(float(g @ g) / gg)
    return S * ref.EPS * math.sqrt(yy / gg) * amp, S * ref.EPS * math.sqrt(dof) / (1 - r * r) ** 1.5 * amp


def measure_c(c, quantile, pairs):
    """The largest ratios (slope, t) of |ols - qr_stats| to the bounds' units over pairs = [(row, [conditioning variants], variant)]."""
    rows = np.array(ref.quantile_table(c.K, quantile))[c.rank2.astype(np.int64) - 2]
    worst = [0.0, 0.0]
    for k, cv, v in pairs:
        y, g, Z = full_model(c, k, cv, v, rows)
        b, _, t = ref.ols(y, g, Z)
        slope, t2, r, yy, gg = ref.qr_stats(y, g, Z)
        u = bounds(c.S, c.S - Z.shape[1] - 1, r, yy, gg, g)
        worst = [max(worst[0], abs(b - slope) / u[0]), max(worst[1], abs(t - t2) / u[1])]
    return worst


# ---- the forward-backward pass -------------------------------------------------------------------------------------------------------------------
SIGNAL_INTS = ("variant", "rank", "n_cond", "dof", "n_cis", "beta_status")
SIGNAL_DOUBLES = ("r", "slope", "p_perm", "beta_shape1", "beta_shape2", "p_beta")


def forward_backward(perm_pass, cond_pass, S, n_cov, p_threshold, max_signals):
    """The contract of rgx_cohort_qtl_independent as a Python loop over two callables: perm_pass() -> the permutation pass's result, cond_pass([(row,
    [variants])]) -> the conditional pass's.  Returns (per row its kept signals as dicts, capped, n_entered, n_forward_rounds, n_series_total)."""
    def ok(q, i):
        return bool(q.n_cis[i]) and q.beta_status[i] != 2 and q.p_beta[i] <= p_threshold

    def record(q, i, rank, n_cond, dof):
        return dict(variant=int(q.best_variant[i]), rank=rank, n_cond=n_cond, dof=int(dof), n_cis=int(q.n_cis[i]), r=float(q.best_r[i]),
                    slope=float(q.best_slope[i]), p_perm=float(q.p_perm[i]), beta_shape1=float(q.beta_shape1[i]),
                    beta_shape2=float(q.beta_shape2[i]), p_beta=float(q.p_beta[i]), beta_status=int(q.beta_status[i]))
    q0 = perm_pass()
    K = q0.n_rows
    fwd, capped, active = [[] for _ in range(K)], [0] * K, set()

    def settle(k):
        if len(fwd[k]) < max_signals and len(fwd[k]) <= S - n_cov - 3:
            active.add(k)
        else:
            active.discard(k)
            capped[k] = 1
    for k in range(K):
        if ok(q0, k):
            fwd[k].append(int(q0.best_variant[k]))
            settle(k)
    n_entered, rounds, total = sum(1 for f in fwd if f), 0, 0
    while active:
        series = [(k, list(fwd[k])) for k in sorted(active)]
        q = cond_pass(series)
        rounds, total = rounds + 1, total + len(series)
        for c, (k, _) in enumerate(series):
            if ok(q, c):
                fwd[k].append(int(q.best_variant[c]))
                settle(k)
            else:
                active.discard(k)
    kept = [[record(q0, k, 1, 0, q0.dof)] if len(fwd[k]) == 1 else [] for k in range(K)]
    series = [(k, fwd[k][:i] + fwd[k][i + 1:], i) for k in range(K) if len(fwd[k]) >= 2 for i in range(len(fwd[k]))]
    if series:
        q = cond_pass([(k, cv) for k, cv, _ in series])
        total += len(series)
        for c, (k, cv, i) in enumerate(series):
            if ok(q, c) and int(q.best_variant[c]) not in [s["variant"] for s in kept[k]]:
                kept[k].append(record(q, c, i + 1, len(cv), q.dof[c]))
    return kept, capped, n_entered, rounds, total, fwd


def same_as_loop(q, loop):
    kept, capped, n_entered, rounds, total, _ = loop
    assert (q.n_entered, q.n_forward_rounds, q.n_series_total, q.n_capped) == (n_entered, rounds, total, sum(capped))
    assert list(q.capped) == capped and list(np.diff(q.sig_begin.astype(np.int64))) == [len(x) for x in kept] and q.sig_begin[0] == 0
    flat = [s for row in kept for s in row]
    assert q.n_signals == len(flat)
    for f in SIGNAL_INTS:
        assert [int(x) for x in getattr(q, f)] == [s[f] for s in flat], f
    for f in SIGNAL_DOUBLES:
        ref.same_bits(getattr(q, f), [s[f] for s in flat])


def same_indep_result(a, b):
    assert (a.n_rows, a.n_signals, a.n_entered, a.n_forward_rounds, a.n_series_total, a.n_capped, a.max_signals, a.p_threshold) == (
        b.n_rows, b.n_signals, b.n_entered, b.n_forward_rounds, b.n_series_total, b.n_capped, b.max_signals, b.p_threshold)
    for f in ("sig_begin", "capped") + SIGNAL_INTS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for f in SIGNAL_DOUBLES:
        ref.same_bits(getattr(a, f), getattr(b, f))


def indep_text(ids, variant_ids, var_pos, starts, q, tstat, pvalue):
    """The Python writer of rgx_cohort_format_qtl_indep."""
    out = ["phenotype_id\tnum_var\tbeta_shape1\tbeta_shape2\tdof\tvariant_id\tdistance\tr\tslope\tslope_se\ttstat\tpval_nominal\tpval_perm\tpval_beta"
           "\trank\tn_cond\n"]
    g17 = pref.g17
    for k in range(len(ids) if q is not None else 0):
        for s in range(int(q.sig_begin[k]), int(q.sig_begin[k + 1])):
            v, dof = int(q.variant[s]), int(q.dof[s])
            r, slope = float(q.r[s]), float(q.slope[s])
            t = tstat(r, dof)
            se = slope / t if not math.isinf(t) else math.copysign(0.0, slope * t)
            out.append("\t".join([ids[k], "%d" % q.n_cis[s], g17(q.beta_shape1[s]), g17(q.beta_shape2[s]), "%d" % dof, variant_ids[v],
                                  "%d" % (int(var_pos[v]) - int(starts[k])), g17(r), g17(slope), g17(se), g17(t), g17(pvalue(t, dof)),
                                  g17(q.p_perm[s]), g17(q.p_beta[s]), "%d" % q.rank[s], "%d" % q.n_cond[s]]) + "\n")
    return "".join(out).encode()
