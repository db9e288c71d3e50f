"""The contract of rgx_cohort_qtl_nominal (include/regtools_amd.h) restated in scalar Python, and the independent references of the sQTL scan tests
(tests/test_cohort_qtl_host.py, tests/test_gpu_cohort_qtl.py).
  restate()       every fused multiply-add as an exact rational (fractions.Fraction) rounded once; plain Python floats, which round every operation
                  on its own, for the rest.  Results are compared with the library's as bit patterns.
  ols()           ordinary least squares of the FULL model y ~ 1 + covariates + g by numpy.linalg.lstsq: coefficient, standard error and t of g
  qr_stats()      the same numbers from a numpy QR residualisation and a correlation -- the second reference, for the tolerance alone
  t_sf_p()        2 * scipy.stats.t.sf(|t|, dof)
"""
import math
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52
NO_PAIR = 0xffffffff

# The tolerance of slope and t against ols(): |slope - slope_ols| <= C * S * EPS * sqrt(yy / gg) * amp and |t - t_ols| <= C * S * EPS * sqrt(dof) /
# (1 - r^2)^1.5 * amp, with amp = |g| / sqrt(gg) (how much of the imputed genotype the covariates take away: the conditioning of the full model) --
# the error of r carried through slope = r sqrt(yy / gg) and t = r sqrt(dof / (1 - r^2)).  C_MEASURED is the largest ratio between TWO references,
# neither the code under test: ols() against qr_stats() over every pair of qtl_cases.PLANTED (measure_c() below; 311 pairs): 0.2593 in the slope,
# 0.2571 in t.  C_TOL is four times the larger, the project's usual margin for another machine's libm.
C_MEASURED, C_TOL = 0.2593, 4 * 0.2593

# The tolerance of rgx_qtl_pvalue against t_sf_p(), relative: four times the largest relative difference between 2 * scipy.stats.t.sf(|t|, dof)
# and scipy.special.betainc(dof / 2, 1 / 2, dof / (dof + t^2)) over P_DOFS x P_TS (measure_p() below), which was 7.29e-14, at dof 997 and |t| = 30.
# No |t| between 0 and 0.5: there dof / (dof + t^2) rounds to a neighbour of 1 and betainc's argument, not either function, sets the difference
# (8e-9 at |t| = 1e-8, 1.6e-13 at dof 997 and |t| = 0.1).
P_DOFS = (1, 2, 10, 997)
P_TS = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.5, 6.0, 8.0, 12.0, 20.0, 30.0, 40.0)
P_MEASURED, P_TOL = 7.29e-14, 4 * 7.29e-14


def fma(a, b, c):
    """fma(a, b, c) of three finite doubles: the exact a * b + c rounded once, with IEEE 754's sign of an exact zero (round to nearest)."""
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact:
        return float(exact)
    prod_neg = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, b) < 0)
    return -0.0 if prod_neg and math.copysign(1.0, c) < 0 else 0.0


def dot64(a, b):
    P = [0.0] * 64
    for s in range(len(a)):
        P[s % 64] = fma(a[s], b[s], P[s % 64])
    off = 32
    while off:
        for l in range(off):
            P[l] = P[l] + P[l + off]
        off //= 2
    return P[0]


def basis(S, cov):
    """The C = n_cov + 1 unit vectors (lists of floats), or None when a covariate is refused."""
    Q = []
    for j in range(len(cov) + 1):
        b = [1.0] * S if j == 0 else [float(x) for x in cov[j - 1]]
        v = list(b)
        for _ in range(2):
            for q in Q:
                d = 0.0
                for s in range(S):
                    d += v[s] * q[s]
                for s in range(S):
                    v[s] = v[s] - d * q[s]
        n2 = b2 = 0.0
        for s in range(S):
            n2 += v[s] * v[s]
            b2 += b[s] * b[s]
        norm = math.sqrt(n2)
        if not norm > 1e-10 * math.sqrt(b2):
            return None
        Q.append([x / norm for x in v])
    return Q


def residual(x, Q):
    x = list(x)
    for q in Q:
        d = dot64(x, q)
        for s in range(len(x)):
            x[s] = fma(-d, q[s], x[s])
    return x, dot64(x, x)


def quantile_table(K, quantile):
    """T[r - 2] for r = 2 .. 2 K, by the library's host function `quantile`."""
    return [quantile(r, K) for r in range(2, 2 * K + 1)]


class Restated(object):
    pass


def cis_range(keys, region, window):
    """[lo, hi) among the ascending (tid, pos) keys of the usable variants."""
    tid, start, end = (int(x) for x in region)
    first, last = (tid, start - min(start, window)), (tid, min(end + window, 2 ** 32 - 1))
    lo = sum(1 for k in keys if k < first)
    hi = sum(1 for k in keys if k <= last)
    return lo, max(lo, hi)


def restate(c, quantile, pairs=None):
    """The whole contract for case c.  pairs: None for every pair, else a set of (k, v) whose r and slope are wanted (the others stay NaN)."""
    K, S, V = c.K, c.S, c.V
    T = quantile_table(K, quantile)
    Q = basis(S, c.cov)
    assert Q is not None
    o = Restated()
    o.yy, o.gg, o.variant_verdict = np.zeros(K), np.zeros(V), np.zeros(V, np.uint8)
    Y, G = [None] * K, [None] * V
    for k in range(K):
        Y[k], o.yy[k] = residual([T[int(r) - 2] for r in c.rank2[k]], Q)
    for v in range(V):
        d = [int(x) for x in c.dosage[v]]
        present = [x for x in d if x >= 0]
        if not present or min(present) == max(present):
            o.variant_verdict[v] = 1
            continue
        mean = float(sum(present)) / float(len(present))
        G[v], o.gg[v] = residual([float(x) if x >= 0 else mean for x in d], Q)
        o.variant_verdict[v] = 0 if o.gg[v] > 1e-12 * S else 2
    usable = [v for v in range(V) if o.variant_verdict[v] == 0]
    keys = [(int(c.var_tid[v]), int(c.var_pos[v])) for v in usable]
    begin, variant, r, slope, best = [0], [], [], [], []
    for k in range(K):
        lo, hi = cis_range(keys, c.regions[k], c.window) if o.yy[k] > 1e-12 * S else (0, 0)
        at, top = NO_PAIR, -1.0
        for u in range(lo, hi):
            v = usable[u]
            variant.append(v)
            if pairs is not None and (k, v) not in pairs:
                r.append(float("nan")); slope.append(float("nan"))
                continue
            acc = 0.0
            for s in range(S):
                acc = fma(Y[k][s], G[v][s], acc)
            r.append(acc / math.sqrt(o.yy[k] * o.gg[v])); slope.append(acc / o.gg[v])
            if abs(r[-1]) > top:
                at, top = len(r) - 1, abs(r[-1])
        begin.append(len(variant)); best.append(at)
    o.pair_begin, o.pair_variant = np.array(begin, np.uint32), np.array(variant, np.uint32)
    o.r, o.slope, o.best = np.array(r, np.float64), np.array(slope, np.float64), np.array(best, np.uint32)
    o.n_pairs = len(variant)
    return o


def restate_pair(c, quantile, k, v, Q=None):
    """(yy, gg, r, slope) of row k and usable variant v alone, for tables too large for restate()."""
    Q = basis(c.S, c.cov) if Q is None else Q
    T = quantile_table(c.K, quantile) if not hasattr(c, "_T") else c._T
    y, yy = residual([T[int(r) - 2] for r in c.rank2[k]], Q)
    d = [int(x) for x in c.dosage[v]]
    present = [x for x in d if x >= 0]
    mean = float(sum(present)) / float(len(present))
    g, gg = residual([float(x) if x >= 0 else mean for x in d], Q)
    acc = 0.0
    for s in range(c.S):
        acc = fma(y[s], g[s], acc)
    return yy, gg, acc / math.sqrt(yy * gg), acc / gg


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_result(a, b, floats=True):
    """Every array of two results: the integers exactly, the doubles as bit patterns."""
    assert a.n_pairs == b.n_pairs
    for f in ("variant_verdict", "pair_begin", "pair_variant", "best"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    if floats:
        for f in ("yy", "gg", "r", "slope"):
            same_bits(getattr(a, f), getattr(b, f))


# ---- the independent references -----------------------------------------------------------------------------------------------------------------
def model(c, k, v, quantile_rows):
    """y, the imputed g and the design [1, covariates] of pair (k, v); quantile_rows: K x S quantiles."""
    y = np.asarray(quantile_rows[k], np.float64)
    d = c.dosage[v].astype(np.float64)
    g = np.where(d >= 0, d, d[d >= 0].mean())
    Z = np.vstack([np.ones(c.S), c.cov.reshape(-1, c.S)]).T
    return y, g, Z


def ols(y, g, Z):
    """lstsq of y ~ Z + g: (coefficient of g, its standard error, t)."""
    X = np.column_stack([Z, g])
    beta = np.linalg.lstsq(X, y, rcond=None)[0]
    res = y - X @ beta
    dof = len(y) - X.shape[1]
    se = math.sqrt(float(res @ res) / dof * np.linalg.inv(X.T @ X)[-1, -1])
    return beta[-1], se, beta[-1] / se


def qr_stats(y, g, Z):
    """(slope, t, r, yy, gg) from residuals against a QR basis of Z."""
    Qz = np.linalg.qr(Z)[0]
    yr, gr = y - Qz @ (Qz.T @ y), g - Qz @ (Qz.T @ g)
    yy, gg, dot = float(yr @ yr), float(gr @ gr), float(yr @ gr)
    r = dot / math.sqrt(yy * gg)
    dof = len(y) - Z.shape[1] - 1
    return dot / gg, r * math.sqrt(dof / (1 - r * r)), r, yy, gg


def bounds(c, r, yy, gg, g):
    """(the slope's, t's) bound per unit of C."""
    amp = math.sqrt(float(g @ g) / gg)
    return c.S * EPS * math.sqrt(yy / gg) * amp, c.S * EPS * math.sqrt(c.dof) / (1 - r * r) ** 1.5 * amp


def t_sf_p(t, dof):
    from scipy.stats import t as student
    return 2 * student.sf(abs(t), dof)


def measure_c(quantile, cases):
    """The largest ratios (slope, t) of |ols - qr_stats| to the bounds' units over every pair of the cases, and the number of pairs."""
    worst, n = [0.0, 0.0], 0
    for c in cases:
        rows = np.array(quantile_table(c.K, quantile))[c.rank2.astype(np.int64) - 2]
        q = restate(c, quantile, pairs=set())
        for k in range(c.K):
            for p in range(q.pair_begin[k], q.pair_begin[k + 1]):
                y, g, Z = model(c, k, int(q.pair_variant[p]), rows)
                b, _, t = ols(y, g, Z)
                slope, t2, r, yy, gg = qr_stats(y, g, Z)
                u = bounds(c, r, yy, gg, g)
                worst = [max(worst[0], abs(b - slope) / u[0]), max(worst[1], abs(t - t2) / u[1])]
                n += 1
    return worst, n


def measure_p():
    """The largest relative difference between 2 * t.sf and betainc over the points with t > 0."""
    from scipy.special import betainc
    worst = 0.0
    for dof in P_DOFS:
        for t in P_TS[1:]:
            a, b = t_sf_p(t, dof), betainc(dof / 2.0, 0.5, dof / (dof + t * t))
            worst = max(worst, abs(a - b) / a)
    return worst


def text(ids, variant_ids, var_pos, starts, q, tstat, pvalue):
    """The Python writer of rgx_cohort_format_qtl: ids[k] the phenotype IDs, starts[k] the rows' starts; tstat and pvalue the library's host
    functions."""
    out = ["phenotype_id\tvariant_id\tdistance\tr\tslope\tslope_se\ttstat\tpval_nominal\tis_best\n"]
    for k in range(len(ids) if q is not None else 0):
        for p in range(int(q.pair_begin[k]), int(q.pair_begin[k + 1])):
            v = int(q.pair_variant[p])
            t = tstat(float(q.r[p]), q.dof)
            se = float(q.slope[p]) / t if not math.isinf(t) else math.copysign(0.0, float(q.slope[p]) * t)
            out.append("%s\t%s\t%d\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\t%d\n" % (ids[k], variant_ids[v], int(var_pos[v]) - int(starts[k]), q.r[p],
                                                                                  q.slope[p], se, t, pvalue(t, q.dof), 1 if int(q.best[k]) == p else 0))
    return "".join(out).encode()
