"""The contract of rgx_cohort_qtl_permute (include/regtools_amd.h) restated in scalar Python, and the independent references of the permutation
pass tests (tests/test_cohort_qtl_perm_host.py, tests/test_gpu_cohort_qtl_perm.py).  Steps (1)-(6) are tests/qtl_ref.py's.
  permutations()  the splitmix64 stream and the Fisher-Yates shuffles in Python integers
  restate()       every permuted chain with qtl_ref's exact rational fma, the max on bit patterns, n_ge, the best pair of the identity
  PSI_X, BETA_AB, BETA_X, measure_special()   the points of the digamma, trigamma and incomplete beta checks, and a function's error against mpmath there
  fit_reference(), fit_mpmath()         scipy.stats.beta.fit and mpmath.findroot on the digamma equations
  text()          the Python writer of rgx_cohort_format_qtl_perm
"""
import math
import struct

import numpy as np

import qtl_ref as ref

MASK = (1 << 64) - 1
NO_PAIR = ref.NO_PAIR
DBL_MIN = 2.0 ** -1022
P_MAX = 1.0 - 2.0 ** -53


def splitmix64(seed):
    z = seed & MASK
    while True:
        z = (z + 0x9E3779B97F4A7C15) & MASK
        x = z
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
        yield x ^ (x >> 31)


def permutations(S, B, seed):
    """(B + 1) x S uint16: row 0 the identity, rows 1 .. B drawn in order from one stream."""
    nxt = splitmix64(seed)
    out = [list(range(S))]
    for _ in range(B):
        p = list(range(S))
        for i in range(S - 1, 0, -1):
            j = (next(nxt) * (i + 1)) >> 64
            p[i], p[j] = p[j], p[i]
        out.append(p)
    return np.array(out, np.uint16)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0] & 0x7fffffffffffffff


class Restated(object):
    pass


def restate(c, quantile, perms, only=None, verdict=None):
    """The whole contract for case c and the (B + 1) x S permutations.  only: None for every (k, b), else a set of (k, b) whose perm_r is wanted
    (the others stay NaN; best_* and n_ge are then not computed).  verdict: None, or the variants' verdicts from a result that was checked
    otherwise -- for tables too large to residualise every variant in rationals: only the variants of the wanted rows are then restated."""
    K, S, V = c.K, c.S, c.V
    B = len(perms) - 1
    T = ref.quantile_table(K, quantile)
    Q = ref.basis(S, c.cov)
    assert Q is not None
    o = Restated()
    o.yy, o.gg = np.zeros(K), np.zeros(V)
    o.variant_verdict = np.zeros(V, np.uint8) if verdict is None else np.array(verdict, np.uint8)
    rows = range(K) if only is None else sorted(set(k for k, _ in only))
    Y, G = {}, [None] * V
    for k in range(K):
        if only is None or k in rows:
            Y[k], o.yy[k] = ref.residual([T[int(r) - 2] for r in c.rank2[k]], Q)

    def variant(v):
        d = [int(x) for x in c.dosage[v]]
        present = [x for x in d if x >= 0]
        if not present or min(present) == max(present):
            return 1
        mean = float(sum(present)) / float(len(present))
        G[v], o.gg[v] = ref.residual([float(x) if x >= 0 else mean for x in d], Q)
        return 0 if o.gg[v] > 1e-12 * S else 2
    if verdict is None:
        for v in range(V):
            o.variant_verdict[v] = variant(v)
    usable = [v for v in range(V) if o.variant_verdict[v] == 0]
    keys = [(int(c.var_tid[v]), int(c.var_pos[v])) for v in usable]
    o.n_cis = np.zeros(K, np.uint32)
    o.perm_r = np.full((K, B + 1), np.nan if only is not None else 0.0)
    o.best_variant, o.best_r, o.best_slope = np.full(K, NO_PAIR, np.uint32), np.zeros(K), np.zeros(K)
    o.n_ge = np.zeros(K, np.uint32)
    for k in rows:
        lo, hi = ref.cis_range(keys, c.regions[k], c.window) if o.yy[k] > 1e-12 * S else (0, 0)
        o.n_cis[k] = hi - lo
        for b in range(B + 1):
            if only is not None and (k, b) not in only:
                continue
            p = [int(x) for x in perms[b]]
            top, at = 0, None
            for u in range(lo, hi):
                v = usable[u]
                if G[v] is None:
                    assert variant(v) == 0
                acc = 0.0
                for s in range(S):
                    acc = ref.fma(Y[k][p[s]], G[v][s], acc)
                r = acc / math.sqrt(o.yy[k] * o.gg[v])
                if at is None or bits(r) > top:
                    top, at = bits(r), (v, r, acc / o.gg[v])
            o.perm_r[k, b] = struct.unpack("<d", struct.pack("<Q", top))[0]
            if b == 0 and at is not None:
                o.best_variant[k], o.best_r[k], o.best_slope[k] = at
        if only is None:
            o.n_ge[k] = sum(1 for b in range(1, B + 1) if bits(o.perm_r[k, b]) >= bits(o.perm_r[k, 0]))
    o.n_pairs = int(o.n_cis.sum())
    return o


def same_perm_result(a, b):
    """Every array of two results (library against library): the integers exactly, the doubles as bit patterns, NaN included."""
    assert (a.n_pairs, a.n_perm, a.dof) == (b.n_pairs, b.n_perm, b.dof)
    for f in ("variant_verdict", "n_cis", "best_variant", "n_ge", "beta_status"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for f in ("yy", "gg", "perm_r", "best_r", "best_slope", "p_perm", "beta_shape1", "beta_shape2", "p_beta"):
        ref.same_bits(getattr(a, f), getattr(b, f))


# ---- the special functions -------------------------------------------------------------------------------------------------------------------------
PSI_X = (1e-3, 0.5, 1.0, 2.5, 10.0, 1e3, 1e6)
BETA_AB = (0.3, 1.0, 2.5, 40.0, 900.0)
BETA_X = (1e-12, 1e-3, 0.2, 0.5, 0.9, 1 - 1e-9)


def rel(got, want):
    """|got - want| / |want| against an mpmath number; a reference below the smallest normal double is met by any result at or below that."""
    import mpmath
    if abs(want) < DBL_MIN:
        return 0.0 if abs(got) <= DBL_MIN else math.inf
    return float(abs(mpmath.mpf(got) - want) / abs(want))


def measure_special(digamma, trigamma, betainc):
    """The largest relative errors (digamma, trigamma, betainc) of three functions f(x), f(x), f(x, a, b) against mpmath at 50 digits."""
    import mpmath
    with mpmath.workdps(50):
        d = max(rel(float(digamma(x)), mpmath.digamma(mpmath.mpf(x))) for x in PSI_X)
        t = max(rel(float(trigamma(x)), mpmath.polygamma(1, mpmath.mpf(x))) for x in PSI_X)
        i = max(rel(float(betainc(x, a, b)), mpmath.betainc(mpmath.mpf(a), mpmath.mpf(b), 0, mpmath.mpf(x), regularized=True))
                for a in BETA_AB for b in BETA_AB for x in BETA_X)
    return d, t, i


def scipy_special():
    from scipy import special
    return special.digamma, lambda x: special.polygamma(1, x), lambda x, a, b: special.betainc(a, b, x)


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------------------
def perm_pvalues(q, k, tstat, pvalue):
    """p_b for b = 1 .. B of row k, clipped as the contract says."""
    return np.array([min(max(pvalue(tstat(float(r), q.dof), q.dof), DBL_MIN), P_MAX) for r in q.perm_r[k, 1:]])


def fit_reference(p):
    from scipy.stats import beta
    a, b, _, _ = beta.fit(p, floc=0, fscale=1)
    return a, b


def fit_mpmath(p):
    """The root of the two digamma equations from the moment start, at 30 digits."""
    import mpmath
    with mpmath.workdps(30):
        x = [mpmath.mpf(float(v)) for v in p]
        n = len(x)
        l1, l2 = sum(mpmath.log(v) for v in x) / n, sum(mpmath.log(1 - v) for v in x) / n
        m = sum(x) / n
        var = sum((v - m) ** 2 for v in x) / n
        a0 = m * (m * (1 - m) / var - 1)
        b0 = a0 * (1 / m - 1)
        f = lambda a, b: (mpmath.digamma(a) - mpmath.digamma(a + b) - l1, mpmath.digamma(b) - mpmath.digamma(a + b) - l2)
        r = mpmath.findroot(f, (a0, b0))
        return float(r[0]), float(r[1])


# ---- text ------------------------------------------------------------------------------------------------------------------------------------------
def g17(x):
    return "nan" if x != x else "%.17g" % x


def text(ids, variant_ids, var_pos, starts, q, tstat, pvalue):
    """The Python writer of rgx_cohort_format_qtl_perm: ids[k] the phenotype IDs, starts[k] the rows' starts; tstat and pvalue the library's host
    functions."""
    out = ["phenotype_id\tnum_var\tbeta_shape1\tbeta_shape2\tdof\tvariant_id\tdistance\tr\tslope\tslope_se\ttstat\tpval_nominal\tpval_perm\tpval_beta\n"]
    for k in range(len(ids) if q is not None else 0):
        if not q.n_cis[k]:
            continue
        v = int(q.best_variant[k])
        r, slope = float(q.best_r[k]), float(q.best_slope[k])
        t = tstat(r, q.dof)
        se = slope / t if not math.isinf(t) else math.copysign(0.0, slope * t)
        out.append("\t".join([ids[k], "%d" % q.n_cis[k], g17(q.beta_shape1[k]), g17(q.beta_shape2[k]), "%d" % q.dof, variant_ids[v],
                              "%d" % (int(var_pos[v]) - int(starts[k])), g17(r), g17(slope), g17(se), g17(t), g17(pvalue(t, q.dof)),
                              g17(q.p_perm[k]), g17(q.p_beta[k])]) + "\n")
    return "".join(out).encode()
