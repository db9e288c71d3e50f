"""The contract of rgx_cohort_qtl_trans (include/regtools_amd.h) restated in scalar Python on top of tests/qtl_ref.py: every fused multiply-add
an exact rational rounded once, EVERY pair of a row that is not flat and a usable variant, the nominal scan's cis test for the exclusion, the hit
test as a comparison of 64-bit patterns; and the Python writer of rgx_cohort_format_qtl_trans.  Results are compared with the library's as bit
patterns (tests/test_cohort_qtl_trans_host.py, tests/test_gpu_cohort_qtl_trans.py).

The tolerance of rgx_qtl_r_threshold against scipy, relative: R_TOL is four times the largest relative difference between TWO references,
neither the code under test -- r = t / sqrt(dof + t^2) with t = scipy.stats.t.isf(p / 2, dof), against r = sqrt(1 - x) with x =
scipy.special.betaincinv(dof / 2, 1 / 2, p) -- over R_DOFS x R_PS (measure_r() below)."""
import math
import struct

import numpy as np

import qtl_ref as ref

R_DOFS = (1, 2, 10, 60, 997)
R_PS = (0.5, 0.01, 1e-5, 1e-8, 1e-50)
# measured 1.46e-11, at dof 997 and p = 1e-50 (1.36e-11 at dof 60 and p = 0.5): t.isf is the looser of the two
R_MEASURED, R_TOL = 1.46e-11, 4 * 1.46e-11


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", abs(float(x))))[0]


def r_from_t_isf(p, dof):
    from scipy.stats import t as student
    t = student.isf(p / 2.0, dof)
    return t / math.sqrt(dof + t * t)


def r_from_betaincinv(p, dof):
    """p = I_x(dof / 2, 1 / 2) at x = dof / (dof + t^2) = 1 - r^2.  Where p is large, x lies near 1 and 1 - x cancels, so that side is taken
    from the mirrored function, 1 - p = I_(r^2)(1 / 2, dof / 2); where p is small, 1 - p is no longer p's complement to the last bit."""
    from scipy.special import betaincinv
    if p >= 1e-3:
        return math.sqrt(betaincinv(0.5, dof / 2.0, 1.0 - p))
    return math.sqrt(1.0 - betaincinv(dof / 2.0, 0.5, p))


def measure_r():
    """The largest relative difference of the two references over R_DOFS x R_PS."""
    worst = 0.0
    for dof in R_DOFS:
        for p in R_PS:
            a, b = r_from_t_isf(p, dof), r_from_betaincinv(p, dof)
            worst = max(worst, abs(a - b) / a)
    return worst


def excluded(key, region, window):
    """The nominal scan's cis test (qtl_ref.cis_range) for one variant's (tid, pos)."""
    tid, start, end = (int(x) for x in region)
    return (tid, start - min(start, window)) <= key <= (tid, min(end + window, 2 ** 32 - 1))


def restate(c, quantile, r_min, exclude_window, pairs=None):
    """The whole contract for case c (its window is not read).  exclude_window: None keeps the cis pairs.  pairs: None for every pair, else a set
    of (k, v): the others are neither computed nor listed, and n_tested alone stays whole."""
    K, S, V = c.K, c.S, c.V
    T = ref.quantile_table(K, quantile)
    Q = ref.basis(S, c.cov)
    assert Q is not None
    o = ref.Restated()
    o.yy, o.gg, o.variant_verdict = np.zeros(K), np.zeros(V), np.zeros(V, np.uint8)
    Y, G = [None] * K, [None] * V
    for k in range(K):
        Y[k], o.yy[k] = ref.residual([T[int(r) - 2] for r in c.rank2[k]], Q)
    for v in range(V):
        d = [int(x) for x in c.dosage[v]]
        present = [x for x in d if x >= 0]
        if not present or min(present) == max(present):
            o.variant_verdict[v] = 1
            continue
        mean = float(sum(present)) / float(len(present))
        G[v], o.gg[v] = ref.residual([float(x) if x >= 0 else mean for x in d], Q)
        o.variant_verdict[v] = 0 if o.gg[v] > 1e-12 * S else 2
    usable = [v for v in range(V) if o.variant_verdict[v] == 0]
    want = bits(r_min)
    begin, variant, r, slope, tested = [0], [], [], [], 0
    for k in range(K):
        for v in usable if o.yy[k] > 1e-12 * S else []:
            if exclude_window is not None and excluded((int(c.var_tid[v]), int(c.var_pos[v])), c.regions[k], int(exclude_window)):
                continue
            tested += 1
            if pairs is not None and (k, v) not in pairs:
                continue
            acc = 0.0
            for s in range(S):
                acc = ref.fma(Y[k][s], G[v][s], acc)
            rr = acc / math.sqrt(o.yy[k] * o.gg[v])
            if bits(rr) >= want:
                variant.append(v); r.append(rr); slope.append(acc / o.gg[v])
        begin.append(len(variant))
    o.hit_begin, o.hit_variant = np.array(begin, np.uint32), np.array(variant, np.uint32)
    o.r, o.slope = np.array(r, np.float64), np.array(slope, np.float64)
    o.n_hits, o.n_tested = len(variant), tested
    return o


def same_result(a, b):
    """Every array of two results: the integers exactly, the doubles as bit patterns."""
    assert (a.n_hits, a.n_tested) == (b.n_hits, b.n_tested)
    for f in ("variant_verdict", "hit_begin", "hit_variant"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for f in ("yy", "gg", "r", "slope"):
        ref.same_bits(getattr(a, f), getattr(b, f))


def text(ids, variant_ids, q, tstat, pvalue):
    """The Python writer of rgx_cohort_format_qtl_trans: ids[k] the phenotype IDs; tstat and pvalue the library's host functions."""
    out = ["phenotype_id\tvariant_id\tr\tslope\tslope_se\ttstat\tpval\n"]
    for k in range(len(ids) if q is not None else 0):
        for p in range(int(q.hit_begin[k]), int(q.hit_begin[k + 1])):
            t = tstat(float(q.r[p]), q.dof)
            se = float(q.slope[p]) / t if not math.isinf(t) else math.copysign(0.0, float(q.slope[p]) * t)
            out.append("%s\t%s\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\n" % (ids[k], variant_ids[int(q.hit_variant[p])], q.r[p], q.slope[p], se, t,
                                                                       pvalue(t, q.dof)))
    return "".join(out).encode()
