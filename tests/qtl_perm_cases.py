"""Inputs of the permutation pass tests (tests/test_cohort_qtl_perm_host.py, tests/test_gpu_cohort_qtl_perm.py) beside tests/qtl_cases.py: a planted
table whose effects are strong enough that no permutation reaches them, and tables whose rows have a chosen number of cis variants."""
import functools

import numpy as np

import qtl_cases as qc

STRONG = (64, 30, 40, 1)       # S, K, V, n_cov
STRONG_B = 199


def strong(S, K, V, n_cov, seed=20261019, window=qc.WINDOW):
    """One contig; every row lies within half a window of its anchor variant, so every row has pairs; every third row is 3 x the dosage of its
    anchor plus unit noise, the others are noise; every row carries the covariates.  No dosage is missing, no variant constant."""
    rng = np.random.default_rng(seed)
    span = 4 * window * max(V // 8, 1)
    var_pos = np.sort(1 + rng.integers(0, span, V)).astype(np.uint32)
    var_tid = np.zeros(V, np.uint32)
    dosage = rng.binomial(2, rng.uniform(0.25, 0.5, V)[:, None], (V, S)).astype(np.int8)
    for v in range(V):
        if dosage[v].min() == dosage[v].max():
            dosage[v, :2] = (dosage[v, 0] + 1) % 3, (dosage[v, 0] + 2) % 3
    cov = rng.standard_normal((n_cov, S))
    anchor = rng.integers(0, V, K)
    regions = np.zeros((K, 3), np.uint32)
    for k in range(K):
        start = max(1, int(var_pos[anchor[k]]) + int(rng.integers(-window // 2, window // 2 + 1)))
        regions[k] = (0, start, start + int(rng.integers(1, 400)))
    X = rng.standard_normal((K, S))
    if n_cov:
        X += rng.standard_normal((K, n_cov)) @ cov * 0.5
    for k in range(0, K, 3):
        X[k] += 3.0 * dosage[anchor[k]].astype(np.float64)
    return qc.Case(rank2=qc.rank2_of(X), regions=regions, var_tid=var_tid, var_pos=var_pos, dosage=dosage, cov=cov, window=window, anchor=anchor)


@functools.lru_cache(maxsize=None)
def strong_case():
    c = strong(*STRONG)
    for a in (c.rank2, c.regions, c.var_tid, c.var_pos, c.dosage, c.cov):
        a.setflags(write=False)
    return c


def rows_with(S, n_cis, V, seed, window=qc.WINDOW):
    """qc.simple (every variant usable) on one contig over a span of 4 windows, its positions redrawn without equals, under window 0 with a leading
    row whose region covers the first n_cis variants exactly: that row's n_cis is n_cis, the other rows have the few variants inside their introns.
    K = 5 rows."""
    assert 1 <= n_cis <= V
    c = qc.simple(S, 5, V, 0, seed=seed, window=window, span=4 * window, contigs=1)
    pos = (1 + np.sort(np.random.default_rng(seed).choice(4 * window, V, replace=False))).astype(np.uint32)
    regions = c.regions.copy()
    regions[0] = (0, 1, pos[n_cis - 1])
    return qc.Case(**dict(c.__dict__, regions=regions, var_pos=pos, window=0))
