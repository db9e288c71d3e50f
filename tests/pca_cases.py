"""Inputs the principal component tests share (tests/test_cohort_pcs_host.py, tests/test_gpu_cohort_pcs.py): K x S tables of rank2 with a planted
low-rank structure, so that the leading eigenvalues of the quantiles' covariance stand apart and their components are well defined."""
import functools

import numpy as np

# (K, S, n_f, ties).  With seed K * 1000 + S the gaps among the first n_f + 1 eigenvalues (n_f capped at S - 1), as sklearn gives them, are at least
# 0.05 of the largest -- the smallest, 0.053, at (2000, 129); the tests that compare components assert it.
SHAPES = [(40, 5, 3, False), (1025, 9, 4, False), (1025, 9, 4, True), (300, 65, 5, False), (4097, 3, 2, False), (65537, 3, 2, True),
          (2000, 129, 6, True)]
MIN_GAP = 0.05


def planted(K, S, n_f, seed=None, ties=False):
    """rank2 (K x S uint32) of X = F L + 0.5 N: F (K x n_f) standard normal, L (n_f x S) standard normal rows scaled by 3 * 0.7**i, N (K x S)
    standard normal, drawn in this order from default_rng(seed); ties: X rounded to halves.  rank2 = twice scipy's average rank per column."""
    from scipy.stats import rankdata
    rng = np.random.default_rng(K * 1000 + S if seed is None else seed)
    F = rng.standard_normal((K, n_f))
    L = rng.standard_normal((n_f, S)) * (3 * 0.7 ** np.arange(n_f))[:, None]
    X = F @ L + 0.5 * rng.standard_normal((K, S))
    if ties:
        X = np.round(X * 2) / 2
    r2 = 2 * rankdata(X, axis=0)
    assert (r2 == np.round(r2)).all()
    return r2.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def shape(K, S, n_f, ties):
    """planted() of one of SHAPES with its own seed, computed once; read-only."""
    r2 = planted(K, S, n_f, ties=ties)
    r2.setflags(write=False)
    return r2


def random_rank2(K, S, seed):
    """Columns that are random permutations of 1 .. K, doubled: no structure, no ties."""
    rng = np.random.default_rng(seed)
    return (2 * (np.argsort(rng.random((K, S)), axis=0) + 1)).astype(np.uint32)
