"""Inputs the trans-sQTL scan tests share (tests/test_cohort_qtl_trans_host.py, tests/test_gpu_cohort_qtl_trans.py): the planted tables of
tests/qtl_cases.py with trans effects added in front of the ranking.  qtl_cases.planted() hands out ranks, not what it ranked, so the phenotypes
are drawn again here the way it draws them -- noise, the covariates, for every third row the dosage of its anchor -- and every fourth row also
carries the dosage of a usable variant on the row's OTHER contig: the planted trans pairs, c.trans = [(row, variant)].  The threshold of the
planted cases is p = PVAL with the cis pairs inside qtl_cases.WINDOW left out."""
import functools

import numpy as np

import qtl_cases as qc

PVAL = 0.01
EFFECT = 1.5
# (twelve samples leave ten degrees of freedom, where p = 0.01 asks for |r| >= 0.708: with 1.5 the restatement finds none of that case's three
# planted pairs, with 2.5 two of them)
SMALL_EFFECT = 2.5
PLANTED = qc.PLANTED


def planted(S, K, V, n_cov, seed=None, effect=EFFECT, **kw):
    c = qc.planted(S, K, V, n_cov, seed=seed, **kw)
    rng = np.random.default_rng((S * 1000003 + K * 1009 + V * 17 + n_cov if seed is None else seed) + 77)
    filled = np.where(c.dosage >= 0, c.dosage, 1).astype(np.float64)
    X = rng.standard_normal((K, S))
    if n_cov:
        X += rng.standard_normal((K, n_cov)) @ c.cov * 0.5
    for k in range(0, K, 3):
        if V:
            X[k] += 0.9 * filled[c.anchor[k]]
    plain = np.setdiff1d(np.arange(V), c.special)
    others = {int(t): plain[c.var_tid[plain] != t] for t in np.unique(c.regions[:, 0])}
    trans = []
    for k in range(0, K, 4):
        other = others[int(c.regions[k, 0])]
        if len(other):
            v = int(other[int(rng.integers(0, len(other)))])
            X[k] += effect * filled[v]
            trans.append((k, v))
    c.rank2 = qc.rank2_of(X)
    c.trans = trans
    return c


@functools.lru_cache(maxsize=None)
def case(S, K, V, n_cov):
    """planted() of one of PLANTED with its own seed, computed once; read-only."""
    c = planted(S, K, V, n_cov, effect=SMALL_EFFECT if S < 20 else EFFECT)
    for a in (c.rank2, c.regions, c.var_tid, c.var_pos, c.dosage, c.cov):
        a.setflags(write=False)
    return c


def hit_pairs(q):
    """The (row, input variant) pairs of a result's hits, in order."""
    begin = np.asarray(q.hit_begin).astype(np.int64)
    rows = np.repeat(np.arange(len(begin) - 1), np.diff(begin))
    return list(zip(rows.tolist(), np.asarray(q.hit_variant).tolist()))


def check_conditions(c, q):
    """What every planted case must meet so that it cannot pass by comparing nothing (q: a result, from the restatement or the library)."""
    assert q.n_tested > 0
    assert q.n_hits >= 1
    assert 4 * q.n_hits <= q.n_tested, "more than a quarter of the pairs are hits"
    found = set(hit_pairs(q)) & set(c.trans)
    assert c.trans and 2 * len(found) >= len(c.trans), "fewer than half of the planted trans pairs are hits"
