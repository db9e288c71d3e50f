"""Inputs of the conditional pass tests (tests/test_cohort_qtl_cond_host.py, tests/test_gpu_cohort_qtl_cond.py) beside tests/qtl_cases.py and
tests/qtl_perm_cases.py: conditioning sets drawn from a row's own usable cis variants, so that every series passes the argument checks."""
import numpy as np

import qtl_cases as qc


def cis_lists(c, cohort, **kw):
    """Per table row the usable cis variants in variant order, from the nominal host twin."""
    a = dict(regions=c.regions, var_tid=c.var_tid, var_pos=c.var_pos, dosage=c.dosage, covariates=c.cov, window=c.window)
    a.update(kw)
    nom = cohort.qtl_nominal_host(cohort.pheno_table_from_rank2(a.pop("rank2", c.rank2)), **a)
    begin = nom.pair_begin.astype(np.int64)
    return [[int(v) for v in nom.pair_variant[begin[k]:begin[k + 1]]] for k in range(c.K)]


def draw(cis, sizes, seed, per_size=None, rows=None, spare=1):
    """[(row, [variants])]: for every m of sizes, series over the rows with at least m + spare cis variants (all, or per_size of them), each
    conditioned on m of its cis variants in a drawn order."""
    rng = np.random.default_rng(seed)
    out = []
    for m in sizes:
        ok = [k for k in (range(len(cis)) if rows is None else rows) if len(cis[k]) >= m + spare]
        if per_size is not None and len(ok) > per_size:
            ok = sorted(int(k) for k in rng.choice(ok, per_size, replace=False))
        for k in ok:
            out.append((k, [int(v) for v in rng.choice(cis[k], m, replace=False)]))
    return out


def wide(S, n_cis, V, seed):
    """qtl_perm_cases.rows_with: row 0 has exactly n_cis cis variants, every variant usable."""
    import qtl_perm_cases as pcs
    return pcs.rows_with(S, n_cis, V, seed)


def lstsq_case():
    return qc.case(70, 24, 40, 4)


def lstsq_series(cis):
    """The series of the least-squares check and of the constant's measurement: every row of lstsq_case() with enough cis variants, m = 1 .. 4."""
    return draw(cis, (1, 2, 3, 4), seed=70)


# ---- the planted case of the forward-backward pass ------------------------------------------------------------------------------------------------
INDEP = dict(S=120, n_two=8, n_one=8, n_null=10, n_tag=4, per_row=7, B=199, perm_seed=5, p_threshold=0.01, max_signals=4)
INDEP_SEED = 9       # chosen on the CPU under the twin (seeds 0 .. 11 tried): every condition of the planted test holds, and a tag row drops its tag


def indep_case(seed=None, **kw):
    """One contig, one covariate, every row with its own cluster of per_row variants a window apart from the next row's, so that a row's cis
    variants are exactly its cluster.  Four kinds of row: TWO of its variants act on it independently (effects 1.6 and 1.2 per allele beside unit
    noise), ONE does (1.6), NONE does, and TAG rows: two causal variants A and B (1.0 and 2.0) and a third variant T = min(2, A + B), which
    is the strongest marginally, goes in first and has nothing left to say once A and B are both in.  Dosages are drawn independently, none
    missing.  Returns the case with .two, .one, .null and .tag: per kind a list of (row, [planted variants])."""
    p = dict(INDEP, **kw)
    rng = np.random.default_rng(INDEP_SEED if seed is None else seed)
    S, per = p["S"], p["per_row"]
    K = p["n_two"] + p["n_one"] + p["n_null"] + p["n_tag"]
    V = K * per
    window = qc.WINDOW
    var_pos = np.concatenate([1 + 10 * window * k + window + np.sort(rng.choice(window, per, replace=False)) for k in range(K)]).astype(np.uint32)
    regions = np.array([(0, 1 + 10 * window * k + window + window // 2, 1 + 10 * window * k + window + window // 2 + 50) for k in range(K)], np.uint32)
    dosage = rng.binomial(2, rng.uniform(0.25, 0.5, V)[:, None], (V, S)).astype(np.int8)
    cov = rng.standard_normal((1, S))
    X = rng.standard_normal((K, S)) + rng.standard_normal((K, 1)) @ cov * 0.5
    kinds = {"two": [], "one": [], "null": [], "tag": []}
    for k in range(K):
        mine = [k * per + int(i) for i in rng.choice(per, 3, replace=False)]
        if k < p["n_two"]:
            X[k] += 1.6 * dosage[mine[0]] + 1.2 * dosage[mine[1]]
            kinds["two"].append((k, sorted(mine[:2])))
        elif k < p["n_two"] + p["n_one"]:
            X[k] += 1.6 * dosage[mine[0]]
            kinds["one"].append((k, mine[:1]))
        elif k < p["n_two"] + p["n_one"] + p["n_null"]:
            kinds["null"].append((k, []))
        else:
            a, b, t = mine
            dosage[a], dosage[b] = rng.binomial(2, 0.3, S), rng.binomial(2, 0.3, S)
            dosage[t] = np.minimum(2, dosage[a].astype(np.int64) + dosage[b]).astype(np.int8)
            X[k] += 1.0 * dosage[a] + 2.0 * dosage[b]
            kinds["tag"].append((k, [a, b, t]))
    for v in range(V):
        if dosage[v].min() == dosage[v].max():
            dosage[v, :2] = (dosage[v, 0] + 1) % 3, (dosage[v, 0] + 2) % 3
    c = qc.Case(rank2=qc.rank2_of(X), regions=regions, var_tid=np.zeros(V, np.uint32), var_pos=var_pos, dosage=dosage, cov=cov, window=window)
    c.__dict__.update(kinds)
    return c
