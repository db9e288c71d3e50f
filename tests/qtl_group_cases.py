"""Inputs of the grouped permutation pass tests (tests/test_cohort_qtl_group_host.py, tests/test_gpu_cohort_qtl_group.py) beside tests/qtl_cases.py
and tests/qtl_perm_cases.py: groupings of a table's rows, a table made for ties, tables whose rows have chosen numbers of cis variants, and tables
with rows that have no cis variant or are flat."""
import numpy as np

import qtl_cases as qc

NO_GROUP = 0xffffffff
NO_PAIR = 0xffffffff


def singletons(K):
    """Every row its own group."""
    return np.arange(K, dtype=np.uint32), K


def one_group(K):
    return np.zeros(K, np.uint32), 1


def round_robin(K, out=1):
    """Rows dealt into three groups in turn -- no group is contiguous -- with row `out` in no group."""
    g = (np.arange(K) % 3).astype(np.uint32)
    g[out] = NO_GROUP
    return g, 3


def runs(K, seed, longest=8):
    """Consecutive runs of 1 .. longest rows."""
    rng = np.random.default_rng(seed)
    g, k, n = np.zeros(K, np.uint32), 0, 0
    while k < K:
        size = int(rng.integers(1, longest + 1))
        g[k:k + size] = n
        k, n = k + size, n + 1
    return g, n


def members(groups, g):
    return [int(k) for k in np.nonzero(np.asarray(groups) == g)[0]]


# ---- ties ------------------------------------------------------------------------------------------------------------------------------------------
TIE_POS = np.array([100, 200, 300, 400, 500, 600], np.uint32)
ALL, ONLY_3, ONLY_5 = (0, 100, 600), (0, 400, 401), (0, 600, 601)


def tie_base():
    """S = 16, K = 8, V = 6 on one contig under window 0; every row's region covers all six variants; row 1 is 5 x the dosage of variant 3 plus
    a little noise, the others are noise: the largest |r| of the table is (row 1, variant 3) -- asserted by the callers through the nominal scan."""
    rng = np.random.default_rng(20261019)
    S, K, V = 16, 8, 6
    dosage = np.array([rng.permutation(np.resize(np.array([0, 1, 2], np.int8), S)) for _ in range(V)], np.int8)
    X = rng.standard_normal((K, S))
    X[1] = 5.0 * dosage[3] + 0.1 * rng.standard_normal(S)
    return qc.Case(rank2=qc.rank2_of(X), regions=np.tile(np.array([ALL], np.uint32), (K, 1)), var_tid=np.zeros(V, np.uint32), var_pos=TIE_POS.copy(),
                   dosage=dosage, cov=np.zeros((0, S)), window=0)


def tie_rows():
    """Rows 1 and 4 are the same row: in one group the lower row wins.  Expected: best_row 1, best_variant 3."""
    c = tie_base()
    r2 = c.rank2.copy()
    r2[4] = r2[1]
    return qc.Case(**dict(c.__dict__, rank2=r2))


def tie_variants(other):
    """Variant `other` has variant 3's dosages: the earlier of the two wins.  Expected: best_row 1, best_variant min(3, other)."""
    c = tie_base()
    d = c.dosage.copy()
    d[other] = d[3]
    return qc.Case(**dict(c.__dict__, dosage=d))


def tie_across():
    """Rows 1 and 4 are the same row and variants 3 and 5 the same variant; row 1 reaches variant 5 alone, row 4 variant 3 alone: a later variant
    of an earlier row against an earlier variant of a later row.  Expected: best_row 1, best_variant 5."""
    c = tie_base()
    r2, d, reg = c.rank2.copy(), c.dosage.copy(), c.regions.copy()
    r2[4] = r2[1]
    d[5] = d[3]
    reg[1], reg[4] = ONLY_5, ONLY_3
    return qc.Case(**dict(c.__dict__, rank2=r2, dosage=d, regions=reg))


def tie_wide():
    """S = 16, K = 20, V = 150 on one contig under the widest window: every row reaches every variant, three tiles of them.  Rows 2 and 18 are the
    same row, 5 x the dosage of variant 7 plus a little noise, and variant 140 has variant 7's dosages.  Group 0 = rows 2 .. 18, group 1 = rows 0, 1
    and 19.  Expected: best_row[0] 2, best_variant[0] 7.  Returns (case, groups)."""
    c = qc.simple(16, 20, 150, 0, seed=5, contigs=1)
    rng = np.random.default_rng(6)
    d = c.dosage.copy()
    d[7] = rng.permutation(np.resize(np.array([0, 1, 2], np.int8), 16))
    d[140] = d[7]
    X = rng.standard_normal((20, 16))
    X[2] = 5.0 * d[7] + 0.1 * rng.standard_normal(16)
    X[18] = X[2]
    groups = np.array([1, 1] + [0] * 17 + [1], np.uint32)
    return qc.Case(**dict(c.__dict__, rank2=qc.rank2_of(X), dosage=d, window=0xffffffff)), groups


# ---- chosen numbers of cis variants -----------------------------------------------------------------------------------------------------------------
def two_rows_with(S, n0, n1, seed, window=qc.WINDOW):
    """qc.simple (every variant usable) on one contig, its positions redrawn without equals, under window 0: row 0 reaches the first n0 variants and
    row 1 the first n1 (none when 0); the other three rows have the few variants inside their introns.  K = 5."""
    V = max(n0, n1, 8)
    c = qc.simple(S, 5, V, 0, seed=seed, window=window, span=4 * window, contigs=1)
    pos = (1 + np.sort(np.random.default_rng(seed).choice(4 * window, V, replace=False))).astype(np.uint32)
    regions = c.regions.copy()
    for k, n in ((0, n0), (1, n1)):
        regions[k] = (0, 1, pos[n - 1]) if n else (0, 4 * window + 10, 4 * window + 20)
    return qc.Case(**dict(c.__dict__, regions=regions, var_pos=pos, window=0))


def rows_with(S, counts, seed, window=qc.WINDOW):
    """two_rows_with for every row: row k reaches the first counts[k] variants (none when 0).  K = len(counts)."""
    V = max(max(counts), 8)
    c = qc.simple(S, len(counts), V, 0, seed=seed, window=window, span=4 * window, contigs=1)
    pos = (1 + np.sort(np.random.default_rng(seed).choice(4 * window, V, replace=False))).astype(np.uint32)
    regions = np.array([(0, 1, pos[n - 1]) if n else (0, 4 * window + 10, 4 * window + 20) for n in counts], np.uint32)
    return qc.Case(**dict(c.__dict__, regions=regions, var_pos=pos, window=0))


# the smallest table that crosses the slab's tail (S = 17), a variant-tile edge (64 and 65 cis variants) and has members without pairs between
# members with pairs: singleton groups of it against the ungrouped pass
MERGED_S, MERGED_COUNTS = 17, (0, 1, 65, 0, 64)


def merged_case():
    return rows_with(MERGED_S, MERGED_COUNTS, seed=1765)


# ---- rows without pairs -----------------------------------------------------------------------------------------------------------------------------
FAR = (1, 4 * qc.WINDOW * 3 + 10 * qc.WINDOW + 5, 4 * qc.WINDOW * 3 + 10 * qc.WINDOW + 300)   # qc.planted's far region for V = 24


def degenerate():
    """qc.case(30, 20, 24, 2) with rows 0, 3 and 7 moved where no variant reaches (row 19 lies there already) and rows 12 and 13 flat.  Groups:
    0 = {0, 1, 2} (its first member has no cis variant), 1 = {6, 7, 8} (its middle one), 2 = {17, 18, 19} (its last one), 3 = {12, 13} (flat rows
    alone), 4 = {} (empty), 5 = {3} (a lone row without cis variants); the other rows are in no group.  Returns (case, groups, n_groups, the
    groups without pairs)."""
    c = qc.case(30, 20, 24, 2)
    assert tuple(int(x) for x in c.regions[19]) == FAR
    reg, r2 = c.regions.copy(), c.rank2.copy()
    reg[0] = reg[7] = reg[3] = FAR
    r2[12] = r2[13] = 20
    g = np.full(20, NO_GROUP, np.uint32)
    g[[0, 1, 2]], g[[6, 7, 8]], g[[17, 18, 19]], g[[12, 13]], g[3] = 0, 1, 2, 3, 5
    return qc.Case(**dict(c.__dict__, regions=reg, rank2=r2)), g, 6, (3, 4, 5)
