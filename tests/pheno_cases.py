"""Inputs the phenotype tests share (tests/test_cohort_pheno_host.py, tests/test_gpu_cohort_pheno.py): cohorts of a chosen number of samples and
rows whose clusters are known by construction, as per-sample tables through rgx_table_unpack (cluster_cases.table_of)."""
import numpy as np

import cluster_cases

SAMPLE_COUNTS = [1, 2, 8, 9, 63, 64, 65, 129]


def groups_of(n_rows):
    """Row r's cluster by construction: rows 2 j and 2 j + 1 share a start; an odd last row joins the pair before it (a cluster of three)."""
    g = np.arange(n_rows) // 2
    if n_rows % 2 and n_rows > 1:
        g[-1] = g[-2]
    return g


def junctions(n_rows):
    """(tid, start, end) of n_rows junctions of one contig in matrix order, clustered as groups_of says (no two clusters share a site)."""
    g, r = groups_of(n_rows), np.arange(n_rows)
    start = 1000 + 100 * g
    return np.zeros(n_rows, np.int64), start, start + 40 + 7 * (r - 2 * g)


def counts(S, n_rows, seed, absent=0.0, empty_clusters=(), duplicates=0):
    """n_rows x S counts, 1 .. 59; an entry is 0 (the sample lacks the junction) with probability `absent`; empty_clusters = [(sample, k, of)]:
    the sample has no reads in the clusters j with j % of == k -- every row of those is missing there; duplicates: for that many j, cluster
    6 j + 3 (rows 12 j + 6, + 7) carries the counts of cluster 6 j (rows 12 j, + 1): equal rows, ties in every column."""
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 60, (n_rows, S))
    c[rng.random((n_rows, S)) < absent] = 0
    for j in range(duplicates):
        c[12 * j + 6: 12 * j + 8] = c[12 * j: 12 * j + 2]
    g = groups_of(n_rows)
    for s, k, of in empty_clusters:
        c[g % of == k, s] = 0
    return c


def tables(count):
    """One table per column of `count` (n_rows x S): the rows whose count there is not 0."""
    n_rows, S = count.shape
    tid, start, end = junctions(n_rows)
    out = []
    for s in range(S):
        k = np.flatnonzero(count[:, s])
        out.append(cluster_cases.table_of(s, tid[k], start[k], end[k], count[k, s], np.full(len(k), ord("+"), np.uint32)))
    return out


def names(S):
    return ["s%03d" % s for s in range(S)]


# K = 1: rows A and B of one cluster over three samples with counts a = 2 b + 1, so that B's ratio (b + 0.5) / (a + b + 0.5) is 1/3 in every
# sample -- flat -- while A's, (a + 0.5) / (a + b + 0.5) = 3.5/4.5, 5.5/7.5, 7.5/10.5, varies
ONE_KEPT = np.array([[3, 5, 7], [1, 2, 3]])
