"""Inputs the refinement tests share (tests/test_cohort_refine_host.py, tests/test_gpu_cohort_refine.py): the hand-made cohort with its expectations
written out, the rows of the wide compare, the heavy-tailed random cohort and the chains whose survivors number exactly what the compaction's
edges need."""
import numpy as np

import cluster_cases

NO = 0xffffffff


def _rows(rows):
    """(tid, start, end, count, strand) -> the rows table_from_rows takes, with thick bounds that contain the junction."""
    return [(t, s, e, s - 10, e + 10, c, strand) for t, s, e, c, strand in rows]


HAND_P = _rows([(0, 100, 200, 60, "+"), (0, 100, 220, 25, "+"), (0, 100, 300, 3, "+"), (0, 250, 300, 40, "+"), (0, 250, 5000, 50, "+"),
                (0, 400, 500, 2, "+"), (0, 400, 600, 3, "+"), (0, 700, 800, 30, "-"), (0, 700, 850, 10, "-")])
HAND_Q = _rows([(0, 100, 200, 20, "+"), (0, 100, 220, 5, "+"), (0, 100, 300, 1, "+"), (0, 150, 300, 6, "+"), (0, 400, 500, 1, "+"),
                (0, 400, 600, 4, "+"), (1, 100, 200, 9, "+")])
# the matrix: chrA 100-200 +, 100-220 +, 100-300 +, 150-300 +, 250-300 +, 250-5000 +, 400-500 +, 400-600 +, 700-800 -, 700-850 -, chrB 100-200 +
HAND_ROWS = [(0, 100, 200, "+"), (0, 100, 220, "+"), (0, 100, 300, "+"), (0, 150, 300, "+"), (0, 250, 300, "+"), (0, 250, 5000, "+"), (0, 400, 500, "+"),
             (0, 400, 600, "+"), (0, 700, 800, "-"), (0, 700, 850, "-"), (1, 100, 200, "+")]
HAND_TOTALS = [80, 30, 4, 6, 40, 50, 3, 7, 30, 10, 9]
CUSTOM = dict(max_intron=1000, min_reads=4, min_ratio=(1, 20))
# (parameters, the literals: whichever of the counts and arrays the expectation names)
HAND = [
    (dict(), dict(n_ineligible=0, n_weak=0, n_components=4, cluster=[0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3])),
    (CUSTOM, dict(n_ineligible=1, n_weak=3, n_components=5, cluster=[0, 0, NO, NO, 1, NO, NO, 2, 3, 3, 4], cl_begin=[0, 2, 3, 4, 6, 7],
                  cl_row=[0, 1, 4, 7, 8, 9, 10], cl_total=[110, 40, 7, 40, 9], cs_begin=[0, 2, 3, 5, 6, 7], cs_sample=[0, 1, 0, 0, 1, 0, 1],
                  cs_total=[85, 25, 40, 3, 4, 40, 9],
                  text=["chrom p q",
                        "chrA:100:200:clu_1_+ 60/85 20/25",
                        "chrA:100:220:clu_1_+ 25/85 5/25",
                        "chrA:250:300:clu_2_+ 40/40 0/0",
                        "chrA:400:600:clu_3_+ 3/3 4/4",
                        "chrA:700:800:clu_4_- 30/40 0/0",
                        "chrA:700:850:clu_4_- 10/40 0/0",
                        "chrB:100:200:clu_5_+ 0/0 9/9"])),
    (dict(CUSTOM, min_rows=2), dict(n_components=5, cluster=[0, 0, NO, NO, NO, NO, NO, NO, 1, 1, NO], cl_total=[110, 40], cs_total=[85, 25, 40])),
    (dict(CUSTOM, max_intron=0), dict(n_ineligible=0, cluster=[0, 0, NO, NO, 1, 1, NO, 2, 3, 3, 4], cl_total=[110, 90, 7, 40, 9])),
    (dict(CUSTOM, min_reads=0), dict(n_weak=2, cluster=[0, 0, NO, NO, 1, NO, 2, 2, 3, 3, 4], cl_total=[110, 40, 10, 40, 9])),
    (dict(CUSTOM, min_ratio=(0, 1)), dict(n_weak=1, cluster=[0, 0, 0, 0, 0, NO, NO, 1, 2, 2, 3], cl_total=[160, 7, 40, 9], cs_total=[128, 32, 3, 4, 40, 9])),
]
# the boundary of the ratio test: row 2 has 4 reads in a stage-1 cluster of T = 160 under max_intron=1000; 4 * 40 = 160 is not below 160
BOUNDARY = [(dict(max_intron=1000, min_ratio=(1, 40)), True), (dict(max_intron=1000, min_ratio=(1, 39)), False)]      # (parameters, row 2 stays)

# the wide compare: X counts 4,000,000,000 in each of two samples, Y counts 1; the left product of X's test passes 2^64
WIDE_P = _rows([(0, 100, 200, 4_000_000_000, "+"), (0, 100, 300, 1, "+")])
WIDE_Q = _rows([(0, 100, 200, 4_000_000_000, "+")])
WIDE_RATIO = (2_000_000_000, 4_000_000_000)


def check_literals(cl, m, want):
    """cl: a CohortClusters; want: one of HAND's literal dicts."""
    for k, v in want.items():
        if k == "text":
            assert cl.counts_text(m).decode().splitlines() == v
        elif isinstance(v, list):
            assert [int(x) for x in getattr(cl, k)] == v, k
        else:
            assert int(getattr(cl, k)) == v, k


def heavy_tables(G, tid, start, end, cls):
    """cluster_cases.sample_tables with heavy-tailed counts: row r counts (1 + (7 r + g) % 9) in sample g, times boost(r) in its home sample
    r % G, boost(r) = 1 << (((r * 2654435761) >> 7) % 14) in wrapping 64-bit arithmetic.  (With uniform counts a giant cluster survives whole
    or vanishes whole.)"""
    n = len(tid)
    r = np.arange(n, dtype=np.uint64)
    boost = np.uint64(1) << (((r * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(14))
    tables = []
    for g in range(G):
        bit = ((r * np.uint64(2654435761) + np.uint64(g) * np.uint64(0x9E3779B1)) >> np.uint64(13)) & np.uint64(1)
        home = r % np.uint64(G) == g
        has = (bit == 1) | home
        count = (np.uint64(1) + (np.uint64(7) * r + np.uint64(g)) % np.uint64(9)) * np.where(home, boost, np.uint64(1))
        k = np.flatnonzero(has)
        strand = np.array([ord("+"), ord("-"), ord("?") if g % 2 == 0 else ord(".")], np.uint32)[cls[k]]
        tables.append(cluster_cases.table_of(g, tid[k], start[k], end[k], count[k], strand))
    return tables


# ---- the edges of the compaction: chains in which every third row of the matrix is weak -------------------------------------------------
# rows of the chain -> survivors (rows - rows // 3): 0 (through max_intron), 1, 63, 64, 64, 65, 4095, 4096, 4096, 4097 -- the wave's and the scan
# tile's edges.  The last row is alive when rows % 3 != 0 and weak when rows % 3 == 0 (96 and 6144).
CHAIN_ROWS = [1, 94, 95, 96, 97, 6142, 6143, 6144, 6145]
CHAIN_MIN_READS = 2


def chain(L):
    """A shortened cluster_cases.staircase(): L junctions of one contig in ONE component, row 2j = (S[j], E[j]), row 2j + 1 = (S[j + 1], E[j]).
    Returns (tid, start, end, cls, count); the count is 1 for every matrix row i with i % 3 == 2 (the matrix is in (start, end) order) and 5
    for the others."""
    J = L // 2 + 2
    pi = np.random.default_rng(9).permutation(J)
    S, E = 1000 + 10 * pi, 10_000_000 + 10 * np.arange(J)
    j = np.arange(L) // 2
    start = np.where(np.arange(L) % 2 == 0, S[j], S[j + 1])
    end = E[j]
    order = np.lexsort((end, start))
    count = np.zeros(L, np.int64)
    count[order] = np.where(np.arange(L) % 3 == 2, 1, 5)
    return np.zeros(L, np.int64), start, end, np.zeros(L, np.int64), count


def chain_survivors(L):
    return L - L // 3
