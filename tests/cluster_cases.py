"""Inputs the cluster tests share (tests/test_cohort_clusters_host.py, tests/test_gpu_cohort_clusters.py): the hand-made cohort with its expectation
written out, the random cohort of 199,998 junctions and the staircase, each as per-sample tables through rgx_table_unpack."""
import ctypes as C

import numpy as np

CONTIGS = [("k0", 9_000_000), ("k1", 9_000_001), ("k2", 9_000_002)]
ANCHOR = 8

# (tid, start, end, thick_start, thick_end, count, strand) per sample; every row is taken (only_anchored=False)
HAND_P = [(0, 100, 200, 90, 230, 3, "+"), (0, 100, 300, 90, 330, 2, "+"), (0, 100, 200, 85, 215, 5, "-"), (0, 500, 600, 480, 630, 1, "?"),
          (1, 100, 200, 90, 230, 7, "+")]
HAND_Q = [(0, 100, 200, 95, 240, 1, "+"), (0, 150, 300, 140, 320, 4, "+"), (0, 500, 700, 490, 750, 2, "."), (0, 400, 450, 380, 470, 6, "+")]
# the matrix's rows: chrA 100-200 +, chrA 100-200 -, chrA 100-300 +, chrA 150-300 +, chrA 400-450 +, chrA 500-600 ?, chrA 500-700 ., chrB 100-200 +
#   rows 0, 2 share a start and rows 2, 3 an end (one cluster of three); row 1 has row 0's coordinates on the other strand (alone); rows 5 and 6
#   share a start and are both class 2; row 7 has row 0's coordinates on another contig (alone); row 4 shares nothing
HAND = dict(n_components=5, cluster=[0, 1, 0, 0, 2, 3, 3, 4], cl_begin=[0, 3, 4, 5, 7, 8], cl_row=[0, 2, 3, 1, 4, 5, 6, 7], cl_total=[10, 5, 6, 3, 7],
            cs_begin=[0, 2, 3, 4, 6, 7], cs_sample=[0, 1, 0, 1, 0, 1, 0], cs_total=[5, 5, 5, 6, 1, 2, 7],
            text=["chrom p q",
                  "chrA:100:200:clu_1_+ 3/5 1/5",
                  "chrA:100:200:clu_2_- 5/5 0/0",
                  "chrA:100:300:clu_1_+ 2/5 0/5",
                  "chrA:150:300:clu_1_+ 0/5 4/5",
                  "chrA:400:450:clu_3_+ 0/0 6/6",
                  "chrA:500:600:clu_4_NA 1/1 0/2",
                  "chrA:500:700:clu_4_NA 0/1 2/2",
                  "chrB:100:200:clu_5_+ 7/7 0/0"])
NO = 0xffffffff
HAND_MIN_ROWS_2 = dict(n_components=5, cluster=[0, NO, 0, 0, NO, 1, 1, NO], cl_begin=[0, 3, 5], cl_row=[0, 2, 3, 5, 6], cl_total=[10, 3],
                       cs_begin=[0, 2, 4], cs_sample=[0, 1, 0, 1], cs_total=[5, 5, 1, 2],
                       text=["chrom p q", "chrA:100:200:clu_1_+ 3/5 1/5", "chrA:100:300:clu_1_+ 2/5 0/5", "chrA:150:300:clu_1_+ 0/5 4/5",
                             "chrA:500:600:clu_2_NA 1/1 0/2", "chrA:500:700:clu_2_NA 0/1 2/2"])


class Sample(object):
    """What Cohort.add and cohort.merge_host read of an extractor, over a hand-made table."""

    def __init__(self, table):
        self.table, self.min_anchor_length_, self._ctx = table, ANCHOR, None


def table_of(g, name, start, end, count, strand):
    """Sample g's table: its header lists CONTIGS rotated by g % 3 (the samples do not agree on the tids); thick bounds start - 8 and end + 8."""
    from regtools_amd import _ffi
    k = len(CONTIGS)
    order = CONTIGS[g % k:] + CONTIGS[:g % k]
    rows = np.zeros((len(name), 12), np.uint32)
    rows[:, 0] = (name - g % k) % k
    for j, col in enumerate((start, end, start - ANCHOR, end + ANCHOR, count)):
        rows[:, 1 + j] = col
    rows[:, 10] = strand
    proto = _ffi.JunctionTable()
    arr = (C.c_char_p * k)(*[c[0].encode() for c in order])
    lens = (C.c_uint32 * k)(*[c[1] for c in order])
    proto.n_ref, proto.ref_name, proto.ref_len = k, arr, lens
    t = C.POINTER(_ffi.JunctionTable)()
    raw = rows.tobytes()
    assert _ffi.lib().rgx_table_unpack(raw, len(rows), C.byref(proto), C.byref(t)) == 0
    return t


def random_junctions():
    """The issue's input: (tid, start, end, cls) of 199,998 distinct junctions over 20,000 donors and 20,000 acceptors per contig and class."""
    rng = np.random.default_rng(5)
    U, P = 200_000, 20_000
    tid = rng.integers(0, 3, U)
    cls = rng.integers(0, 3, U)
    d = rng.integers(0, P, U)
    a = rng.integers(0, P, U)
    start = 1000 + 7 * d
    end = 1000 + 7 * P + 1000 + 7 * a
    rows = np.unique(np.stack([tid, start, end, cls], axis=1), axis=0)
    return rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]


def staircase():
    """65,536 junctions in ONE component whose diameter is 65,536: row 2j = (S[j], E[j]), row 2j + 1 = (S[j + 1], E[j])."""
    L = 65_536
    J = L // 2 + 1
    pi = np.random.default_rng(9).permutation(J)
    S, E = 1000 + 10 * pi, 10_000_000 + 10 * np.arange(J)
    j = np.arange(L) // 2
    start = np.where(np.arange(L) % 2 == 0, S[j], S[j + 1])
    end = E[j]
    assert len(set(zip(start.tolist(), end.tolist()))) == L
    return np.zeros(L, np.int64), start, end, np.zeros(L, np.int64)


def sample_tables(G, tid, start, end, cls, big=None):
    """G tables over the junctions r = 0 .. n-1: row r is in sample g when a fixed hash bit says so, and in sample r % G always; its count there is
    1 + (7 r + g) % 9.  big = {row: samples}: the row is in each of those samples and counts 4,000,000,000 there."""
    n = len(tid)
    r = np.arange(n, dtype=np.uint64)
    tables = []
    for g in range(G):
        bit = ((r * np.uint64(2654435761) + np.uint64(g) * np.uint64(0x9E3779B1)) >> np.uint64(13)) & np.uint64(1)
        has = (bit == 1) | (r % np.uint64(G) == g)
        count = 1 + (7 * r + g) % 9
        for row, samples in (big or {}).items():
            if g in samples:
                has[row] = True
                count[row] = 4_000_000_000
        k = np.flatnonzero(has)
        strand = np.array([ord("+"), ord("-"), ord("?") if g % 2 == 0 else ord(".")], np.uint32)[cls[k]]
        tables.append(table_of(g, tid[k], start[k], end[k], count[k], strand))
    return tables


def free_tables(tables):
    from regtools_amd import _ffi
    for t in tables:
        _ffi.lib().rgx_table_free(t)
