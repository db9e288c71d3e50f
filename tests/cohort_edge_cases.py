"""Inputs of the cohort edge tests (tests/test_cohort_edge_cases_host.py, tests/test_gpu_cohort_edges.py): small cohorts, as data, that put the
integer kernels of csrc/cohort_kernels.hip and the denominator half of csrc/cluster_kernels.hip at their wave, workgroup, form-threshold and
filter edges.  Every case carries CLAIMS -- which kernel form it takes and at what distance from the threshold, which run lengths occur, where
zero counts lie, which clusters have no run -- and `check` proves them from a matrix alone: the restatement's on the CPU, the device's own on
the GPU.  The three thresholds are those of launch_cohort_reduce (n_rows * 32 <= n_triples), of the cluster calls' wave_per_row
(n * 32 <= nnz) and of launch_cluster_cs_sum (n_cs * 32 <= M)."""
import ctypes as C

import numpy as np

import bamio

CONTIGS = [("e0", 4_294_967_295), ("e1", 1_000_000), ("e2", 3_000_000_000)]
ANCHOR = 8
M32 = 0xffffffff
NO = 0xffffffff
P32 = 1 << 32


def row(contig, start, end, count, strand="+", la=ANCHOR, ra=ANCHOR):
    """(contig, start, end, thick_start, thick_end, count, strand character): la and ra are the anchors, start - thick_start and thick_end - end."""
    return (contig, start, end, (start - la) & M32, (end + ra) & M32, count, strand)


class Sample(object):
    """Sample g's rows, each as `row` gives it.  Its header lists CONTIGS rotated by g % 3 (the samples do not agree on the tids); tid is the
    row's contig in THAT order."""

    def __init__(self, g, rows, min_anchor=ANCHOR):
        k = len(CONTIGS)
        self.g, self.min_anchor = g, min_anchor
        self.contigs = CONTIGS[g % k:] + CONTIGS[:g % k]
        a = np.array([r[:6] + (ord(r[6]),) for r in rows], np.int64).reshape(-1, 7)
        self.tid = (a[:, 0] - g % k) % k
        self.start, self.end, self.thick_start, self.thick_end, self.count, self.strand = (a[:, j] for j in range(1, 7))

    def table(self):
        from regtools_amd import _ffi
        rows = np.zeros((len(self.start), 12), np.uint32)
        for j, col in enumerate((self.tid, self.start, self.end, self.thick_start, self.thick_end, self.count)):
            rows[:, j] = col
        rows[:, 10] = self.strand
        proto = _ffi.JunctionTable()
        k = len(self.contigs)
        arr = (C.c_char_p * k)(*[c[0].encode() for c in self.contigs])
        lens = (C.c_uint32 * k)(*[c[1] for c in self.contigs])
        proto.n_ref, proto.ref_name, proto.ref_len = k, arr, lens
        t = C.POINTER(_ffi.JunctionTable)()
        raw = rows.tobytes() or b"\0"
        assert _ffi.lib().rgx_table_unpack(raw, len(rows), C.byref(proto), C.byref(t)) == 0
        return t


class Loaded(object):
    """What Cohort.add and cohort.merge_host read of an extractor, over a Sample's table."""

    def __init__(self, sample):
        self.table, self.min_anchor_length_, self._ctx = sample.table(), sample.min_anchor, None


def load(samples):
    return [Loaded(s) for s in samples]


def free(loaded):
    from regtools_amd import _ffi
    for s in loaded:
        _ffi.lib().rgx_table_free(s.table)


class Case(object):
    """samples and their names; the cohort's parameters (every row, no filter, unless said otherwise); the filter pairs, cluster and refine
    arguments the tests run it with; its claims."""

    def __init__(self, name, samples, claims, only_anchored=False, filters=(), cluster_kw=(dict(),), refine_kw=()):
        self.name, self.samples, self.claims, self.only_anchored = name, samples, claims, only_anchored
        self.names = ["x%03d" % s.g for s in samples]
        self.filters, self.cluster_kw, self.refine_kw = list(filters), list(cluster_kw), list(refine_kw)

    def params(self, min_samples=1, min_total=0):
        return dict(only_anchored=self.only_anchored, min_samples=min_samples, min_total=min_total)

    def __repr__(self):
        return self.name


def qchar(g):
    """The character of a class-2 row in sample g: the samples alternate, so the row's is its last sample's."""
    return "?" if g % 2 == 0 else "."


# ---- accumulate and finish --------------------------------------------------------------------------------------------------------------
def _triples(n, parity):
    """Sample 0 holds n keys, sample 1 those with k % 2 == parity: runs of one and two alternate in the sorted triples."""
    def strand(k, g):
        return ("+", "-", qchar(g))[k % 3]
    s0 = [row(0, 1000 + 10 * k, 1100 + 10 * k + k % 7, 1 + k % 9, strand(k, 0), ANCHOR + k % 5, ANCHOR + k % 3) for k in range(n)]
    s1 = [row(0, 1000 + 10 * k, 1100 + 10 * k + k % 7, 2 + k % 5, strand(k, 1), ANCHOR + k % 4, ANCHOR + k % 6) for k in range(n) if k % 2 == parity]
    last_shared = (n - 1) % 2 == parity
    # key k starts at sorted position k + (keys below k that sample 1 holds); a run of two at 3 j (parity 0) or 3 j + 1 (parity 1)
    at = [p for p in (255, 511) if (p - parity) % 3 == 0 and 2 * ((p - parity) // 3) + parity < n]
    return Case("triples_n%d" % n, [Sample(0, s0), Sample(1, s1)],
                dict(reduce="lane", last_is_head=not last_shared, run_of_two_at=at, n_rows=n, n_triples=n + len(s1)))


def _wave_anchor(i):
    """Row i of the append-waves table sits in lane i % 64 of wave i // 64 of k_cohort_append."""
    w, lane = divmod(i, 64)
    exact = (ANCHOR, ANCHOR)
    short = (ANCHOR - 1, ANCHOR) if lane % 2 else (ANCHOR, ANCHOR - 1)          # one short, on either side
    if w == 0: return short                                                    # nothing: the wave returns early
    if w == 1: return exact if lane == 0 else short
    if w == 2: return exact if lane == 63 else short
    if w == 3: return exact
    if w == 4: return exact if lane % 2 else short
    if w == 5: return (ANCHOR + lane % 13, ANCHOR + lane % 7)
    return exact if lane % 3 == 0 else short                                   # the partial wave


WAVE_ROWS = 64 * 6 + 37


def wave_rows(n=WAVE_ROWS):
    return [row(0, 1000 + 400 * i, 1100 + 400 * i + i % 50, 1 + i % 3, "+-"[i % 2], *_wave_anchor(i)) for i in range(n)]


def wave_masks(sample):
    """Per wave of 64 table rows: the lanes whose row has both anchors, as a 64-bit number."""
    import cohort_ref
    keep = cohort_ref.anchored(sample)
    return [sum(1 << l for l, k in enumerate(keep[w:w + 64]) if k) for w in range(0, len(keep), 64)]


WAVE_BAM_CONTIGS = [("b0", 1_000_000), ("b1", 2_000)]                         # (a BAM header holds signed 32-bit lengths: contigs of its own)
WAVE_MASKS = [0, 1, 1 << 63, (1 << 64) - 1, sum(1 << l for l in range(1, 64, 2))]


def wave_bam_records():
    """The append-waves table as reads: count[i] reads `la`M `end - start`N `ra`M per row at thick_start, in coordinate order, on the first of
    WAVE_BAM_CONTIGS.  `junctions extract` gives the rows of wave_rows back, in their order (its output ascends by thick_start)."""
    recs = []
    for i, (_, start, end, ts, te, count, strand) in enumerate(wave_rows()):
        for c in range(count):
            recs.append(bamio.record(0, ts, "%dM%dN%dM" % (start - ts, end - start, te - end), qname="w%04d_%d" % (i, c), aux=bamio.tagA("XS", strand)))
    return recs


def _waves():
    every = wave_rows(65)
    none = [row(0, 900_000 + 400 * i, 900_100 + 400 * i, 2, "+", ANCHOR - 1 - i % 3, ANCHOR + i % 2) for i in range(64)]
    return Case("append_waves", [Sample(0, wave_rows()), Sample(1, none), Sample(2, [r[:3] + (r[1] - 20, r[2] + 30) + r[5:] for r in every])],
                dict(wave_masks=WAVE_MASKS, sample_without_triples=1), only_anchored=True)


def _shared(S, runs, P, big=False, tag=""):
    """S samples over three shared keys held by runs[0], runs[1] (the first samples) and runs[2] (the last samples) of them, and P private keys.
    Key 0 and key 1 have the same coordinates on the two strands; key 2 is class 2."""
    r0, r1, r2 = runs
    rows = [[] for _ in range(S)]
    for g in range(S):
        if g < r0:                    # the smallest thick_start with the run's last triple, the largest thick_end with triple 64 of a longer run
            la = 40 if g == r0 - 1 else ANCHOR + (g * 5) % 11
            ra = 50 if g == (63 if r0 > 64 else r0 - 1) else ANCHOR + (g * 3) % 13
            rows[g].append(row(0, 2000, 2100, 40_000_000 + g if big else 1 + g % 9, "+", la, ra))
        if g < r1:                    # ... and the other way round
            la = 40 if g == (63 if r1 > 64 else r1 - 1) else ANCHOR + (g * 7) % 11
            ra = 50 if g == r1 - 1 else ANCHOR + (g * 5) % 13
            rows[g].append(row(0, 2000, 2100, 1 + g % 7, "-", la, ra))
        if g >= S - r2:
            rows[g].append(row(2, 5000, 5200, 2 + g % 3, qchar(g), ANCHOR + g % 4, ANCHOR + g % 5))
    for p in range(P):
        rows[(p * 7) % S].append(row(1, 100 + 50 * p, 180 + 50 * p, 3 + p, "+-"[p % 2]))
    n_rows, n_triples = 3 + P, sum(runs) + P
    claims = dict(reduce="wave" if n_rows * 32 <= n_triples else "lane", reduce_margin=n_triples - 32 * n_rows, runs=sorted(set(runs) | ({1} if P else set())),
                  n_rows=n_rows, n_triples=n_triples, class2_char=qchar(S - 1), total_past_2_32=big)
    return Case("shared_S%d%s" % (S, tag), [Sample(g, r) for g, r in enumerate(rows)], claims)


def _filter_lane():
    k151 = (4_000_000_000, P32 + 5 - 4_000_000_000 - 1, 1)                      # the three samples' counts of key 151: 2^32 + 5 together
    def c0(k): return {0: 5, 299: 1, 150: 7, 151: k151[0]}.get(k, 10 + k % 9)
    def c1(k): return {299: 2, 151: k151[1]}.get(k, 10 + k % 5)
    s0 = [row(0, 1000 + 10 * k, 1100 + 10 * k, c0(k), "+-"[k % 2]) for k in range(300)]
    s1 = [row(0, 1000 + 10 * k, 1100 + 10 * k, c1(k), "+-"[k % 2], ANCHOR + 2, ANCHOR + 1) for k in range(300) if k % 2]
    s2 = [row(0, 1000 + 10 * k, 1100 + 10 * k, c, "+-"[k % 2]) for k, c in ((7, 3), (151, k151[2]))]
    filters = [dict(name="none", min_samples=1, min_total=0, n_kept=300),
               dict(name="last", min_samples=1, min_total=4, n_kept=299, last_dropped=True, first_dropped=False),
               dict(name="first", min_samples=2, min_total=0, n_kept=150, first_dropped=True, last_dropped=False, between=True),
               dict(name="exact", min_samples=1, min_total=7, n_kept=298, exact=True, first_dropped=True, last_dropped=True),
               dict(name="between", min_samples=1, min_total=8, n_kept=297, between=True),
               dict(name="every", min_samples=4, min_total=0, n_kept=0),
               dict(name="exact_past_2_32", min_samples=1, min_total=P32 + 5, n_kept=1, exact=True),
               dict(name="above", min_samples=1, min_total=P32 + 6, n_kept=0)]
    return Case("filter_lane", [Sample(0, s0), Sample(1, s1), Sample(2, s2)], dict(reduce="lane", n_rows=300, total_past_2_32=True), filters=filters)


def _filter_wave():
    S, runs = 40, (40, 33, 40, 39, 38)
    def count(j, g):
        return (1, 2, 110_000_000 if g < 39 else P32 + 5 - 39 * 110_000_000, 3, 4 if g == 0 else 1)[j]
    rows = [[row(0, 1000 + 100 * j, 1050 + 100 * j, count(j, g), "+", ANCHOR + g % 3, ANCHOR + g % 4) for j in range(5) if g < runs[j]] for g in range(S)]
    filters = [dict(name="none", min_samples=1, min_total=0, n_kept=5),
               dict(name="between", min_samples=34, min_total=0, n_kept=4, between=True, first_dropped=False, last_dropped=False),
               dict(name="last", min_samples=39, min_total=0, n_kept=3, last_dropped=True, first_dropped=False),
               dict(name="first_exact", min_samples=1, min_total=41, n_kept=4, first_dropped=True, last_dropped=False, exact=True),
               dict(name="every", min_samples=41, min_total=0, n_kept=0),
               dict(name="exact_past_2_32", min_samples=1, min_total=P32 + 5, n_kept=1, exact=True, first_dropped=True, last_dropped=True),
               dict(name="above", min_samples=1, min_total=P32 + 6, n_kept=0)]
    return Case("filter_wave", [Sample(g, r) for g, r in enumerate(rows)],
                dict(reduce="wave", reduce_margin=sum(runs) - 160, n_rows=5, total_past_2_32=True), filters=filters)


def _big_coords():
    """start and end at and above 2^31, a thick_end close to 2^32 and an intron longer than 2^31: the key sort and the site sorts take the
    coordinates as unsigned, and so does every difference."""
    H = 1 << 31
    a = [row(0, H - 100, H + 50, 3, "+"), row(0, H, H + 100, 4, "+"), row(0, H, H + 300, 5, "+"), row(0, 100, H + 100, 6, "+"),
         row(0, 4_294_967_000, 4_294_967_200, 7, "-", 9, 90), row(2, 2_999_999_000, 2_999_999_900, 1, "+")]
    b = [row(0, H + 5, 4_294_967_200, 2, "-", 30, 95), row(0, H, H + 100, 9, "+", 20, 20), row(0, 90, 190, 1, "+"), row(0, H - 100, H + 50, 1, "+", 12, 8)]
    return Case("big_coords", [Sample(0, a), Sample(1, b)], dict(coords_from_2_31=True, n_rows=8), cluster_kw=[dict(), dict(min_rows=2)],
                refine_kw=[dict(), dict(max_intron=H - 1)])                     # (one row's intron is 2^31 long)


# ---- cluster sums -------------------------------------------------------------------------------------------------------------------------
ZERO_ROWS = [("Z0", 100, 200, "zero"), ("Z0", 100, 300, "zero"), ("A", 1000, 1100, "ends"), ("A", 1000, 1200, "first_trip"), ("X", 2000, 2100, "full"),
             ("B", 3000, 3100, "last_trip"), ("B", 3000, 3200, "alternate"), ("Y", 4000, 4100, "full"), ("C", 5000, 5100, "zero"), ("C", 5000, 5200, "full"),
             ("Z1", 6000, 6100, "zero"), ("Z1", 6000, 6200, "zero")]


def _is_zero(pattern, g, S):
    """Sample g is lane g % 64 of trip g // 64 of a row's wave in k_cluster_expand<64>."""
    if pattern == "zero": return True
    if pattern == "full": return False
    if pattern == "ends": return g in (0, min(63, S - 1))
    if pattern == "first_trip": return g < 64
    if pattern == "alternate": return g % 2 == 0
    t0 = 64 * ((S - 1) // 64)                                                   # last_trip: the partial last trip, or the row's second half
    return g >= (t0 if t0 else S // 2)


def _zeros(S, lacking=None, tag=""):
    """Every sample holds every row, so absence is a ZERO COUNT.  Pairs of rows share a start (clusters Z0, A, B, C, Z1); X and Y are alone
    between them, have counts everywhere, and leave with min_rows = 2.  Z0 and Z1 are clusters without a run."""
    rows = [[] for _ in range(S)]
    for i, (_, start, end, pattern) in enumerate(ZERO_ROWS):
        for g in range(S):
            if lacking == (g, i):
                continue
            rows[g].append(row(0, start, end, 0 if _is_zero(pattern, g, S) else 1 + (g + 3 * i) % 7))
    n, nnz = len(ZERO_ROWS), len(ZERO_ROWS) * S - (1 if lacking else 0)
    claims = dict(expand="wave" if n * 32 <= nnz else "lane", expand_margin=nnz - 32 * n, n_rows=n, zeros_in_clustered_rows=True,
                  n_clusters={2: 5, 1: 7}, no_run_clusters={2: [0, 4], 1: [0, 6]}, dropped_between=True)
    return Case("zeros_S%d%s" % (S, tag), [Sample(g, r) for g, r in enumerate(rows)], claims, cluster_kw=[dict(min_rows=2), dict()],
                refine_kw=[dict(min_rows=2), dict(min_reads=1, min_rows=2), dict(min_reads=1)])


def _sums(R, big=False, zero_one=False, tag=""):
    """One cluster of R rows on a shared donor over three samples: three (cluster, sample) runs of R entries each."""
    rows = [[row(0, 1000, 2000 + 10 * i, 0 if zero_one and (g, i) == (2, 5) else 70_000_000 + i if big and g == 0 else 1 + (i + g) % 5) for i in range(R)]
            for g in range(3)]
    M = 3 * R - (1 if zero_one else 0)
    claims = dict(sum="wave" if 96 <= M else "lane", sum_margin=M - 96, cs_runs=sorted({R, R - 1} if zero_one else {R}), n_clusters={1: 1},
                  cs_total_past_2_32=big, n_rows=R)
    return Case("sums_R%d%s" % (R, tag), [Sample(g, r) for g, r in enumerate(rows)], claims, refine_kw=[dict(), dict(min_reads=1)])


def _width(C, zero):
    """C clusters of one row each over two samples; the clusters in `zero` count nothing anywhere and have no run."""
    rows = [[row(0, 1000 + 100 * c, 1050 + 100 * c, 0 if c in zero else 1 + (c + g) % 4) for c in range(C)] for g in range(2)]
    return Case("width_C%d" % C, [Sample(g, r) for g, r in enumerate(rows)], dict(n_clusters={1: C}, no_run_clusters={1: sorted(zero)}, n_rows=C))


def _many_samples(S):
    """S samples over four rows in two clusters: the pair sort's sample key is bitlen(S - 1) wide."""
    site = [(1000, 1100), (1000, 1200), (3000, 3100), (3000, 3200)]
    rows = [[row(0, site[j][0], site[j][1], 1 + g % 5) for j in sorted({g % 4, (g + 1) % 4})] for g in range(S)]
    return Case("samples_%d" % S, [Sample(g, r) for g, r in enumerate(rows)], dict(n_clusters={1: 2}, n_rows=4, last_sample_counts=S - 1))


ACCUMULATE = ([_triples(n, 1 if n == 513 else 0) for n in (1, 63, 64, 65, 255, 256, 257, 513)] + [_waves()] +
              [_shared(32, (32, 32, 32), 0, tag="_at"), _shared(32, (32, 32, 31), 0, tag="_below"), _shared(33, (33, 33, 33), 0),
               _shared(63, (63, 63, 63), 3, tag="_at"), _shared(63, (63, 63, 62), 3, tag="_below"), _shared(64, (64, 64, 64), 3),
               _shared(65, (65, 65, 64), 3), _shared(129, (129, 129, 65), 7, big=True)] + [_big_coords()])
FILTERS = [_filter_lane(), _filter_wave()]
ZEROS = [_zeros(S) for S in (8, 32, 64, 65, 129, 200)] + [_zeros(32, lacking=(5, 4), tag="_below")]
SUMS = [_sums(R, big=R == 65) for R in (1, 7, 8, 9, 17, 31, 32, 33, 63, 64, 65, 129)] + [_sums(32, zero_one=True, tag="_below")]
WIDTHS = [_width(1, {0}), _width(2, {0}), _width(255, {0, 127, 254}), _width(256, {0, 128, 255}), _width(257, {0, 128, 256})]
MANY = [_many_samples(256), _many_samples(257)]
CLUSTER = ZEROS + SUMS + WIDTHS + MANY
ALL = ACCUMULATE + FILTERS + CLUSTER
SECOND_FINISH = [("shared_S65", 62), ("shared_S129", 126)]                     # (case, samples in front of the first finish): three more, a second finish


def by_name(name):
    return [c for c in ALL if c.name == name][0]


# ---- the claims, proven from a matrix (and the clusters of it) alone --------------------------------------------------------------------
def _get(cl, k):
    return np.asarray(cl[k] if isinstance(cl, dict) else getattr(cl, k))


def entries(m, cl):
    """(cluster, sample, count) of every count entry of a clustered row."""
    n_per = np.diff(np.asarray(m.row_begin).astype(np.int64))
    c = _get(cl, "cluster").astype(np.int64)[np.repeat(np.arange(int(m.n)), n_per)]
    take = c != NO
    return c[take], np.asarray(m.col_sample).astype(np.int64)[take], np.asarray(m.val_count).astype(np.int64)[take]


def check(case, m):
    """The claims about the matrix: m is the case's unfiltered matrix, the restatement's or the device's."""
    cl = case.claims
    n, T = int(m.n), int(m.n_triples)
    n_with, total, row_begin = np.asarray(m.n_with).astype(np.int64), np.asarray(m.total), np.asarray(m.row_begin).astype(np.int64)
    nnz = int(row_begin[-1])
    assert nnz == T                                                            # no filter: every triple is an entry
    if "n_rows" in cl: assert n == cl["n_rows"]
    if "n_triples" in cl: assert T == cl["n_triples"]
    if "reduce" in cl: assert ("wave" if n * 32 <= T else "lane") == cl["reduce"]
    if "reduce_margin" in cl: assert T - 32 * n == cl["reduce_margin"]
    if "expand" in cl: assert ("wave" if n * 32 <= nnz else "lane") == cl["expand"]
    if "expand_margin" in cl: assert nnz - 32 * n == cl["expand_margin"]
    if "runs" in cl: assert set(cl["runs"]) <= set(n_with.tolist())
    if "last_is_head" in cl: assert (n_with[-1] == 1) == cl["last_is_head"]
    for p in cl.get("run_of_two_at", ()): assert n_with[np.flatnonzero(row_begin[:-1] == p)].tolist() == [2]
    if cl.get("total_past_2_32"): assert int(total.max()) > P32
    if "class2_char" in cl: assert [s for s in m.strand if s not in (b"+", b"-")] == [cl["class2_char"].encode()]
    if cl.get("coords_from_2_31"): assert (np.asarray(m.start).astype(np.int64) >= 1 << 31).sum() >= 3 and (np.asarray(m.start).astype(np.int64) < 1 << 31).sum() >= 3
    if "wave_masks" in cl: assert set(cl["wave_masks"]) <= set(wave_masks(case.samples[0]))
    if "sample_without_triples" in cl: assert cl["sample_without_triples"] not in np.asarray(m.col_sample).tolist() and m.n_samples == len(case.samples)
    if "last_sample_counts" in cl: assert int(np.asarray(m.col_sample).max()) == cl["last_sample_counts"] == m.n_samples - 1


def check_clusters(case, m, cl, min_rows):
    """The claims about the clusters `cl` (a CohortClusters or a restatement's dict) of the case's unfiltered matrix m with this min_rows."""
    claims = case.claims
    cluster, cs_begin = _get(cl, "cluster").astype(np.int64), _get(cl, "cs_begin").astype(np.int64)
    C = len(cs_begin) - 1
    c, s, v = entries(m, cl)
    M, n_cs = int((v != 0).sum()), len(_get(cl, "cs_sample"))
    if "n_clusters" in claims and min_rows in claims["n_clusters"]: assert C == claims["n_clusters"][min_rows]
    if claims.get("zeros_in_clustered_rows"): assert (v == 0).sum() > 0 and M > 0
    if "no_run_clusters" in claims and min_rows in claims["no_run_clusters"]:
        assert np.flatnonzero(np.diff(cs_begin) == 0).tolist() == claims["no_run_clusters"][min_rows]
    if "sum" in claims: assert ("wave" if n_cs * 32 <= M else "lane") == claims["sum"]
    if "sum_margin" in claims: assert M - 32 * n_cs == claims["sum_margin"]
    if "cs_runs" in claims: assert sorted(set(np.unique((c * m.n_samples + s)[v != 0], return_counts=True)[1].tolist())) == claims["cs_runs"]
    if claims.get("cs_total_past_2_32"): assert int(_get(cl, "cs_total").max()) > P32
    if claims.get("dropped_between") and min_rows == 2:
        out = np.flatnonzero(cluster == NO)
        inner = [i for i in out if 0 < i < len(cluster) - 1 and cluster[i - 1] != NO and cluster[i + 1] != NO]
        assert inner and all((np.asarray(m.val_count)[int(m.row_begin[i]):int(m.row_begin[i + 1])] != 0).all() for i in inner)


def check_filter(m, f):
    """The claims of the filter pair f, from the unfiltered matrix m."""
    kept = (np.asarray(m.n_with).astype(np.int64) >= f["min_samples"]) & (np.asarray(m.total).astype(np.uint64) >= np.uint64(f["min_total"]))
    assert int(kept.sum()) == f["n_kept"]
    if "first_dropped" in f: assert (not kept[0]) == f["first_dropped"]
    if "last_dropped" in f: assert (not kept[-1]) == f["last_dropped"]
    if f.get("exact"): assert (np.asarray(m.total)[kept].astype(np.uint64) == np.uint64(f["min_total"])).sum() == 1
    if f.get("between"): assert any(kept[i - 1] and not kept[i] and kept[i + 1] for i in range(1, len(kept) - 1))
