"""Plain numpy references of the stages behind the DEFLATE launch -- exclusive scan, stable multi-word sort, the group-by of junction events
with first-seen naming and output order -- and a generator of keys that collide in k_preagg's LDS table (TEST INFRASTRUCTURE ONLY; nothing here
imports the product).  tests/test_stage_reference.py pins group_by to the oracle's BED12; tests/test_gpu_stage_kernels.py holds the kernels to these."""
import numpy as np

ROW_COLUMNS = ("tid", "start", "end", "ts", "te", "count", "name_rank", "first_seen", "last_seen", "strand")      # k_rows_out's ten columns


def excl_scan(a):
    """-> (exclusive prefix sums, total), both in uint64"""
    inc = np.cumsum(np.asarray(a, dtype=np.uint64), dtype=np.uint64)
    out = np.zeros(len(inc), dtype=np.uint64)
    out[1:] = inc[:-1]
    return out, (int(inc[-1]) if len(inc) else 0)


def stable_sort(words, nbits):
    """The positions 0..n-1 in stable order of the key whose word k (k = 0 least significant) is the low nbits[k] bits of words[k].  Unique, so a
    sort under test is compared with the whole permutation."""
    masked = [np.asarray(w, dtype=np.uint64) & np.uint64((1 << b) - 1) for w, b in zip(words, nbits)]
    if sum(nbits) <= 64:                                    # one packed key: several times cheaper than a lexsort of the columns
        key = np.zeros(len(masked[0]), dtype=np.uint64)
        shift = 0
        for m, b in zip(masked, nbits):
            key |= m << np.uint64(shift)
            shift += b
        return np.argsort(key, kind="stable").astype(np.uint32)
    return np.lexsort(tuple(masked)).astype(np.uint32)      # (the last key is the primary one; lexsort is stable)


def group_by(tid, start, ilen_cls, ts, te, strand, rank_of_group):
    """Junction events in file order -> (rows, row_of_event).  The contract of JunctionsExtractor::add_junction and its output order
    (junctions_extractor.cc:152-157, :233; junctions_extractor.h:117-140): one row per key (tid, start, ilen_cls = length << 2 | strand class) with the
    number of its events, the smallest thick_start, the largest thick_end, its first and last event, the strand byte of the last event, end = start +
    length and a 1-based name rank in order of first events; rows ordered by (rank_of_group[tid], thick_start, thick_end, name rank).  rows: a dict of
    the ten uint32 columns ROW_COLUMNS; row_of_event[i] = the output row event i went into."""
    tid, start, ilen_cls, ts, te = [np.asarray(a, dtype=np.uint32) for a in (tid, start, ilen_cls, ts, te)]
    strand = np.asarray(strand, dtype=np.uint8)
    n = len(tid)
    if n == 0:
        return {k: np.zeros(0, dtype=np.uint32) for k in ROW_COLUMNS}, np.zeros(0, dtype=np.uint32)
    # two words of the key at a time: (tid, start) -> a dense id, then (id, ilen_cls)
    _, id1 = np.unique(tid.astype(np.uint64) << np.uint64(32) | start.astype(np.uint64), return_inverse=True)
    _, first, inv, count = np.unique(id1.astype(np.uint64).reshape(-1) << np.uint64(32) | ilen_cls.astype(np.uint64),
                                     return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    u = len(first)
    at = np.arange(n, dtype=np.int64)
    last = np.zeros(u, dtype=np.int64)
    np.maximum.at(last, inv, at)
    ts_min = np.full(u, 0xffffffff, dtype=np.uint32)
    np.minimum.at(ts_min, inv, ts)
    te_max = np.zeros(u, dtype=np.uint32)
    np.maximum.at(te_max, inv, te)
    name_rank = np.empty(u, dtype=np.uint32)
    name_rank[np.argsort(first, kind="stable")] = np.arange(1, u + 1, dtype=np.uint32)
    k_tid, k_start, k_ilen = tid[first], start[first], ilen_cls[first]
    rank = np.asarray(rank_of_group, dtype=np.uint32)[k_tid]
    # (rank, ts, te, name rank), least significant pair first; two packed sorts are several times cheaper than a lexsort of four columns
    u64 = lambda hi, lo: hi.astype(np.uint64) << np.uint64(32) | lo.astype(np.uint64)
    order = np.argsort(u64(te_max, name_rank), kind="stable")
    order = order[np.argsort(u64(rank, ts_min)[order], kind="stable")]
    rows = {"tid": k_tid, "start": k_start, "end": k_start + (k_ilen >> np.uint32(2)), "ts": ts_min, "te": te_max, "count": count.astype(np.uint32),
            "name_rank": name_rank, "first_seen": first.astype(np.uint32), "last_seen": last.astype(np.uint32), "strand": strand[last].astype(np.uint32)}
    rows = {k: np.ascontiguousarray(v[order], dtype=np.uint32) for k, v in rows.items()}
    pos = np.empty(u, dtype=np.uint32)
    pos[order] = np.arange(u, dtype=np.uint32)
    return rows, pos[inv]


def preagg_slot(tid, start, ilen_cls):
    """The slot of k_preagg's LDS table (2048 slots for its 1024-event tiles) a key is first tried in.  RESTATED from reduce_kernels.hip (k_preagg): should
    the kernel's hash change, colliding_keys still returns distinct plausible keys -- they just no longer collide, and nothing fails."""
    h = (np.asarray(start, dtype=np.uint32) * np.uint32(0x9E3779B1)) ^ (np.asarray(ilen_cls, dtype=np.uint32) * np.uint32(0x85EBCA6B)) ^ \
        (np.asarray(tid, dtype=np.uint32) * np.uint32(0xC2B2AE35))
    return (h ^ (h >> np.uint32(15))) & np.uint32(2047)


def colliding_keys(slot, m, rng):
    """m distinct plausible keys (tid < 25, start < 2^29, intron length 70..500000, strand class 0..2) that all start their probe in `slot`
    -> (tid, start, ilen_cls), uint32 each"""
    got, seen = [], set()
    while len(got) < m:
        k = 1 << 21
        tid = rng.integers(0, 25, k, dtype=np.uint32)
        start = rng.integers(0, 1 << 29, k, dtype=np.uint32)
        ilen_cls = rng.integers(70, 500001, k, dtype=np.uint32) << np.uint32(2) | rng.integers(0, 3, k, dtype=np.uint32)
        for i in np.nonzero(preagg_slot(tid, start, ilen_cls) == slot)[0]:
            key = (int(tid[i]), int(start[i]), int(ilen_cls[i]))
            if key not in seen and len(got) < m:
                seen.add(key)
                got.append(key)
    a = np.array(got, dtype=np.uint32).reshape(m, 3)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()
