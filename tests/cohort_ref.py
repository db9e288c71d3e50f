"""The EXPECTATION of the cohort junction-by-sample matrix (tests/test_cohort_edge_cases_host.py, tests/test_gpu_cohort_edges.py,
tests/test_gpu_cohort.py): the contract of rgx_cohort_* in include/regtools_amd.h restated with numpy -- which rows take part, contigs matched by
name in order of first appearance, the key, the per-row reductions, the strand character, both filters and the CSR image of the kept rows.
Coordinates are unsigned 32-bit numbers held in int64, so differences wrap as the header says they do.  It shares no code with the product;
tests/cluster_ref.py and tests/refine_ref.py read its result as they read a CohortMatrix."""
import numpy as np

M32 = 0xffffffff


class Matrix(object):
    """The attributes of regtools_amd.cohort.CohortMatrix that the restatements and the tests read."""


def u32(a):
    return np.asarray(a).astype(np.int64) & M32


def strand_class(chars):
    chars = np.asarray(chars)
    return np.where(chars == ord("+"), 0, np.where(chars == ord("-"), 1, 2))


def last_sample_strand(group, sample, chars, n_groups):
    """Per group 0 .. n_groups - 1 (every one has a member): the strand character of its member with the highest sample number."""
    group, sample, chars = np.asarray(group, np.int64), np.asarray(sample, np.int64), np.asarray(chars)
    best = np.full(n_groups, -1, np.int64)
    np.maximum.at(best, group, sample)
    out = np.zeros(n_groups, np.uint8)
    decides = sample == best[group]
    out[group[decides]] = chars[decides]
    return out.view("S1")


def anchored(s):
    """Which rows of the sample s have both anchors: start - thick_start >= min_anchor and thick_end - end >= min_anchor, unsigned 32-bit."""
    return (((u32(s.start) - u32(s.thick_start)) & M32) >= s.min_anchor) & (((u32(s.thick_end) - u32(s.end)) & M32) >= s.min_anchor)


def matrix(samples, names, only_anchored=True, min_samples=1, min_total=1):
    """samples: objects with contigs = [(name, length)] in the sample's header order, min_anchor, and per row tid (into contigs), start, end,
    thick_start, thick_end, count, strand (character codes)."""
    ref_name, ref_len = [], []
    cols = []
    for g, s in enumerate(samples):
        for nm, ln in s.contigs:
            if nm in ref_name:
                assert ref_len[ref_name.index(nm)] == ln, "one name with two lengths is an error of the contract, not a matrix"
            else:
                ref_name.append(nm); ref_len.append(ln)
        to_cohort = np.array([ref_name.index(nm) for nm, _ in s.contigs], np.int64)
        keep = anchored(s) if only_anchored else np.ones(len(s.start), bool)
        tid = to_cohort[np.asarray(s.tid, np.int64)] if len(s.start) else np.zeros(0, np.int64)
        cols.append([c[keep] for c in (tid, u32(s.start), u32(s.end), u32(s.thick_start), u32(s.thick_end), u32(s.count), u32(s.strand),
                                       np.full(len(s.start), g, np.int64))])
    if cols:
        tid, start, end, ts, te, count, chars, sample = [np.concatenate(c) for c in zip(*cols)]
    else:
        tid = start = end = ts = te = count = chars = sample = np.zeros(0, np.int64)
    cls = strand_class(chars)
    order = np.lexsort((sample, cls, end, start, tid))
    tid, start, end, ts, te, count, chars, sample, cls = [c[order] for c in (tid, start, end, ts, te, count, chars, sample, cls)]
    T = len(tid)
    head = np.ones(T, bool)
    if T:
        head[1:] = (tid[1:] != tid[:-1]) | (start[1:] != start[:-1]) | (end[1:] != end[:-1]) | (cls[1:] != cls[:-1])
    group = np.cumsum(head) - 1
    n = int(head.sum())
    assert len(set(zip(group.tolist(), sample.tolist()))) == T, "a sample has at most one row per key"
    n_with = np.bincount(group, minlength=n).astype(np.int64)
    total = np.zeros(n, np.uint64); np.add.at(total, group, count.astype(np.uint64))
    lo = np.full(n, M32, np.int64); np.minimum.at(lo, group, ts)
    hi = np.zeros(n, np.int64); np.maximum.at(hi, group, te)
    strand = last_sample_strand(group, sample, chars, n)
    kept = (n_with >= min_samples) & (total >= np.uint64(min_total))
    of_kept = kept[group] if T else np.zeros(0, bool)
    m = Matrix()
    m.unfiltered_rows, m.kept = n, kept                    # (not part of the product's matrix: what the tests' conditions are computed from)
    m.n, m.n_samples, m.n_triples = int(kept.sum()), len(samples), T
    m.ref_name, m.ref_len, m.sample_name = ref_name, ref_len, list(names)
    first = np.flatnonzero(head)
    m.tid, m.start, m.end = tid[first][kept], start[first][kept], end[first][kept]
    m.thick_start, m.thick_end, m.strand = lo[kept], hi[kept], strand[kept]
    m.n_with, m.total = n_with[kept], total[kept]
    m.row_begin = np.concatenate([[0], np.cumsum(n_with[kept])]).astype(np.int64)
    m.col_sample, m.val_count = sample[of_kept], count[of_kept]
    return m


FIELDS = ("tid", "start", "end", "thick_start", "thick_end", "n_with", "total", "row_begin", "col_sample", "val_count")


def same(got, want):
    """got: a regtools_amd.cohort.CohortMatrix; want: matrix() of the same samples.  Every array and count, exactly."""
    assert (got.n, got.n_samples, got.n_triples) == (want.n, want.n_samples, want.n_triples)
    assert (got.ref_name, got.ref_len, got.sample_name) == (want.ref_name, want.ref_len, want.sample_name)
    for k in FIELDS:
        a, b = np.asarray(getattr(got, k)), np.asarray(getattr(want, k))
        assert a.shape == b.shape and np.array_equal(a.astype(np.uint64), b.astype(np.uint64)), k
    assert got.strand.shape == want.strand.shape and np.array_equal(got.strand, want.strand), "strand"
