"""The EXPECTATION of the cohort's intron clusters (tests/test_cohort_clusters_host.py, tests/test_gpu_cohort_clusters.py): the contract of
include/regtools_amd.h restated with a plain Python union-find with path compression over (tid, class, start) and (tid, class, end) dictionaries,
numpy for the totals, and the perind.counts-style text written here.  It shares no code with the product and reads a matrix only through the
numpy views of regtools_amd.cohort.CohortMatrix (or any object with the same attributes)."""
import numpy as np

NO_CLUSTER = 0xffffffff


def cls_of(strand):
    return 0 if strand == b"+" else 1 if strand == b"-" else 2


def components(n, edges_a, edges_b):
    """label[v] = smallest vertex of v's component (union-find, path compression)."""
    parent = list(range(n))

    def find(v):
        r = v
        while parent[r] != r:
            r = parent[r]
        while parent[v] != r:
            parent[v], v = r, parent[v]
        return r
    for a, b in zip(edges_a, edges_b):
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(v) for v in range(n)], dtype=np.int64)


def row_labels(tid, start, end, strand):
    """Rows are linked when tid and class agree and start or end does: label[i] = lowest row of i's component."""
    n = len(tid)
    first_a, first_b, ea, eb = {}, {}, [], []
    cls = [cls_of(s) for s in strand]
    for i in range(n):
        ka, kb = (int(tid[i]), cls[i], int(start[i])), (int(tid[i]), cls[i], int(end[i]))
        for key, first in ((ka, first_a), (kb, first_b)):
            if key in first:
                ea.append(first[key]); eb.append(i)
            else:
                first[key] = i
    return components(n, ea, eb)


def clusters(m, min_rows=1, min_total=0):
    """dict of every array of rgx_cohort_clusters plus n_clusters and n_components, for the matrix m."""
    n = int(m.n)
    label = row_labels(m.tid, m.start, m.end, m.strand)
    rows_of = np.bincount(label, minlength=n) if n else np.zeros(0, np.int64)
    total_of = np.zeros(n, np.uint64)
    np.add.at(total_of, label, m.total.astype(np.uint64))
    roots = np.flatnonzero(label == np.arange(n))
    kept = np.array([r for r in roots if rows_of[r] >= min_rows and int(total_of[r]) >= min_total], dtype=np.int64)
    number = np.full(n, NO_CLUSTER, np.int64)
    number[kept] = np.arange(len(kept))
    cluster = number[label] if n else np.zeros(0, np.int64)
    C = len(kept)
    clustered = np.flatnonzero(cluster != NO_CLUSTER)
    cl_row = clustered[np.argsort(cluster[clustered], kind="stable")]
    cl_begin = np.concatenate([[0], np.cumsum(rows_of[kept])]).astype(np.int64)
    # per (cluster, sample): the sum of the counts, the pairs whose sum is not zero
    row_of_entry = np.repeat(np.arange(n), np.diff(m.row_begin).astype(np.int64))
    c_of_entry = cluster[row_of_entry] if n else np.zeros(0, np.int64)
    take = c_of_entry != NO_CLUSTER
    S = max(int(m.n_samples), 1)
    pair = c_of_entry[take] * S + m.col_sample[take].astype(np.int64)
    uniq, inv = np.unique(pair, return_inverse=True)
    sums = np.zeros(len(uniq), np.uint64)
    np.add.at(sums, inv, m.val_count[take].astype(np.uint64))
    nz = sums != 0
    uniq, sums = uniq[nz], sums[nz]
    cs_begin = np.searchsorted(uniq // S, np.arange(C + 1)).astype(np.int64)
    return dict(n_clusters=C, n_components=len(roots), cluster=cluster, cl_begin=cl_begin, cl_row=cl_row, cl_total=total_of[kept],
                cs_begin=cs_begin, cs_sample=uniq % S, cs_total=sums)


def counts_text(m, want):
    """The perind.counts-style text of the clusters `want` (as clusters() returns them) of the matrix m."""
    n, S, C = int(m.n), int(m.n_samples), want["n_clusters"]
    head = "chrom" + "".join(" " + s for s in m.sample_name) + "\n"
    rows = np.flatnonzero(want["cluster"] != NO_CLUSTER) if n else np.zeros(0, np.int64)
    if not len(rows):
        return head.encode()
    num = np.zeros((n, S), np.uint64)
    num[np.repeat(np.arange(n), np.diff(m.row_begin).astype(np.int64)), m.col_sample] = m.val_count
    den = np.zeros((C, S), np.uint64)
    den[np.repeat(np.arange(C), np.diff(want["cs_begin"])), want["cs_sample"]] = want["cs_total"]
    fields = np.char.add(np.char.add(num[rows].astype("U20"), "/"), den[want["cluster"][rows]].astype("U20"))
    out = [head]
    for k, i in enumerate(rows):
        tag = ("+", "-", "NA")[cls_of(m.strand[i])]
        out.append("%s:%d:%d:clu_%d_%s %s\n" % (m.ref_name[int(m.tid[i])], m.start[i], m.end[i], int(want["cluster"][i]) + 1, tag, " ".join(fields[k])) if S
                   else "%s:%d:%d:clu_%d_%s\n" % (m.ref_name[int(m.tid[i])], m.start[i], m.end[i], int(want["cluster"][i]) + 1, tag))
    return "".join(out).encode()


def same(got, want):
    """got: a regtools_amd.cohort.CohortClusters; want: clusters() of the same matrix.  Every array, exactly."""
    assert (got.n_clusters, got.n_components) == (want["n_clusters"], want["n_components"])
    for k in ("cluster", "cl_begin", "cl_row", "cl_total", "cs_begin", "cs_sample", "cs_total"):
        a, b = np.asarray(getattr(got, k)), np.asarray(want[k])
        assert a.shape == b.shape and np.array_equal(a.astype(np.uint64), b.astype(np.uint64)), k


def same_clusters(a, b):
    """Two CohortClusters (the device's and the twin's), every array and count."""
    assert (a.n_rows, a.n_clusters, a.n_components) == (b.n_rows, b.n_clusters, b.n_components)
    for k in ("cluster", "cl_begin", "cl_row", "cl_total", "cs_begin", "cs_sample", "cs_total"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
