"""The EXPECTATION of the cohort's refined intron clusters (tests/test_cohort_refine_host.py, tests/test_gpu_cohort_refine.py): the contract of
rgx_cohort_refine in include/regtools_amd.h restated in Python.  The link rule and the union-find are tests/cluster_ref.py's; the ratio test is
done on Python integers (no width to overflow); the removal is ITERATED until a round removes nothing, as LeafCutter's recursion would, and the
restatement asserts that the loop body ran at most twice -- the product does one pass, and this is where that is checked.  It shares no code with
the product and reads a matrix only through the numpy views of regtools_amd.cohort.CohortMatrix."""
import numpy as np

import cluster_ref

NO_CLUSTER = cluster_ref.NO_CLUSTER


def labels(m, alive):
    """label[i] = lowest row of i's component among the alive rows; a row that is not alive is alone."""
    n = int(m.n)
    label = np.arange(n, dtype=np.int64)
    sub = np.flatnonzero(alive)
    if len(sub):
        label[sub] = sub[cluster_ref.row_labels(m.tid[sub], m.start[sub], m.end[sub], m.strand[sub])]
    return label


def removal(m, max_intron=0, min_reads=0, min_ratio=(0, 1)):
    """dict(alive, label, n_ineligible, n_weak, removed_per_round, by_reads, by_ratio, stage1_label): which rows stay, and their components."""
    n = int(m.n)
    num, den = int(min_ratio[0]), int(min_ratio[1])
    total = [int(x) for x in m.total]
    length = m.end.astype(np.int64) - m.start.astype(np.int64)
    alive = np.ones(n, bool) if max_intron == 0 else length <= max_intron
    n_ineligible = n - int(alive.sum())
    removed, by_reads, by_ratio, stage1 = [], 0, 0, None
    while True:
        label = labels(m, alive)
        if stage1 is None:
            stage1 = label
        T = {}
        for i in np.flatnonzero(alive):
            T[int(label[i])] = T.get(int(label[i]), 0) + total[i]
        weak = []
        for i in np.flatnonzero(alive):
            few, small = total[i] < min_reads, total[i] * den < num * T[int(label[i])]
            if few or small:
                weak.append(i)
                if len(removed) == 0:
                    by_reads += few and not small
                    by_ratio += small and not few
        removed.append(len(weak))
        if not weak:
            break
        alive = alive.copy()
        alive[weak] = False
    assert len(removed) <= 2, removed                      # one removal is the whole refinement: the second round never removes anything
    return dict(alive=alive, label=label, n_ineligible=n_ineligible, n_weak=sum(removed), removed_per_round=removed, by_reads=int(by_reads),
                by_ratio=int(by_ratio), stage1_label=stage1, stage1_alive=(np.ones(n, bool) if max_intron == 0 else length <= max_intron))


def clusters_of(m, rem, min_rows=1, min_total=0):
    """Every array of rgx_cohort_clusters plus the counts, from a removal() of the matrix m."""
    n = int(m.n)
    alive, label = rem["alive"], rem["label"]
    rows_of = np.bincount(label[alive], minlength=n) if n else np.zeros(0, np.int64)
    total_of = np.zeros(n, np.uint64)
    np.add.at(total_of, label[alive], m.total[alive].astype(np.uint64))
    roots = np.flatnonzero(alive & (label == np.arange(n)))
    kept = np.array([r for r in roots if rows_of[r] >= min_rows and int(total_of[r]) >= min_total], dtype=np.int64)
    number = np.full(n, NO_CLUSTER, np.int64)
    number[kept] = np.arange(len(kept))
    cluster = np.where(alive, number[label], NO_CLUSTER) if n else np.zeros(0, np.int64)
    C = len(kept)
    clustered = np.flatnonzero(cluster != NO_CLUSTER)
    cl_row = clustered[np.argsort(cluster[clustered], kind="stable")]
    cl_begin = np.concatenate([[0], np.cumsum(rows_of[kept])]).astype(np.int64)
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
    return dict(n_clusters=C, n_components=len(roots), n_ineligible=rem["n_ineligible"], n_weak=rem["n_weak"], cluster=cluster, cl_begin=cl_begin,
                cl_row=cl_row, cl_total=total_of[kept], cs_begin=cs_begin, cs_sample=uniq % S, cs_total=sums)


def refine(m, max_intron=0, min_reads=0, min_ratio=(0, 1), min_rows=1, min_total=0):
    return clusters_of(m, removal(m, max_intron, min_reads, min_ratio), min_rows, min_total)


def counts_text(m, want):
    return cluster_ref.counts_text(m, want)


def same(got, want):
    """got: a CohortClusters from refine / refine_host; want: refine() of the same matrix.  Every array and count, exactly."""
    assert (got.n_ineligible, got.n_weak) == (want["n_ineligible"], want["n_weak"])
    cluster_ref.same(got, want)


def same_clusters(a, b):
    """Two CohortClusters, every array and count, the two removal counts included."""
    assert (a.n_ineligible, a.n_weak) == (b.n_ineligible, b.n_weak)
    cluster_ref.same_clusters(a, b)
