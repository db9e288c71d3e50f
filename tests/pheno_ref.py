"""An independent restatement of the phenotype table's contract (rgx_cohort_phenotypes in include/regtools_amd.h) in numpy, for
tests/test_cohort_pheno_host.py and tests/test_gpu_cohort_pheno.py.  It shares no code with the product: dense tables instead of CSR lookups,
the contract's partial sums written as loops over float64 scalars (`ordered_sum`; `row_stats` runs the same additions a column of partials at a
time, so that 200,000 rows take a second, and is checked against the scalar loops bit for bit), ranks from scipy.stats.rankdata and quantiles from
scipy.stats.norm.ppf."""
import math

import numpy as np

NO = 0xffffffff
PARTIALS = 64


def dense_num(m):
    """n x S: the rows' counts, 0 where the CSR has no entry."""
    d = np.zeros((m.n, m.n_samples), np.uint64)
    rows = np.repeat(np.arange(m.n), np.diff(m.row_begin).astype(np.int64))
    d[rows, m.col_sample] = m.val_count
    return d


def dense_den(cl, n_samples):
    """C x S: the clusters' reads per sample, 0 where the CSR has no entry."""
    d = np.zeros((cl.n_clusters, n_samples), np.uint64)
    ks = np.repeat(np.arange(cl.n_clusters), np.diff(cl.cs_begin).astype(np.int64))
    d[ks, cl.cs_sample] = cl.cs_total
    return d


def ordered_sum(values, present):
    """The contract's sum, as written: 64 partials, sample s to partial s % 64 in ascending s, then halved from 32 down to 1."""
    P = [np.float64(0.0)] * PARTIALS
    for s in range(len(values)):
        if present[s]:
            P[s % PARTIALS] = P[s % PARTIALS] + np.float64(values[s])
    off = PARTIALS // 2
    while off:
        for l in range(off):
            P[l] = P[l] + P[l + off]
        off //= 2
    return P[0]


def row_stats_scalar(num, den):
    """(n_na, mean, sd) of one row from its S counts and its cluster's S denominators, with scalar float64 arithmetic only."""
    S = len(num)
    present = [int(d) > 0 for d in den]
    x = [(np.float64(int(a)) + np.float64(0.5)) / (np.float64(int(b)) + np.float64(0.5)) if p else None for a, b, p in zip(num, den, present)]
    n_na = S - sum(present)
    if n_na == S:
        return n_na, np.float64(0.0), np.float64(0.0)
    mean = ordered_sum(x, present) / np.float64(S - n_na)
    sq = [None if v is None else (v - mean) * (v - mean) for v in x]
    return n_na, mean, np.float64(math.sqrt(ordered_sum(sq, present) / np.float64(S)))


def _ordered_sums(values, present):
    """ordered_sum for every row of an R x S table at once: the same additions in the same order (adding +0.0 for an absent entry is exact, the
    partials never being negative)."""
    R, S = values.shape
    P = np.zeros((R, PARTIALS), np.float64)
    v = np.where(present, values, 0.0)
    for s in range(S):
        P[:, s % PARTIALS] = P[:, s % PARTIALS] + v[:, s]
    off = PARTIALS // 2
    while off:
        P[:, :off] = P[:, :off] + P[:, off:2 * off]
        off //= 2
    return P[:, 0].copy()


def phenotypes(m, cl, max_missing=(4, 10), min_sd=0.005):
    """The contract on a CohortMatrix and its CohortClusters (or anything with their arrays): a dict of row, n_na, mean, sd, rank2 (K x S), z
    (K x S, the standardised entries) and the counts."""
    from scipy.stats import rankdata
    S = m.n_samples
    na_num, na_den = max_missing
    cluster = np.asarray(cl.cluster, np.uint32)
    cand = np.flatnonzero(cluster != NO)
    out = dict(n_clustered=len(cand), n_samples=S)
    if len(cand) == 0 or S == 0:
        out.update(row=np.zeros(0, np.uint32), n_na=np.zeros(0, np.uint32), mean=np.zeros(0), sd=np.zeros(0), rank2=np.zeros((0, S), np.uint32),
                   z=np.zeros((0, S)), n_drop_na=len(cand), n_drop_sd=0)
        return out
    num = dense_num(m)[cand]
    den = dense_den(cl, S)[cluster[cand]]
    present = den > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (num.astype(np.float64) + 0.5) / (den.astype(np.float64) + 0.5)
        n_na = (S - present.sum(axis=1)).astype(np.int64)
        mean = _ordered_sums(x, present) / (S - n_na).astype(np.float64)
        d = x - mean[:, None]
        sd = np.sqrt(_ordered_sums(d * d, present) / np.float64(S))
    drop_na = (n_na == S) | (n_na * na_den > S * na_num)                      # (Python-sized integers are not needed: both sides are below 2^63)
    flat = ~drop_na & (~(sd > 0) | (sd < min_sd))
    kept = ~drop_na & ~flat
    K = int(kept.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(present[kept], (x[kept] - mean[kept][:, None]) / sd[kept][:, None], 0.0)
    rank2 = np.zeros((K, S), np.uint32)
    for s in range(S):
        r2 = rankdata(z[:, s], method="average") * 2
        assert np.array_equal(r2, np.round(r2))
        rank2[:, s] = r2.astype(np.uint32)
    out.update(row=cand[kept].astype(np.uint32), n_na=n_na[kept].astype(np.uint32), mean=mean[kept], sd=sd[kept], rank2=rank2, z=z,
               n_drop_na=int(drop_na.sum()), n_drop_sd=int(flat.sum()),
               all_mean=mean, all_sd=sd, all_n_na=n_na, all_num=num, all_den=den)
    return out


def quantiles(rank2, K):
    from scipy.stats import norm
    return norm.ppf(np.asarray(rank2, np.float64) / (2.0 * (K + 1)))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def same(ph, want):
    """ph: a CohortPhenotypes; want: phenotypes()'s dict.  Integers exactly, mean and sd as bit patterns."""
    assert (ph.n_rows, ph.n_samples, ph.n_clustered, ph.n_drop_na, ph.n_drop_sd) == (
        len(want["row"]), want["n_samples"], want["n_clustered"], want["n_drop_na"], want["n_drop_sd"])
    assert np.array_equal(ph.row, want["row"]) and np.array_equal(ph.n_na, want["n_na"])
    assert np.array_equal(bits(ph.mean), bits(want["mean"])), "mean differs in %d rows" % (bits(ph.mean) != bits(want["mean"])).sum()
    assert np.array_equal(bits(ph.sd), bits(want["sd"])), "sd differs in %d rows" % (bits(ph.sd) != bits(want["sd"])).sum()
    assert ph.rank2.shape == want["rank2"].shape and np.array_equal(ph.rank2, want["rank2"])


def same_tables(a, b):
    """Two CohortPhenotypes, array for array (ms_pheno aside)."""
    assert (a.n_rows, a.n_samples, a.n_clustered, a.n_drop_na, a.n_drop_sd) == (b.n_rows, b.n_samples, b.n_clustered, b.n_drop_na, b.n_drop_sd)
    assert np.array_equal(a.row, b.row) and np.array_equal(a.n_na, b.n_na) and np.array_equal(a.rank2, b.rank2)
    assert np.array_equal(bits(a.mean), bits(b.mean)) and np.array_equal(bits(a.sd), bits(b.sd))


def text(m, cl, ph, quantile):
    """The table's text by a writer of its own; quantile(rank2, K) supplies the numbers."""
    K = len(ph.row)
    lines = ["#Chr\tstart\tend\tID" + "".join("\t" + s for s in m.sample_name) + "\n"]
    for k in range(K):
        i = int(ph.row[k])
        contig, strand = m.ref_name[int(m.tid[i])], m.strand[i].decode()
        f = [contig, "%d" % m.start[i], "%d" % m.end[i],
             "%s:%d:%d:clu_%d_%s" % (contig, m.start[i], m.end[i], int(cl.cluster[i]) + 1, strand if strand in "+-" else "NA")]
        f += ["%.17g" % quantile(int(r), K) for r in ph.rank2[k]]
        lines.append("\t".join(f) + "\n")
    return "".join(lines).encode()
