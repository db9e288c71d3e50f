"""Inputs the sQTL scan tests share (tests/test_cohort_qtl_host.py, tests/test_gpu_cohort_qtl.py): planted tables from a seeded generator.  A
case holds rank2 (K x S), regions (K x 3: tid, start, end), var_tid / var_pos (V, ascending, with equal positions), dosage (V x S int8), cov
(n_cov x S) and window.  What is planted: a few rows carry the effect of a variant inside their window; every row carries the covariates; some
dosages are missing; some variants are constant (all equal, all missing, equal where present); with explained=True one variant equals covariate 0,
so that the covariates explain it; two contigs; the last row lies where no variant reaches."""
import functools

import numpy as np

WINDOW = 1000
# (S, K, V, n_cov): the planted cases; S up to 70 and K, V up to 40, small enough for the restatement's rational arithmetic
PLANTED = [(12, 9, 16, 0), (30, 20, 24, 2), (64, 16, 20, 1), (65, 40, 40, 3), (70, 24, 40, 4)]


class Case(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.K, self.S = self.rank2.shape
        self.V = len(self.var_pos)
        self.n_cov = len(self.cov)
        self.dof = self.S - self.n_cov - 2

    def args(self):
        return (self.regions, self.var_tid, self.var_pos, self.dosage, self.cov, self.window)


def rank2_of(X):
    """Twice the average rank of every entry inside its column."""
    from scipy.stats import rankdata
    r2 = 2 * rankdata(X, axis=0)
    assert (r2 == np.round(r2)).all()
    return r2.astype(np.uint32)


def planted(S, K, V, n_cov, seed=None, window=WINDOW, explained=True, n_constant=None, missing=0.04, contigs=2, far_row=True, span=None):
    rng = np.random.default_rng(S * 1000003 + K * 1009 + V * 17 + n_cov if seed is None else seed)
    span = span if span is not None else max(4 * window, 1) * max(V // 8, 1)
    # variants: ascending by (tid, pos), a run of equal positions
    var_tid = np.sort(rng.integers(0, contigs, V)).astype(np.uint32)
    var_pos = (1 + rng.integers(0, span, V)).astype(np.uint32)
    if V > 4:
        var_pos[2] = var_pos[3]
    order = np.lexsort((var_pos, var_tid))
    var_tid, var_pos = var_tid[order], var_pos[order]
    maf = rng.uniform(0.15, 0.5, V)
    dosage = rng.binomial(2, maf[:, None], (V, S)).astype(np.int8)
    for v in range(V):                                          # (a drawn variant is not constant)
        if dosage[v].min() == dosage[v].max():
            dosage[v, :2] = (dosage[v, 0] + 1) % 3, (dosage[v, 0] + 2) % 3
    cov = rng.standard_normal((n_cov, S))
    n_constant = min(3, V // 8) if n_constant is None else n_constant
    special = rng.permutation(V)[:n_constant + 1]
    if explained and n_cov and V > 1:
        cov[0] = dosage[special[n_constant]].astype(np.float64)  # (no missing entries below: the covariate IS the variant)
    miss = rng.random((V, S)) < missing
    if explained and n_cov and V > 1:
        miss[special[n_constant]] = False
    dosage[miss] = -1
    for v in range(V):                                          # (nor does the missingness make it constant)
        if v not in special[:n_constant]:
            present = dosage[v][dosage[v] >= 0]
            if len(present) < 2 or present.min() == present.max():
                dosage[v] = rng.permutation(np.resize(np.array([0, 1, 2], np.int8), S))
                if explained and n_cov and v == special[n_constant]:
                    cov[0] = dosage[v].astype(np.float64)
    for i, v in enumerate(special[:n_constant]):
        if i % 3 == 0:
            dosage[v] = 1
        elif i % 3 == 1:
            dosage[v] = -1
        else:
            dosage[v] = np.where(rng.random(S) < 0.3, -1, 2)
    # rows: a region near a variant of its contig, the last one far behind every variant
    regions = np.zeros((K, 3), np.uint32)
    anchor = rng.integers(0, max(V, 1), K)
    for k in range(K):
        a = anchor[k] if V else 0
        start = max(1, int(var_pos[a]) + int(rng.integers(-window // 2, window // 2 + 1))) if V else 1 + int(rng.integers(0, span))
        regions[k] = (var_tid[a] if V else 0, start, start + int(rng.integers(1, 400)))
    if far_row and K > 1:
        regions[K - 1] = (contigs - 1, span + 10 * window + 5, span + 10 * window + 300)
    # phenotypes: noise + the covariates + for every third row the dosage of its anchor
    X = rng.standard_normal((K, S))
    if n_cov:
        X += rng.standard_normal((K, n_cov)) @ cov * 0.5
    for k in range(0, K, 3):
        if V:
            X[k] += 0.9 * np.where(dosage[anchor[k]] >= 0, dosage[anchor[k]], 1).astype(np.float64)
    return Case(rank2=rank2_of(X), regions=regions, var_tid=var_tid, var_pos=var_pos, dosage=dosage, cov=cov, window=window,
                anchor=anchor, special=special, n_constant=n_constant)


@functools.lru_cache(maxsize=None)
def case(S, K, V, n_cov):
    """planted() of one of PLANTED with its own seed, computed once; read-only."""
    c = planted(S, K, V, n_cov)
    for a in (c.rank2, c.regions, c.var_tid, c.var_pos, c.dosage, c.cov):
        a.setflags(write=False)
    return c


def check_conditions(c, q):
    """What every case must meet so that it cannot pass by comparing nothing (q: a result, from the restatement or the library)."""
    verdict, begin = np.asarray(q.variant_verdict), np.asarray(q.pair_begin).astype(np.int64)
    assert q.n_pairs > 0
    assert 4 * int((verdict != 0).sum()) <= c.V, "more than a quarter of the variants are unusable"
    assert 4 * int((np.diff(begin) == 0).sum()) <= c.K, "more than a quarter of the rows have no pairs"


def simple(S, K, V, n_cov, seed, window=WINDOW, span=None, contigs=2):
    """A planted case without the special variants: every one of the V variants is usable (asserted by the callers through the result)."""
    return planted(S, K, V, n_cov, seed=seed, window=window, explained=False, n_constant=0, missing=0.0, far_row=False, span=span, contigs=contigs)


def variants_near(regions, S, V, seed, window=WINDOW):
    """(var_tid, var_pos, dosage) for the rows of a cohort's table: V variants within the window of rows drawn from `regions`, ascending."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(regions), V)
    tid = regions[k, 0].astype(np.uint32)
    pos = np.maximum(1, regions[k, 1].astype(np.int64) + rng.integers(-window, window + 1, V)).astype(np.uint32)
    order = np.lexsort((pos, tid))
    dosage = rng.binomial(2, 0.4, (V, S)).astype(np.int8)
    dosage[:, 0], dosage[:, 1] = 0, 2                          # (no variant is constant)
    dosage[rng.random((V, S)) < 0.05] = -1
    dosage[:, 0], dosage[:, 1] = 0, 2
    return tid[order], pos[order], dosage


def write_vcf(path, m, regions, n, seed, samples):
    """A VCF of n usable records near the table's rows and the kinds the tool leaves out, in file order NOT sorted inside a contig.  Returns what the
    tool should make of it: (tid, pos, dosage in the order of `m`'s samples, ids), sorted stably by (tid, pos), and the three counts."""
    rng = np.random.default_rng(seed)
    names = list(m.ref_name)
    lines = ["##fileformat=VCFv4.2"] + ["##contig=<ID=%s>" % c for c in names] + ["##contig=<ID=elsewhere>",
             '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">', '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Depth">',
             "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples)]
    calls = ["0/0", "0/1", "1/0", "1/1", "0|1", "1|1", "./.", "./1", "1", "0/0/1", "."]
    value = {"0/0": 0, "0/1": 1, "1/0": 1, "1/1": 2, "0|1": 1, "1|1": 2}
    kept, skipped = [], [0, 0, 0]
    for i in range(n):
        k = int(rng.integers(0, len(regions)))
        tid, pos = int(regions[k, 0]), max(1, int(regions[k, 1]) + int(rng.integers(-300, 301)))
        gts = [calls[int(j)] for j in rng.choice(len(calls), len(samples), p=[.3, .2, .1, .15, .05, .05, .05, .02, .03, .02, .03])]
        gts[0], gts[1] = "0/0", "1/1"                             # (not constant, whichever samples the cohort takes... two of them are its)
        vid = "." if i % 2 else "rs%d" % i
        kind = i % 11
        if kind == 3:
            lines.append("%s\t%d\t%s\tA\tC,G\t.\t.\t.\tGT\t%s" % (names[tid], pos, vid, "\t".join(gts))); skipped[0] += 1
        elif kind == 5:
            lines.append("%s\t%d\t%s\tA\tC\t.\t.\t.\tDP\t%s" % (names[tid], pos, vid, "\t".join("7" for _ in gts))); skipped[1] += 1
        elif kind == 7:
            lines.append("elsewhere\t%d\t%s\tA\tC\t.\t.\t.\tGT\t%s" % (pos, vid, "\t".join(gts))); skipped[2] += 1
        else:
            fmt, cols = ("GT:DP", [g + ":9" for g in gts]) if kind == 2 else ("GT", gts)
            lines.append("%s\t%d\t%s\tG\tT\t.\t.\t.\t%s\t%s" % (names[tid], pos, vid, fmt, "\t".join(cols)))
            by_name = dict(zip(samples, gts))
            kept.append((tid, pos, [value.get(by_name.get(s), -1) for s in m.sample_name], vid if vid != "." else "%s:%d:G:T" % (names[tid], pos)))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    order = sorted(range(len(kept)), key=lambda i: (kept[i][0], kept[i][1]))
    kept = [kept[i] for i in order]
    return (np.array([x[0] for x in kept], np.uint32), np.array([x[1] for x in kept], np.uint32), np.array([x[2] for x in kept], np.int8),
            [x[3] for x in kept], skipped)
