#!/usr/bin/env python3
"""Measure the cohort junction-by-sample matrix (rgx_cohort_*) on one MI355X.  Prints one JSON line per part.

  --part pipeline   what accumulation costs the pipeline: sustained ms per file of a depth-2 Pipeline over --files submissions of one
                    configs[1]-shaped file (--reads), WITHOUT Cohort.add after each wait (the yardstick: the pipeline as it was) and WITH it,
                    alternating in one process, --reps times each; the two sets of times are printed whole
  --part finish     rgx_cohort_finish (ms_finish) beside rgx_cohort_merge_host on the same rows, for every SAMPLESxROWS of --sizes; the matrices
                    are compared; bytes moved per triple (counted from the passes, see finish_bytes_per_triple) over ms_finish against 8 TB/s

  --cluster         rgx_cohort_cluster (ms_cluster) on the matrix of the same SAMPLESxROWS cohorts: first and warm
                    calls on both paths (the matrix still in HBM behind its finish; uploaded through a cohort that never saw it), beside
                    rgx_cohort_cluster_host on the same matrix and the ms_finish of the same run; the results are compared word for word; bytes
                    moved per count entry by step 4 (counted from the passes, see cluster_bytes_per_entry) over ms_cluster against 8 TB/s

  --refine          rgx_cohort_refine (ms_cluster of its result) on the same cohorts, beside rgx_cohort_cluster on the same matrix in
                    the same process and rgx_cohort_refine_host: first and warm calls on both paths, the removal counts and rounds, and whether
                    every result was identical word for word between the paths and to the twin.  A size may end in ":heavy" (a sparse cohort with
                    heavy-tailed counts: a row counts up to 8,192 times as much in its home sample), the case in which the refinement bites;
                    --refine-params "max_intron,min_reads,num/den,min_rows,min_total" (default LeafCutter's customary 100000,5,1/1000,2,30)

  --pheno           rgx_cohort_phenotypes (ms_pheno) on the same cohorts, behind rgx_cohort_refine with --refine-params: first and warm
                    calls on both paths beside ms_cluster of the refinement in the same process and rgx_cohort_phenotypes_host, the kept rows and
                    the two drop counts, and whether the paths and the twin were identical (integers, and mean / sd as bit patterns);
                    --pheno-params "num/den,min_sd" (default 4/10,0.005); bytes moved per table entry (pheno_bytes_per_entry) over ms_pheno

  --pcs             rgx_cohort_pheno_pcs (ms_pcs, ms_gram, ms_eigen) on the phenotype tables of the same cohorts (behind
                    rgx_cohort_refine and rgx_cohort_phenotypes, whose ms_pheno of the same run is printed beside it), then on planted tables
                    --planted "SAMPLESxROWS,..." (a low-rank signal plus noise, ranked per column): first and warm calls, --n-pcs components
                    (default 10, clipped to the table), rgx_cohort_pheno_pcs_host's times, whether every array was identical to the twin's as bit
                    patterns, and K S (S + 1) / 2 fused multiply-adds over ms_gram as GFMA/s

  --qtl             rgx_cohort_qtl_nominal (ms_qtl, ms_residual, ms_pairs) on planted tables --planted "SAMPLESxROWSxVARIANTS,..."
                    (planted_rank2's table; rows and variants spread evenly over one contig of 500 bases per row; binomial dosages, 2 % missing):
                    first and warm calls with --n-cov principal components of the table as covariates (default 10, clipped) and --window (default
                    100000), beside rgx_cohort_qtl_nominal_host; the pairs P, P S fused multiply-adds over ms_pairs as GFMA/s (and the 4,096 S per tile that were issued), and whether every
                    device run was identical to the others and to the twin in every array as bit patterns

  --group           rgx_cohort_qtl_permute_grouped on --qtl's planted tables with --perms B permutations, the rows grouped in runs of
                    four (the planted table has no clusters), beside rgx_cohort_qtl_permute in the same process on the same inputs: --reps warm calls
                    of each behind a first one; ms_products, ms_beta, ms_perm, tiles and fill, the bytes copied home, the ratio of the warm
                    ms_products beside the spread of the ungrouped calls; every group checked as the maximum of its members
  --perm            rgx_cohort_qtl_permute (ms_perm, ms_residual, ms_products, ms_beta) on --qtl's planted tables with --perms B
                    permutations (default 1000, seed 0): first and warm calls; P (B + 1) S fused multiply-adds of the contract over ms_products as
                    GFMA/s, the 4,096 S per tile that were issued, the tile fill; rgx_cohort_qtl_permute_host where its P (B + 1) S stay below
                    --host-fmas (default 2e11), identical as bit patterns; and ms_pairs of rgx_cohort_qtl_nominal on the same inputs beside it
  --indep           rgx_cohort_qtl_independent on --qtl's planted tables with --perms B permutations: ms per phase, rounds and series;
                    then rgx_cohort_qtl_permute_conditional at m = 1 and m = 8 beside rgx_cohort_qtl_permute in the same process: ms_products per
                    tile of each, and the host twin when its work stays below --host-fmas
  --trans           rgx_cohort_qtl_trans (ms_trans, ms_residual, ms_count, ms_emit) on --qtl's planted tables at p <= --pval
                    (default 1e-5) with the pairs inside --window left out: --reps calls with the tile mapping's super-tiles of --band row blocks
                    (default 4) and --reps without the mapping; the 4,096 S fused multiply-adds issued per tile over ms_count as GFMA/s; beside it
                    rgx_cohort_qtl_nominal under the widest window on the same inputs, whose tiles are all full, as the yardstick; the twin where
                    its K U S stay below --host-fmas; every device run identical to the others and to the twin

Kernel times come from a run of its own:  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_cohort.py --part finish --no-host"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANCHOR = 8


class Sample(object):
    """What Cohort.add and cohort.merge_host read of an extractor, over a table made with numpy."""

    def __init__(self, table):
        self.table, self.min_anchor_length_, self._ctx = table, ANCHOR, None


MIXES = {"sparse": (5, 5, 10 / 3.0),      # a fifth of a sample's keys are in every sample, a fifth in no other, the rest drawn from a pool of 2 x rows
         "shared": (6, 150, 5.0),          # a sixth in every sample, 1 in 150 private, the rest from a pool of 5 x as many: most keys are in dozens of samples
         "heavy": (5, 5, 10 / 3.0)}        # sparse, with heavy-tailed counts and long-range junctions (make_sample): the input a refinement bites on


def make_sample(g, rows, rng, mix):
    """`rows` rows of sample g (tests/test_gpu_cohort.py builds its samples the same way)."""
    from regtools_amd import _ffi
    c, p, pool = MIXES[mix]
    common, private = rows // c, max(1, rows // p)
    draw = rows - common - private
    n_pool = int(draw * pool)
    ids = np.concatenate([np.arange(common), common + rng.choice(n_pool, draw, replace=False),
                          common + n_pool + g * private + np.arange(private)]).astype(np.int64)
    ids = rng.permutation(ids)
    t = np.zeros((rows, 12), np.uint32)
    start = 1000 + 3 * (ids // 23) + 40 * (ids % 2)
    end = start + 100 + ids % 50
    t[:, 0], t[:, 1], t[:, 2] = ids % 23, start, end
    t[:, 3] = start - ANCHOR - (ids * 3 + g * 5) % 20
    t[:, 4] = end + ANCHOR + (ids * 7 + g * 11) % 20
    t[:, 5] = 1 + (ids * 7 + g) % 9
    if mix == "heavy":
        # one key in 16 shares its start with a key far away on the contig (a long intron that ties clusters together), and a key counts up to
        # 8,192 times as much in its home sample (ids % 64 == g % 64)
        far = ids % 16 == 0
        end = np.where(far, start + 150_000 + 3 * (ids % 4096), end)
        t[:, 2], t[:, 4] = end, end + ANCHOR + (ids * 7 + g * 11) % 20
        boost = np.uint64(1) << (((ids.astype(np.uint64) * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(14))
        t[:, 5] = np.where(ids % 64 == g % 64, t[:, 5].astype(np.uint64) * boost, t[:, 5]).astype(np.uint32)
    t[:, 10] = np.where(ids % 3 == 0, ord("-"), ord("+"))
    proto = _ffi.JunctionTable()
    arr = (C.c_char_p * 23)(*[b"c%02d" % k for k in range(23)])
    lens = (C.c_uint32 * 23)(*([250_000_000] * 23))
    proto.n_ref, proto.ref_name, proto.ref_len = 23, arr, lens
    out = C.POINTER(_ffi.JunctionTable)()
    assert _ffi.lib().rgx_table_unpack(t.tobytes(), rows, C.byref(proto), C.byref(out)) == 0
    return out


def finish_bytes_per_triple(start_bits, end_bits, tid_bits):
    """HBM bytes per triple that finish's passes read and write: per key word one gather (permutation 4 + word 4 in, 4 out) and per
    8-bit pass a histogram read of the key (4) and a scatter (key + permutation in and out, 16); then the gather of the seven columns (4 + 28 in,
    28 out), the head flags (16 in, 4 out), their scan (4 in twice, 4 out), the row starts (8 in), the reduction (12 in) and the CSR image
    (4 x 4 in, 8 out).  Per-row words and the copy to the host are not counted."""
    passes = 1 + (end_bits + 7) // 8 + (start_bits + 7) // 8 + (tid_bits + 7) // 8
    return 4 * 12 + passes * 20 + 60 + 20 + 12 + 8 + 12 + 24


def part_finish(a):
    import regtools_amd
    from regtools_amd import _ffi, cohort
    ctx = regtools_amd.Context(0)
    for size in a.sizes.split(","):
        shape, _, mix = size.partition(":")
        mix = mix or "sparse"
        n_samples, rows = [int(x) for x in shape.lower().split("x")]
        rng = np.random.default_rng(3)
        t0 = time.time()
        tables = [make_sample(g, rows, rng, mix) for g in range(n_samples)]
        samples, names = [Sample(t) for t in tables], ["s%04d" % g for g in range(n_samples)]
        t_gen = time.time() - t0
        co = regtools_amd.Cohort(ctx=ctx)
        t0 = time.time()
        for s, nm in zip(samples, names):
            co.add(s, nm)
        t_add = time.time() - t0
        ms = []
        for _ in range(a.reps):                      # (the first finish grows the cohort's workspace and the page-locked result block)
            m = co.finish()
            ms.append(round(m.ms_finish, 3))
        bits = (int(m.start.max()).bit_length(), int(m.end.max()).bit_length(), max(1, (len(m.ref_name) - 1).bit_length()))
        bpt = finish_bytes_per_triple(*bits)
        best = min(ms[1:] or ms)
        line = {"part": "finish", "mix": mix, "samples": n_samples, "rows_per_sample": rows, "triples": m.n_triples, "rows": m.n, "mean_samples_per_row": round(m.n_triples / max(1, m.n), 2),
                "ms_finish": ms, "ms_finish_best_warm": best, "s_generate": round(t_gen, 2), "ms_add_wall_upload_path": round(1e3 * t_add, 1),
                "bytes_per_triple_counted": bpt, "TBps_over_ms_finish": round(bpt * m.n_triples / best / 1e9, 3),
                "share_of_8TBps": round(bpt * m.n_triples / best / 1e9 / 8.0, 4)}
        if not a.no_host:
            t0 = time.time()
            h = cohort.merge_host(samples, names)
            line["ms_merge_host_wall"] = round(1e3 * (time.time() - t0), 1)
            line["ms_merge_host"] = round(h.ms_finish, 1)
            line["device_over_host"] = round(h.ms_finish / best, 1)
            same = (m.n, m.n_triples) == (h.n, h.n_triples) and all(np.array_equal(getattr(m, k), getattr(h, k)) for k in
                    ("tid", "start", "end", "thick_start", "thick_end", "strand", "n_with", "total", "row_begin", "col_sample", "val_count"))
            line["identical_to_host"] = bool(same)
            assert same, "the device matrix differs from the host twin's"
            h.close()
        m.close()
        co.close()
        for t in tables:
            _ffi.lib().rgx_table_free(t)
        print(json.dumps(line), flush=True)


def cluster_bytes_per_entry(sample_bits, cluster_bits):
    """HBM bytes per count entry that step 4 of rgx_cohort_cluster reads and writes: the row lengths (val_count, 4 in), the
    expansion (col_sample + val_count in, three words out: 20), per key word of the pair sort its 8-bit passes (histogram read of the key 4 +
    scatter of key and permutation in and out 16) and, for the second word, one gather (permutation 4 + word 4 in, 4 out), the head flags (two
    permutation entries and their two words each: 24 in, 4 out), their scan (4 in twice, 4 out), the run starts (8 in) and the sums (permutation
    and count: 8 in).  Per-row, per-run and per-cluster words and the copy to the host are not counted."""
    passes = (sample_bits + 7) // 8 + (cluster_bits + 7) // 8
    return 4 + 20 + passes * 20 + 12 + 28 + 12 + 8 + 8


CLUSTER_ARRAYS = ("cluster", "cl_begin", "cl_row", "cl_total", "cs_begin", "cs_sample", "cs_total")


def part_cluster(a):
    import regtools_amd
    from regtools_amd import _ffi, cohort
    ctx = regtools_amd.Context(0)
    for size in a.sizes.split(","):
        shape, _, mix = size.partition(":")
        mix = mix or "sparse"
        n_samples, rows = [int(x) for x in shape.lower().split("x")]
        rng = np.random.default_rng(3)
        tables = [make_sample(g, rows, rng, mix) for g in range(n_samples)]
        co = regtools_amd.Cohort(ctx=ctx)
        for g, t in enumerate(tables):
            co.add(Sample(t), "s%04d" % g)
        for _ in range(2):                           # (the second finish is a warm one)
            m = co.finish()
        in_hbm, uploaded = [], []
        for _ in range(a.reps):                      # (the first call grows the cohort's workspace and the page-locked result block)
            cl = co.cluster(m)
            in_hbm.append(round(cl.ms_cluster, 3))
        other = regtools_amd.Cohort(ctx=ctx)
        for _ in range(a.reps):
            up = other.cluster(m)
            uploaded.append(round(up.ms_cluster, 3))
        assert co.cluster_paths == [1] * a.reps and other.cluster_paths == [0] * a.reps
        entries = int(m.row_begin[-1])
        sizes = np.diff(cl.cl_begin)
        bpe = cluster_bytes_per_entry(max(1, (n_samples - 1).bit_length()), max(1, (cl.n_clusters - 1).bit_length()))
        best = min(in_hbm[1:] or in_hbm)
        line = {"part": "cluster", "mix": mix, "samples": n_samples, "rows_per_sample": rows, "rows": m.n, "count_entries": entries,
                "components": cl.n_components, "clusters": cl.n_clusters, "largest_cluster_rows": int(sizes.max()), "singletons": int((sizes == 1).sum()),
                "cluster_sample_pairs": int(cl.cs_begin[-1]), "n_rounds": cl.n_rounds, "ms_finish_same_run": round(m.ms_finish, 3),
                "ms_cluster_in_hbm": in_hbm, "ms_cluster_uploaded": uploaded, "ms_cluster_best_warm": best,
                "paths_equal": bool(all(np.array_equal(getattr(cl, k), getattr(up, k)) for k in CLUSTER_ARRAYS)),
                "step4_bytes_per_entry_counted": bpe, "step4_TBps_over_ms_cluster": round(bpe * entries / best / 1e9, 3),
                "share_of_8TBps": round(bpe * entries / best / 1e9 / 8.0, 4)}
        assert line["paths_equal"], "the two paths differ"
        if not a.no_host:
            h = cohort.cluster_host(m)
            line["ms_cluster_host"] = round(h.ms_cluster, 1)
            line["device_over_host"] = round(h.ms_cluster / best, 1)
            same = (cl.n_clusters, cl.n_components) == (h.n_clusters, h.n_components) and all(np.array_equal(getattr(cl, k), getattr(h, k)) for k in CLUSTER_ARRAYS)
            line["identical_to_host"] = bool(same)
            assert same, "the device clusters differ from the host twin's"
            h.close()
        cl.close(); up.close(); m.close(); co.close(); other.close()
        for t in tables:
            _ffi.lib().rgx_table_free(t)
        print(json.dumps(line), flush=True)


def part_refine(a):
    import regtools_amd
    from regtools_amd import _ffi, cohort
    f = a.refine_params.split(",")
    num, den = [int(x) for x in f[2].split("/")]
    kw = dict(max_intron=int(f[0]), min_reads=int(f[1]), min_ratio=(num, den), min_rows=int(f[3]), min_total=int(f[4]))
    ctx = regtools_amd.Context(0)
    for size in a.sizes.split(","):
        shape, _, mix = size.partition(":")
        mix = mix or "sparse"
        n_samples, rows = [int(x) for x in shape.lower().split("x")]
        rng = np.random.default_rng(3)
        tables = [make_sample(g, rows, rng, mix) for g in range(n_samples)]
        co = regtools_amd.Cohort(ctx=ctx)
        for g, t in enumerate(tables):
            co.add(Sample(t), "s%04d" % g)
        for _ in range(2):                           # (the second finish is a warm one)
            m = co.finish()
        other = regtools_amd.Cohort(ctx=ctx)
        plain, in_hbm, uploaded, same_paths, results = [], [], [], True, []
        for _ in range(a.reps):                      # cluster and refine alternate on the same matrix, in the same process
            cl = co.cluster(m, min_rows=kw["min_rows"], min_total=kw["min_total"])
            plain.append(round(cl.ms_cluster, 3))
            rf = co.refine(m, **kw)
            in_hbm.append(round(rf.ms_cluster, 3))
            up = other.refine(m, **kw)
            uploaded.append(round(up.ms_cluster, 3))
            same_paths &= (rf.n_ineligible, rf.n_weak, rf.n_components) == (up.n_ineligible, up.n_weak, up.n_components) and all(
                np.array_equal(getattr(rf, k), getattr(up, k)) for k in CLUSTER_ARRAYS)
            results.append(rf)
        assert co.cluster_paths == [1, 1] * a.reps and other.cluster_paths == [0] * a.reps
        sizes, plain_sizes = np.diff(rf.cl_begin), np.diff(cl.cl_begin)
        line = {"part": "refine", "mix": mix, "samples": n_samples, "rows_per_sample": rows, "rows": m.n, "count_entries": int(m.row_begin[-1]), "params": kw,
                "n_ineligible": rf.n_ineligible, "n_weak": rf.n_weak, "components": rf.n_components, "clusters": rf.n_clusters,
                "largest_cluster_rows": int(sizes.max()) if len(sizes) else 0, "rows_clustered": int(rf.cl_begin[-1]),
                "unrefined_clusters": cl.n_clusters, "unrefined_largest_cluster_rows": int(plain_sizes.max()) if len(plain_sizes) else 0,
                "n_rounds": rf.n_rounds, "n_rounds_cluster": cl.n_rounds, "ms_refine_in_hbm": in_hbm, "ms_refine_uploaded": uploaded, "ms_cluster": plain,
                "ms_refine_best_warm": min(in_hbm[1:] or in_hbm), "ms_cluster_best_warm": min(plain[1:] or plain), "paths_equal_every_time": bool(same_paths)}
        assert same_paths, "the two paths differ"
        if not a.no_host:
            h = cohort.refine_host(m, **kw)
            line["ms_refine_host"] = round(h.ms_cluster, 1)
            line["device_over_host"] = round(h.ms_cluster / line["ms_refine_best_warm"], 1)
            same = all((r.n_clusters, r.n_components, r.n_ineligible, r.n_weak) == (h.n_clusters, h.n_components, h.n_ineligible, h.n_weak) and all(
                np.array_equal(getattr(r, k), getattr(h, k)) for k in CLUSTER_ARRAYS) for r in results)
            line["identical_to_host_every_time"] = bool(same)
            assert same, "the device's refined clusters differ from the host twin's"
            h.close()
        for r in results:
            r.close()
        m.close(); co.close(); other.close()
        for t in tables:
            _ffi.lib().rgx_table_free(t)
        print(json.dumps(line), flush=True)


def pheno_bytes_per_entry(sample_bits):
    """HBM bytes per entry of the K x S table that rgx_cohort_phenotypes reads and writes behind the row statistics: the keys (12
    out), the sort -- per 8-bit pass a histogram read of the key (4) and a scatter of key and permutation in and out (16); four passes on the low
    word, a gather (permutation 4 + word 4 in, 4 out) and four passes on the high word, a gather and the sample word's passes -- the tie heads (two
    permutation entries and their two words each: 24 in, 4 out), their scan (4 in twice, 4 out), the run starts (8 in) and the ranks (permutation,
    head, scan and two run starts: 20 in, 4 out).  The CSR lookups of the statistics and of the keys (per row: they stay in cache across a row's
    samples), per-row words and the copy to the host are not counted."""
    passes = 8 + (sample_bits + 7) // 8
    return 12 + passes * 20 + 2 * 12 + 28 + 12 + 8 + 24


PHENO_ARRAYS = ("row", "n_na", "rank2")


def same_pheno(a, b):
    return (a.n_rows, a.n_clustered, a.n_drop_na, a.n_drop_sd) == (b.n_rows, b.n_clustered, b.n_drop_na, b.n_drop_sd) and all(
        np.array_equal(getattr(a, k), getattr(b, k)) for k in PHENO_ARRAYS) and all(
        np.array_equal(getattr(a, k).view(np.uint64), getattr(b, k).view(np.uint64)) for k in ("mean", "sd"))


def part_pheno(a):
    import regtools_amd
    from regtools_amd import _ffi, cohort
    f = a.refine_params.split(",")
    num, den = [int(x) for x in f[2].split("/")]
    kw = dict(max_intron=int(f[0]), min_reads=int(f[1]), min_ratio=(num, den), min_rows=int(f[3]), min_total=int(f[4]))
    share, min_sd = a.pheno_params.split(",")
    pkw = dict(max_missing=tuple(int(x) for x in share.split("/")), min_sd=float(min_sd))
    ctx = regtools_amd.Context(0)
    for size in a.sizes.split(","):
        shape, _, mix = size.partition(":")
        mix = mix or "sparse"
        n_samples, rows = [int(x) for x in shape.lower().split("x")]
        rng = np.random.default_rng(3)
        tables = [make_sample(g, rows, rng, mix) for g in range(n_samples)]
        co = regtools_amd.Cohort(ctx=ctx)
        for g, t in enumerate(tables):
            co.add(Sample(t), "s%04d" % g)
        for _ in range(2):                           # (the second finish is a warm one)
            m = co.finish()
        other = regtools_amd.Cohort(ctx=ctx)
        refine, in_hbm, uploaded, same_paths, ph = [], [], [], True, None
        for _ in range(a.reps):                      # refine and phenotypes alternate on the same matrix, in the same process
            rf = co.refine(m, **kw)
            refine.append(round(rf.ms_cluster, 3))
            ph = co.phenotypes(m, rf, **pkw)
            in_hbm.append(round(ph.ms_pheno, 3))
            up = other.phenotypes(m, rf, **pkw)
            uploaded.append(round(up.ms_pheno, 3))
            same_paths &= same_pheno(ph, up)
        assert co.cluster_paths == [1, 1] * a.reps and other.cluster_paths == [0] * a.reps
        entries = ph.n_rows * n_samples
        bpe = pheno_bytes_per_entry(max(1, (n_samples - 1).bit_length()))
        best = min(in_hbm[1:] or in_hbm)
        line = {"part": "pheno", "mix": mix, "samples": n_samples, "rows_per_sample": rows, "rows": m.n, "count_entries": int(m.row_begin[-1]),
                "refine_params": kw, "pheno_params": {"max_missing": list(pkw["max_missing"]), "min_sd": pkw["min_sd"]},
                "n_clustered": ph.n_clustered, "n_drop_na": ph.n_drop_na, "n_drop_sd": ph.n_drop_sd, "rows_kept": ph.n_rows, "table_entries": entries,
                "ms_pheno_in_hbm": in_hbm, "ms_pheno_uploaded": uploaded, "ms_refine_same_run": refine, "ms_pheno_best_warm": best,
                "ms_refine_best_warm": min(refine[1:] or refine), "paths_equal_every_time": bool(same_paths),
                "bytes_per_entry_counted": bpe, "TBps_over_ms_pheno": round(bpe * entries / best / 1e9, 3),
                "share_of_8TBps": round(bpe * entries / best / 1e9 / 8.0, 4)}
        assert same_paths, "the two paths differ"
        if not a.no_host:
            h = cohort.phenotypes_host(m, rf, **pkw)
            line["ms_pheno_host"] = round(h.ms_pheno, 1)
            line["device_over_host"] = round(h.ms_pheno / best, 1)
            line["identical_to_host"] = bool(same_pheno(ph, h))
            assert line["identical_to_host"], "the device's phenotype table differs from the host twin's"
            h.close()
        ph.close(); up.close(); rf.close(); m.close(); co.close(); other.close()
        for t in tables:
            _ffi.lib().rgx_table_free(t)
        print(json.dumps(line), flush=True)


def planted_rank2(n_samples, rows, n_f=5, seed=7):
    """rows x n_samples uint32: twice the rank per column of X = F L + 0.5 N (tests/pca_cases.py's construction in float32, no ties), made 64 columns
    at a time."""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((rows, n_f), dtype=np.float32)
    out = np.empty((rows, n_samples), np.uint32)
    for s0 in range(0, n_samples, 64):
        w = min(64, n_samples - s0)
        L = rng.standard_normal((n_f, w), dtype=np.float32) * (3 * 0.7 ** np.arange(n_f, dtype=np.float32))[:, None]
        X = F @ L + 0.5 * rng.standard_normal((rows, w), dtype=np.float32)
        order = np.argsort(X, axis=0, kind="stable")
        rank = np.empty_like(order)
        np.put_along_axis(rank, order, np.arange(1, rows + 1, dtype=order.dtype)[:, None], axis=0)
        out[:, s0:s0 + w] = 2 * rank
    return out


PCS_ARRAYS = ("col_sum", "gram", "variance", "component")


def same_pcs(a, b):
    return (a.n_rows, a.n_samples, a.n_pcs) == (b.n_rows, b.n_samples, b.n_pcs) and all(
        np.array_equal(np.ascontiguousarray(getattr(a, k)).view(np.uint64), np.ascontiguousarray(getattr(b, k)).view(np.uint64)) for k in PCS_ARRAYS)


def pcs_line(a, co, ph, line):
    """The --pcs measurements of one table, added to `line` and printed."""
    from regtools_amd import cohort
    K, S = ph.n_rows, ph.n_samples
    line.update({"rows_kept": K, "samples": S})
    if K < 2 or S < 1 or S > 2048:
        line["skipped"] = "a table of %d rows and %d samples has no components" % (K, S)
        print(json.dumps(line), flush=True)
        return
    n_pcs = min(a.n_pcs, K, S)
    runs = [co.pheno_pcs(ph, n_pcs) for _ in range(a.reps)]
    warm = runs[1:] or runs
    best = min(warm, key=lambda p: p.ms_gram)
    fmas = K * S * (S + 1) // 2
    line.update({"n_pcs": n_pcs, "n_chunks": min(64, -(-K // 1024)), "tile_pairs": (-(-S // 64)) * (-(-S // 64) + 1) // 2,
                 "ms_pcs": [round(p.ms_pcs, 3) for p in runs], "ms_gram": [round(p.ms_gram, 3) for p in runs],
                 "ms_eigen": [round(p.ms_eigen, 3) for p in runs], "ms_gram_best_warm": round(best.ms_gram, 3),
                 "ms_eigen_best_warm": round(min(p.ms_eigen for p in warm), 3), "fmas": fmas, "GFMA_per_s_over_ms_gram": round(fmas / best.ms_gram / 1e6, 1),
                 "identical_every_time": bool(all(same_pcs(runs[0], p) for p in runs[1:]))})
    assert line["identical_every_time"], "two device runs differ"
    if not a.no_host:
        h = cohort.pheno_pcs_host(ph, n_pcs)
        line.update({"ms_pcs_host": round(h.ms_pcs, 1), "ms_gram_host": round(h.ms_gram, 1), "ms_eigen_host": round(h.ms_eigen, 1),
                     "gram_device_over_host": round(h.ms_gram / best.ms_gram, 1), "identical_to_host": bool(same_pcs(runs[0], h))})
        assert line["identical_to_host"], "the device's principal components differ from the host twin's"
        h.close()
    for p in runs:
        p.close()
    print(json.dumps(line), flush=True)


def part_pcs(a):
    import regtools_amd
    from regtools_amd import _ffi, cohort
    f = a.refine_params.split(",")
    num, den = [int(x) for x in f[2].split("/")]
    kw = dict(max_intron=int(f[0]), min_reads=int(f[1]), min_ratio=(num, den), min_rows=int(f[3]), min_total=int(f[4]))
    share, min_sd = a.pheno_params.split(",")
    pkw = dict(max_missing=tuple(int(x) for x in share.split("/")), min_sd=float(min_sd))
    ctx = regtools_amd.Context(0)
    for size in [x for x in a.sizes.split(",") if x]:
        shape, _, mix = size.partition(":")
        mix = mix or "sparse"
        n_samples, rows = [int(x) for x in shape.lower().split("x")]
        rng = np.random.default_rng(3)
        tables = [make_sample(g, rows, rng, mix) for g in range(n_samples)]
        co = regtools_amd.Cohort(ctx=ctx)
        for g, t in enumerate(tables):
            co.add(Sample(t), "s%04d" % g)
        m = co.finish()
        pheno = []
        for _ in range(a.reps):
            rf = co.refine(m, **kw)
            ph = co.phenotypes(m, rf, **pkw)
            pheno.append(round(ph.ms_pheno, 3))
        pcs_line(a, co, ph, {"part": "pcs", "table": "cohort", "mix": mix, "rows_per_sample": rows, "rows": m.n, "ms_pheno_same_run": pheno})
        ph.close(); rf.close(); m.close(); co.close()
        for t in tables:
            _ffi.lib().rgx_table_free(t)
    co = regtools_amd.Cohort(ctx=ctx)
    for size in [x for x in a.planted.split(",") if x]:
        n_samples, rows = [int(x) for x in size.lower().split("x")]
        t0 = time.time()
        ph = cohort.pheno_table_from_rank2(planted_rank2(n_samples, rows))
        pcs_line(a, co, ph, {"part": "pcs", "table": "planted", "s_generate": round(time.time() - t0, 1)})
    co.close()


QTL_ARRAYS = ("variant_verdict", "yy", "gg", "pair_begin", "pair_variant", "r", "slope", "best")


def same_qtl(a, b):
    def bits(x):
        x = np.ascontiguousarray(x)
        return x.view(np.uint64) if x.dtype == np.float64 else x
    return a.n_pairs == b.n_pairs and all(np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))) for k in QTL_ARRAYS)


def planted_qtl_inputs(a, co, S, K, V):
    """--qtl's and --perm's table: (the phenotype table, regions, positions, dosages, the components taken as covariates or None, their number)."""
    from regtools_amd import cohort
    rng = np.random.default_rng(11)
    ph = cohort.pheno_table_from_rank2(planted_rank2(S, K))
    span = 500 * K
    start = np.sort(rng.integers(1, span, K)).astype(np.uint32)
    regions = np.stack([np.zeros(K, np.uint32), start, start + rng.integers(50, 5000, K).astype(np.uint32)], axis=1)
    pos = np.sort(rng.integers(1, span, V)).astype(np.uint32)
    dosage = rng.binomial(2, rng.uniform(0.05, 0.5, V)[:, None], (V, S)).astype(np.int8)
    dosage[rng.random((V, S)) < 0.02] = -1
    n_cov = max(0, min(a.n_cov, K, S - 3))
    return ph, regions, pos, dosage, co.pheno_pcs(ph, n_cov) if n_cov else None, n_cov


def part_qtl(a):
    import regtools_amd
    from regtools_amd import cohort
    co = regtools_amd.Cohort(ctx=regtools_amd.Context(0))
    for size in [x for x in (a.planted or "64x4000x6000").split(",") if x]:
        S, K, V = [int(x) for x in size.lower().split("x")]
        t0 = time.time()
        ph, regions, pos, dosage, pcs, n_cov = planted_qtl_inputs(a, co, S, K, V)
        args = (ph, regions, np.zeros(V, np.uint32), pos, dosage, pcs.component if pcs else None, a.window)
        line = {"part": "qtl", "samples": S, "rows": K, "variants": V, "n_cov": n_cov, "window": a.window, "s_generate": round(time.time() - t0, 1)}
        runs = [co.qtl_nominal(*args) for _ in range(a.reps)]
        warm = runs[1:] or runs
        best = min(warm, key=lambda q: q.ms_pairs)
        P = runs[0].n_pairs
        line.update({"pairs": P, "usable_variants": int((runs[0].variant_verdict == 0).sum()), "flat_rows": runs[0].n_flat_rows,
                     "ms_qtl": [round(q.ms_qtl, 3) for q in runs], "ms_residual": [round(q.ms_residual, 3) for q in runs],
                     "ms_pairs": [round(q.ms_pairs, 3) for q in runs], "ms_pairs_best_warm": round(best.ms_pairs, 3), "fmas": P * S,
                     "tiles": runs[0].n_tiles, "tile_fill": round(P / (4096.0 * runs[0].n_tiles), 3) if runs[0].n_tiles else None,
                     "GFMA_per_s_issued_over_ms_pairs": round(4096.0 * runs[0].n_tiles * S / best.ms_pairs / 1e6, 1) if best.ms_pairs > 0 else None,
                     "GFMA_per_s_over_ms_pairs": round(P * S / best.ms_pairs / 1e6, 1) if best.ms_pairs > 0 else None,
                     "identical_every_time": bool(all(same_qtl(runs[0], q) for q in runs[1:]))})
        assert line["identical_every_time"], "two device runs differ"
        if not a.no_host:
            h = cohort.qtl_nominal_host(*args)
            line.update({"ms_qtl_host": round(h.ms_qtl, 1), "ms_residual_host": round(h.ms_residual, 1), "ms_pairs_host": round(h.ms_pairs, 1),
                         "identical_to_host": bool(same_qtl(runs[0], h))})
            assert line["identical_to_host"], "the device's scan differs from the host twin's"
            h.close()
        for q in runs:
            q.close()
        print(json.dumps(line), flush=True)
    co.close()


TRANS_ARRAYS = ("variant_verdict", "yy", "gg", "hit_begin", "hit_variant", "r", "slope")


def same_trans(a, b):
    def bits(x):
        x = np.ascontiguousarray(x)
        return x.view(np.uint64) if x.dtype == np.float64 else x
    return (a.n_hits, a.n_tested) == (b.n_hits, b.n_tested) and all(np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))) for k in TRANS_ARRAYS)


def part_trans(a):
    """rgx_cohort_qtl_trans on --qtl's planted tables at p <= --pval, the cis pairs inside --window left out: --reps calls with the tile mapping's
    super-tiles (--band row blocks) and --reps without the mapping, every one identical; the issued fused multiply-adds (4,096 S per tile of usable
    variants) over the best warm ms_count; beside it, in the same process on the same inputs, rgx_cohort_qtl_nominal under the widest window, whose
    tiles are all full: k_qtl_pairs, the same slab loop, as the yardstick.  The twin runs when its fused multiply-adds stay below --host-fmas."""
    import regtools_amd
    from regtools_amd import cohort
    co = regtools_amd.Cohort(ctx=regtools_amd.Context(0))
    for size in [x for x in (a.planted or "64x4000x6000").split(",") if x]:
        S, K, V = [int(x) for x in size.lower().split("x")]
        t0 = time.time()
        ph, regions, pos, dosage, pcs, n_cov = planted_qtl_inputs(a, co, S, K, V)
        args = (ph, regions, np.zeros(V, np.uint32), pos, dosage, pcs.component if pcs else None)
        kw = dict(pval=a.pval, exclude_window=a.window)
        line = {"part": "trans", "samples": S, "rows": K, "variants": V, "n_cov": n_cov, "pval": a.pval, "exclude_window": a.window,
                "s_generate": round(time.time() - t0, 1)}
        runs = {}
        for band in (a.band, 0):
            os.environ["REGTOOLS_AMD_TRANS_BAND"] = str(band)
            runs[band] = [co.qtl_trans(*args, **kw) for _ in range(a.reps)]
        del os.environ["REGTOOLS_AMD_TRANS_BAND"]
        first = runs[a.band][0]
        U = int((first.variant_verdict == 0).sum())
        issued = 4096.0 * S * ((K + 63) // 64) * ((U + 63) // 64)
        line.update({"usable_variants": U, "flat_rows": first.n_flat_rows, "tested": first.n_tested, "hits": first.n_hits, "tiles": first.n_tiles,
                     "hit_tiles": first.n_hit_tiles, "fmas_issued": issued, "r_min": cohort.qtl_r_threshold(a.pval, first.dof)})
        for band, name in ((a.band, "band%d" % a.band), (0, "unmapped")):
            rs = runs[band]
            best = min((rs[1:] or rs), key=lambda q: q.ms_count)
            line.update({"ms_trans_" + name: [round(q.ms_trans, 3) for q in rs], "ms_count_" + name: [round(q.ms_count, 3) for q in rs],
                         "ms_emit_" + name: [round(q.ms_emit, 3) for q in rs], "ms_residual_" + name: [round(q.ms_residual, 3) for q in rs],
                         "GFMA_per_s_issued_count_" + name: round(issued / best.ms_count / 1e6, 1) if best.ms_count > 0 else None})
        every = runs[a.band] + runs[0]
        line["identical_every_time"] = bool(all(same_trans(every[0], q) for q in every[1:]))
        assert line["identical_every_time"], "two device runs differ"
        # the yardstick stores every pair (20 bytes each): on the same inputs up to 2^26 pairs, else on a table of fewer rows and the same variants
        Kn = K if K * V <= 1 << 26 else max(64, (1 << 26) // V // 64 * 64)
        if Kn * V <= 1 << 28:
            n_args = args
            if Kn != K:
                ph_n, regions_n, pos_n, dosage_n, pcs_n, _ = planted_qtl_inputs(a, co, S, Kn, V)
                n_args = (ph_n, regions_n, np.zeros(V, np.uint32), pos_n, dosage_n, pcs_n.component if pcs_n else None)
            nominal = [co.qtl_nominal(*n_args, 0xffffffff) for _ in range(a.reps)]
            best = min((nominal[1:] or nominal), key=lambda q: q.ms_pairs)
            line.update({"nominal_rows": Kn, "nominal_pairs": nominal[0].n_pairs, "nominal_tiles": nominal[0].n_tiles,
                         "nominal_tile_fill": round(nominal[0].n_pairs / (4096.0 * nominal[0].n_tiles), 3) if nominal[0].n_tiles else None,
                         "nominal_ms_pairs": [round(q.ms_pairs, 3) for q in nominal],
                         "GFMA_per_s_issued_nominal_pairs": round(4096.0 * nominal[0].n_tiles * S / best.ms_pairs / 1e6, 1) if best.ms_pairs > 0 else None})
            for q in nominal:
                q.close()
        if not a.no_host and float(K) * U * S <= a.host_fmas:
            h = cohort.qtl_trans_host(*args, **kw)
            line.update({"ms_trans_host": round(h.ms_trans, 1), "ms_count_host": round(h.ms_count, 1), "identical_to_host": bool(same_trans(every[0], h))})
            assert line["identical_to_host"], "the device's scan differs from the host twin's"
            h.close()
        for q in every:
            q.close()
        print(json.dumps(line), flush=True)
    co.close()


PERM_ARRAYS = ("variant_verdict", "yy", "gg", "n_cis", "perm_r", "best_variant", "best_r", "best_slope", "n_ge", "p_perm", "beta_shape1", "beta_shape2",
               "p_beta", "beta_status")


def same_perm(a, b):
    def bits(x):
        x = np.ascontiguousarray(x)
        return x.view(np.uint64) if x.dtype == np.float64 else x
    return a.n_pairs == b.n_pairs and all(np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))) for k in PERM_ARRAYS)


def part_perm(a):
    import regtools_amd
    from regtools_amd import cohort
    co = regtools_amd.Cohort(ctx=regtools_amd.Context(0))
    for size in [x for x in (a.planted or "64x4000x6000").split(",") if x]:
        S, K, V = [int(x) for x in size.lower().split("x")]
        t0 = time.time()
        ph, regions, pos, dosage, pcs, n_cov = planted_qtl_inputs(a, co, S, K, V)
        B = a.perms
        perms = cohort.qtl_permutations(S, B, 0)
        args = (ph, regions, np.zeros(V, np.uint32), pos, dosage, pcs.component if pcs else None, a.window)
        line = {"part": "perm", "samples": S, "rows": K, "variants": V, "n_cov": n_cov, "window": a.window, "perms": B,
                "s_generate": round(time.time() - t0, 1)}
        runs = [co.qtl_permute(*args, perms=perms) for _ in range(a.reps)]
        warm = runs[1:] or runs
        best = min(warm, key=lambda q: q.ms_products)
        P, tiles = runs[0].n_pairs, runs[0].n_tiles
        fmas = P * (B + 1) * S
        line.update({"pairs": P, "rows_with_pairs": int((runs[0].n_cis > 0).sum()), "ms_perm": [round(q.ms_perm, 3) for q in runs],
                     "ms_residual": [round(q.ms_residual, 3) for q in runs], "ms_products": [round(q.ms_products, 3) for q in runs],
                     "ms_beta": [round(q.ms_beta, 1) for q in runs], "ms_products_best_warm": round(best.ms_products, 3), "fmas": fmas,
                     "tiles": tiles, "tile_fill": round(P * (B + 1) / (4096.0 * tiles), 3) if tiles else None,
                     "GFMA_per_s_issued_over_ms_products": round(4096.0 * tiles * S / best.ms_products / 1e6, 1) if best.ms_products > 0 else None,
                     "GFMA_per_s_over_ms_products": round(fmas / best.ms_products / 1e6, 1) if best.ms_products > 0 else None,
                     "beta_status_counts": np.bincount(runs[0].beta_status, minlength=3).tolist(),
                     "identical_every_time": bool(all(same_perm(runs[0], q) for q in runs[1:]))})
        assert line["identical_every_time"], "two device runs differ"
        nominal = [co.qtl_nominal(*args) for _ in range(2)]
        line.update({"nominal_ms_pairs": [round(q.ms_pairs, 3) for q in nominal], "nominal_ms_qtl": [round(q.ms_qtl, 3) for q in nominal]})
        has = nominal[0].best != 0xffffffff
        assert np.array_equal(runs[0].best_variant[has], nominal[0].pair_variant[nominal[0].best[has]]), "the best variants differ from the nominal scan's"
        for q in nominal:
            q.close()
        if not a.no_host and fmas <= a.host_fmas:
            h = cohort.qtl_permute_host(*args, perms=perms)
            line.update({"ms_perm_host": round(h.ms_perm, 1), "ms_products_host": round(h.ms_products, 1), "ms_beta_host": round(h.ms_beta, 1),
                         "identical_to_host": bool(same_perm(runs[0], h))})
            assert line["identical_to_host"], "the device's permutation pass differs from the host twin's"
            h.close()
        for q in runs:
            q.close()
        print(json.dumps(line), flush=True)
    co.close()


GROUP_ARRAYS = ("variant_verdict", "yy", "gg", "n_cis", "grp_begin", "grp_row", "group_n_cis", "perm_r", "best_row", "best_variant", "best_r",
                "best_slope", "n_ge", "p_perm", "beta_shape1", "beta_shape2", "p_beta", "beta_status")


def same_group(a, b):
    def bits(x):
        x = np.ascontiguousarray(x)
        return x.view(np.uint64) if x.dtype == np.float64 else x
    return a.n_pairs == b.n_pairs and all(np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))) for k in GROUP_ARRAYS)


def part_group(a):
    """rgx_cohort_qtl_permute_grouped beside rgx_cohort_qtl_permute in one process on the same inputs; the planted table has no clusters, so its
    groups are runs of four rows."""
    import regtools_amd
    from regtools_amd import cohort
    co = regtools_amd.Cohort(ctx=regtools_amd.Context(0))
    for size in [x for x in (a.planted or "64x4000x6000").split(",") if x]:
        S, K, V = [int(x) for x in size.lower().split("x")]
        ph, regions, pos, dosage, pcs, n_cov = planted_qtl_inputs(a, co, S, K, V)
        B = a.perms
        perms = cohort.qtl_permutations(S, B, 0)
        groups, G = (np.arange(K) // 4).astype(np.uint32), (K + 3) // 4
        tail = (np.zeros(V, np.uint32), pos, dosage, pcs.component if pcs else None, a.window)
        line = {"part": "group", "samples": S, "rows": K, "variants": V, "n_cov": n_cov, "window": a.window, "perms": B, "groups": G}
        flat = [co.qtl_permute(ph, regions, *tail, perms=perms) for _ in range(a.reps + 1)]
        runs = [co.qtl_permute_grouped(ph, regions, groups, G, *tail, perms=perms) for _ in range(a.reps + 1)]
        warm_flat, warm = [q.ms_products for q in flat[1:]], [q.ms_products for q in runs[1:]]
        P, tiles = runs[0].n_pairs, runs[0].n_tiles
        fmas = P * (B + 1) * S
        ub, gb = np.ascontiguousarray(flat[0].perm_r).view(np.uint64), np.ascontiguousarray(runs[0].perm_r).view(np.uint64)
        pad = np.zeros(((-K) % 4, B + 1), np.uint64)
        line.update({"pairs": P, "groups_with_pairs": int((runs[0].group_n_cis > 0).sum()), "ms_perm": [round(q.ms_perm, 3) for q in runs],
                     "ms_residual": [round(q.ms_residual, 3) for q in runs], "ms_products": [round(q.ms_products, 3) for q in runs],
                     "ms_beta": [round(q.ms_beta, 1) for q in runs], "ms_products_best_warm": round(min(warm), 3), "fmas": fmas,
                     "tiles": tiles, "tile_fill": round(P * (B + 1) / (4096.0 * tiles), 3) if tiles else None,
                     "GFMA_per_s_over_ms_products": round(fmas / min(warm) / 1e6, 1) if min(warm) > 0 else None,
                     "bytes_home": int(G * (B + 1) * 8 + G * 24 + K * 12 + V * 9 + 32),
                     "ungrouped_ms_products": [round(q.ms_products, 3) for q in flat], "ungrouped_ms_beta": [round(q.ms_beta, 1) for q in flat],
                     "ungrouped_ms_perm": [round(q.ms_perm, 3) for q in flat], "ungrouped_tiles": flat[0].n_tiles,
                     "ungrouped_bytes_home": int(K * (B + 1) * 8 + K * 32 + V * 9 + 32),
                     "ungrouped_warm_spread": [round(min(warm_flat), 3), round(max(warm_flat), 3)],
                     "ratio_products_best_warm": round(min(warm) / min(warm_flat), 4),
                     "ratio_products_median_warm": round(float(np.median(warm)) / float(np.median(warm_flat)), 4),
                     "ratio_beta_median_warm": round(float(np.median([q.ms_beta for q in runs[1:]])) / float(np.median([q.ms_beta for q in flat[1:]])), 4),
                     "groups_over_rows": round(G / K, 4),
                     "max_identity": bool(np.array_equal(gb, np.concatenate([ub, pad]).reshape(G, 4, B + 1).max(axis=1))),
                     "identical_every_time": bool(all(same_group(runs[0], q) for q in runs[1:]))})
        assert line["identical_every_time"], "two device runs differ"
        assert line["max_identity"], "a group is not the maximum of its members"
        if not a.no_host and fmas <= a.host_fmas:
            h = cohort.qtl_permute_grouped_host(ph, regions, groups, G, *tail, perms=perms)
            line.update({"ms_perm_host": round(h.ms_perm, 1), "ms_products_host": round(h.ms_products, 1), "ms_beta_host": round(h.ms_beta, 1),
                         "identical_to_host": bool(same_group(runs[0], h))})
            assert line["identical_to_host"], "the device's grouped pass differs from the host twin's"
            h.close()
        for q in runs + flat:
            q.close()
        print(json.dumps(line), flush=True)
    co.close()


def part_indep(a):
    """rgx_cohort_qtl_independent on --qtl's planted tables with --perms B permutations at p_beta <= --pval-indep: --reps calls, ms per phase, the
    rounds and the series; then the conditional pass alone at m = 1 and m = 8 over every row with at least nine cis variants, each conditioned on
    its first m, beside the permutation pass in the same process on the same inputs: ms_products of each and per tile of 64 x 64 products, which
    is what compares k_qtl_perm_cond with k_qtl_perm (the permutation pass walks every row's tiles, the conditional pass the series' rows')."""
    import regtools_amd
    from regtools_amd import cohort
    co = regtools_amd.Cohort(ctx=regtools_amd.Context(0))
    for size in [x for x in (a.planted or "64x4000x6000").split(",") if x]:
        S, K, V = [int(x) for x in size.lower().split("x")]
        t0 = time.time()
        ph, regions, pos, dosage, pcs, n_cov = planted_qtl_inputs(a, co, S, K, V)
        B = a.perms
        perms = cohort.qtl_permutations(S, B, 0)
        args = (ph, regions, np.zeros(V, np.uint32), pos, dosage, pcs.component if pcs else None, a.window)
        line = {"part": "indep", "samples": S, "rows": K, "variants": V, "n_cov": n_cov, "window": a.window, "perms": B, "p_threshold": a.pval_indep,
                "s_generate": round(time.time() - t0, 1)}
        runs = [co.qtl_independent(*args, perms=perms, p_threshold=a.pval_indep, max_signals=8) for _ in range(a.reps)]
        q = runs[0]
        line.update({"entered": q.n_entered, "forward_rounds": q.n_forward_rounds, "series": q.n_series_total, "signals": q.n_signals,
                     "capped": q.n_capped, "ms_indep": [round(r.ms_indep, 3) for r in runs], "ms_round0": [round(r.ms_round0, 3) for r in runs],
                     "ms_forward": [round(r.ms_forward, 3) for r in runs], "ms_backward": [round(r.ms_backward, 3) for r in runs]})
        nominal = co.qtl_nominal(*args)
        begin = nominal.pair_begin.astype(np.int64)
        rows = np.nonzero(np.diff(begin) >= 9)[0]
        first = np.stack([nominal.pair_variant[begin[rows] + j] for j in range(8)], axis=1) if len(rows) else np.zeros((0, 8), np.uint32)
        nominal.close()
        plain = [co.qtl_permute(*args, perms=perms) for _ in range(a.reps)]
        best = min(plain[1:] or plain, key=lambda r: r.ms_products)
        line.update({"perm_ms_products": [round(r.ms_products, 3) for r in plain], "perm_tiles": plain[0].n_tiles,
                     "perm_us_per_tile": round(1e3 * best.ms_products / max(plain[0].n_tiles, 1), 4)})
        for m in (1, 8):
            lists = (rows.astype(np.uint32), (np.arange(len(rows) + 1) * m).astype(np.uint32), np.ascontiguousarray(first[:, :m]).reshape(-1))
            cond = [co.qtl_permute_conditional(args[0], args[1], *lists, *args[2:], perms=perms) for _ in range(a.reps)] if len(rows) else []
            if not cond:
                continue
            cb = min(cond[1:] or cond, key=lambda r: r.ms_products)
            per_tile = 1e3 * cb.ms_products / max(cond[0].n_tiles, 1)
            line.update({"cond_m%d_series" % m: len(rows), "cond_m%d_ms_prepare" % m: [round(r.ms_prepare, 3) for r in cond],
                         "cond_m%d_ms_products" % m: [round(r.ms_products, 3) for r in cond], "cond_m%d_tiles" % m: cond[0].n_tiles,
                         "cond_m%d_us_per_tile" % m: round(per_tile, 4),
                         "cond_m%d_per_tile_over_perm" % m: round(per_tile / (1e3 * best.ms_products / max(plain[0].n_tiles, 1)), 3)})
            for r in cond:
                r.close()
        for r in plain:
            r.close()
        if not a.no_host and K * V * S * (B + 1) / 64 <= a.host_fmas:
            h = cohort.qtl_independent_host(*args, perms=perms, p_threshold=a.pval_indep, max_signals=8)
            same = (h.n_signals == q.n_signals and np.array_equal(h.sig_begin, q.sig_begin) and np.array_equal(h.variant, q.variant)
                    and np.array_equal(h.p_beta.view(np.uint64), q.p_beta.view(np.uint64)) and np.array_equal(h.r.view(np.uint64), q.r.view(np.uint64)))
            line.update({"ms_indep_host": round(h.ms_indep, 1), "identical_to_host": bool(same)})
            assert same, "the device's independent signals differ from the host twin's"
            h.close()
        for r in runs:
            r.close()
        print(json.dumps(line), flush=True)
    co.close()


def part_pipeline(a):
    import regtools_amd
    from regtools_amd import synth
    t0 = time.time()
    bam, bai, st = synth.generate(a.reads, shape="short", seed=1, threads=min(16, os.cpu_count() or 8))
    t_gen = time.time() - t0
    pin = regtools_amd.PinnedBuffer(bam)
    ctx = regtools_amd.Context(0)
    pl = regtools_amd.Pipeline(0, 2)

    def run(nf, co):
        """nf files, two in flight; file k is added (when there is a cohort) before file k + 2 is submitted.  Returns the seconds from the first
        submit to the last wait's return (bench.py's sustained pass).  An add is an enqueue; the finish that follows OUTSIDE the window drains the
        cohort's stream and shows that every append ran."""
        t = time.time()
        tickets = [pl.submit(bai_bytes=bai, host_ptr=pin.ptr, host_len=len(bam), strandness=0) for _ in range(min(2, nf))]
        rows = 0
        for k in range(nf):
            je = pl.wait(tickets[k])
            rows = je.table.contents.n
            if co is not None:
                co.add(je, "f%d" % len(co.add_paths))
            if k + 2 < nf:
                tickets.append(pl.submit(bai_bytes=bai, host_ptr=pin.ptr, host_len=len(bam), strandness=0))
        return time.time() - t, rows

    run(4, None)                                     # both contexts' first calls: their workspaces
    warm = regtools_amd.Cohort(ctx=ctx)
    run(4, warm)
    warm.finish().close(); warm.close()
    without, with_, paths, finish_ms, rows = [], [], [], [], 0
    for _ in range(a.reps):
        dt, rows = run(a.files, None)
        without.append(round(1e3 * dt / a.files, 3))
        co = regtools_amd.Cohort(ctx=ctx)
        dt, rows = run(a.files, co)
        with_.append(round(1e3 * dt / a.files, 3))
        paths.append(sum(co.add_paths))
        m = co.finish()                              # (outside the window; also proves every append ran)
        assert m.n_samples == a.files and m.n_triples > 0
        finish_ms.append(round(m.ms_finish, 3)); add_ms = m.ms_add_total
        m.close(); co.close()
    pl.close()
    overlap = min(with_) <= max(without) and min(without) <= max(with_)
    print(json.dumps({"part": "pipeline", "reads": st["n_reads"], "file_MB": round(len(bam) / 1e6, 1), "rows_per_file": int(rows), "files": a.files,
                      "in_flight": 2, "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES", ""), "s_generate": round(t_gen, 1),
                      "ms_per_file_without_cohort": without, "ms_per_file_with_cohort_add": with_, "ranges_overlap": bool(overlap),
                      "device_path_adds_per_run": paths, "ms_in_add_per_file_host": round(add_ms / a.files, 4), "ms_finish_of_the_run": finish_ms}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["all", "pipeline", "finish"])
    ap.add_argument("--cluster", action="store_true", help="the cluster part, alone")
    ap.add_argument("--refine", action="store_true", help="the refine part, alone")
    ap.add_argument("--pheno", action="store_true", help="the phenotype part, alone")
    ap.add_argument("--pcs", action="store_true", help="the principal component part, alone")
    ap.add_argument("--qtl", action="store_true", help="the sQTL scan part, alone")
    ap.add_argument("--perm", action="store_true", help="the sQTL permutation part, alone")
    ap.add_argument("--group", action="store_true", help="the grouped sQTL permutation part beside the ungrouped one, alone")
    ap.add_argument("--trans", action="store_true", help="the trans sQTL scan part beside the nominal scan's product kernel, alone")
    ap.add_argument("--indep", action="store_true", help="the conditionally independent signals beside the permutation pass, alone")
    ap.add_argument("--pval-indep", type=float, default=0.05, help="--indep: the threshold on the beta-approximated p")
    ap.add_argument("--pval", type=float, default=1e-5, help="--trans: the p-value threshold")
    ap.add_argument("--band", type=int, default=4, help="--trans: row blocks of a super-tile in the tile mapping (beside 0: no mapping)")
    ap.add_argument("--perms", type=int, default=1000, help="--perm: permutations")
    ap.add_argument("--host-fmas", type=float, default=2e11, help="--perm: the twin runs when its fused multiply-adds stay below this")
    ap.add_argument("--n-cov", type=int, default=10, help="--qtl: principal components taken as covariates (clipped to the samples less three)")
    ap.add_argument("--window", type=int, default=100000, help="--qtl: the cis window")
    ap.add_argument("--planted", default="", help="--pcs: planted tables, SAMPLESxROWS; --qtl: SAMPLESxROWSxVARIANTS; comma separated")
    ap.add_argument("--n-pcs", type=int, default=10, help="--pcs: components asked for (clipped to the table)")
    ap.add_argument("--pheno-params", default="4/10,0.005", help="num/den of the missing share, min_sd")
    ap.add_argument("--refine-params", default="100000,5,1/1000,2,30", help="max_intron,min_reads,num/den,min_rows,min_total")
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--files", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="64x100000:sparse,512x300000:shared", help="SAMPLESxROWS[:sparse|shared], comma separated")
    ap.add_argument("--no-host", action="store_true", help="skip rgx_cohort_merge_host / rgx_cohort_cluster_host (profiling runs)")
    a = ap.parse_args()
    if a.cluster:
        return part_cluster(a)
    if a.refine:
        return part_refine(a)
    if a.pheno:
        return part_pheno(a)
    if a.pcs:
        return part_pcs(a)
    if a.qtl:
        return part_qtl(a)
    if a.trans:
        return part_trans(a)
    if a.perm:
        return part_perm(a)
    if a.group:
        return part_group(a)
    if a.indep:
        return part_indep(a)
    if a.part in ("all", "pipeline"):
        part_pipeline(a)
    if a.part in ("all", "finish"):
        part_finish(a)


if __name__ == "__main__":
    main()
