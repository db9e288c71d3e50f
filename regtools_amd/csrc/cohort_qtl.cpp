// cohort_qtl.cpp -- the nominal cis-sQTL scan of the cohort's phenotype table: rgx_cohort_qtl_nominal (device), its host twin
// rgx_cohort_qtl_nominal_host, rgx_cohort_pheno_regions and the text (contract in include/regtools_amd.h; the nominal pass of FastQTL and
// tensorQTL, which the reference does not contain).  Device side: qtl_kernels.hip; arithmetic: qtl_core.h; t and p: qtl_stats.cpp.
//   QtlPrep (qtl_run.h, qtl_prep.cpp): inputs in HBM -> residuals Y, G row-major with yy, gg and the verdicts -> the usable variants compacted
//   -> Yt, Gt sample-major
//   NominalRun: per row its range of usable variants, per 64 rows the tiles -> ONE wait for P and the tile count
//   -> one workgroup per tile: r, slope, pair_variant -> per row the best pair -> the copies back
#include "qtl_run.h"

#include <cmath>

namespace {

rgx_qtl_result *qtl_alloc(uint64_t K, uint32_t S, uint32_t V, uint32_t n_cov, uint64_t P, bool pinned) {
    rgx_qtl_result *q = result_alloc<rgx_qtl_result>(pinned, [&](rgx_qtl_result &r, BlockTake &take) {
        take(r.yy, K); take(r.gg, V); take(r.r, P); take(r.slope, P); take(r.pair_begin, K + 1); take(r.pair_variant, P); take(r.best, K);
        take(r.variant_verdict, V);
    });
    if (q) { qtl_result_head(q, K, S, V, n_cov); q->n_pairs = P; }
    return q;
}

int too_many_pairs(uint64_t P, char *err, size_t errlen) {
    return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: %llu pairs of a row and a variant; the sQTL scan takes at most 2^32 - 2^16\n", (unsigned long long)P);
}

// The device run: QtlPrep's shared stages with the nominal scan's own behind them.  The scans of the rows' counts and of the tile counts land in
// the words it asked the row workspace for.
struct NominalRun : QtlPrep {
    Events<2> ev_pairs;                                        // products begin, best done
    uint64_t P = 0, n_tiles = 0;
    uint32_t *pair_begin = nullptr, *tile_begin = nullptr, *pair_variant = nullptr, *best = nullptr; double *r = nullptr, *slope = nullptr;

    NominalRun(rgx_cohort *co, const QtlArgs &a, char *err, size_t errlen)
        : QtlPrep(co, "qtl nominal", a, /*want_Yt=*/true, (size_t)a.ph->n_rows + 1 + (a.ph->n_rows + kQtlTile - 1) / kQtlTile + 1, err, errlen) {}

    // 4. the rows' ranges and the tiles; the call's one wait in front of its results: P, the tile count, the flags
    int plan() {
        pair_begin = own; tile_begin = own + K + 1;
        plan_launch();
        launch_scan_u32(count, pair_begin, K + 1, nullptr, tmp, st);
        launch_scan_u32(tile_count, tile_begin, n_blocks + 1, nullptr, tmp, st);
        uint64_t h[4];
        HIP_TRY(hipMemcpyAsync(h, head, 32, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        mark("plan");
        if (int rc = bad_flags((const uint32_t *)(h + 2), K, err, errlen)) return rc;
        P = h[0]; n_tiles = h[1];
        if (P > kQtlMaxPairs) return too_many_pairs(P, err, errlen);
        if (n_tiles > kQtlMaxTiles) return fail(err, errlen, RGX_ERR_ARG,
            "regtools_amd: %llu tiles of 64 rows and 64 variants; the sQTL scan takes at most 2^31 - 1 (rows far out of position order)\n",
            (unsigned long long)n_tiles);
        if (int rc = grow(co->qt_out, (size_t)P * 20 + (size_t)K * 4 + 256, "regtools_amd: no device memory for %llu pairs\n", (unsigned long long)P)) return rc;
        // first writers: r, slope, pair_variant k_qtl_pairs (every pair lies in one tile); best k_qtl_best (whole)
        Carve o = carve(co->qt_out);
        r = o.take<double>(P); slope = o.take<double>(P); pair_variant = o.u32(P); best = o.u32(K);
        CARVE_TRY(o, "sQTL pair");
        if (int rc = carved(o, "sQTL pair")) return rc;
        return RGX_OK;
    }
    // 5. one workgroup per tile, then a wave per row
    int pairs() {
        HIP_TRY(ev_pairs.create());
        HIP_TRY(hipEventRecord(ev_pairs[0], st));
        launch_qtl_pairs(Yt, ldy, Gt, ldg, S, K, (uint32_t)n_tiles, tile_begin, blk_lo, lo, count, pair_begin, yy, u_gg, u_var, r, slope, pair_variant, st);
        mark("pair products");
        launch_qtl_best(r, pair_begin, K, best, st);
        HIP_TRY(hipEventRecord(ev_pairs[1], st));
        mark("best pairs");
        return RGX_OK;
    }
    // 6. the copies back, one wait
    int finish(rgx_qtl_result **out) {
        rgx_qtl_result *q = qtl_alloc(K, S, V, a.n_cov, P, /*pinned=*/true);
        if (!q) { (void)hipStreamSynchronize(st); return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no memory for the result of %llu pairs\n",
            (unsigned long long)P); }
        CopyBack back{st};
        copy_back(back, q);
        back(q->pair_begin, pair_begin, ((size_t)K + 1) * 4); back(q->r, r, (size_t)P * 8); back(q->slope, slope, (size_t)P * 8);
        back(q->pair_variant, pair_variant, (size_t)P * 4); back(q->best, best, (size_t)K * 4);
        float ms_res = 0, ms_pr = 0;
        const int rc = wait(back, {{ev[0], ev[1], &ms_res}, {ev_pairs[0], ev_pairs[1], &ms_pr}}, "sQTL scan");
        if (rc != RGX_OK) { rgx_cohort_qtl_free(q); return rc; }
        count_verdicts(q);
        q->n_tiles = n_tiles;
        q->ms_residual = ms_res; q->ms_pairs = ms_pr; q->ms_qtl = now_ms() - t0;
        *out = q;
        return RGX_OK;
    }
};

}  // namespace

extern "C" void rgx_cohort_qtl_free(rgx_qtl_result *q) { result_free(q); }

extern "C" int rgx_cohort_pheno_regions(const rgx_cohort_matrix *m, const rgx_pheno_table *ph, rgx_qtl_region *out, char *err, size_t errlen) {
    if (!m || !ph || (ph->n_rows && (!out || !ph->row))) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_pheno_regions needs a matrix, a phenotype table and room\n");
    for (uint64_t k = 0; k < ph->n_rows; ++k) {
        const uint32_t i = ph->row[k];
        if (i >= m->n) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: row %u of the phenotype table is no row of a matrix of %llu\n", i,
            (unsigned long long)m->n);
        out[k].tid = m->tid[i]; out[k].start = m->start[i]; out[k].end = m->end[i];
    }
    return RGX_OK;
}

extern "C" int rgx_cohort_qtl_nominal(rgx_cohort *co, const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants,
                                      const uint32_t *var_tid, const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates,
                                      uint32_t window, rgx_qtl_result **out, char *err, size_t errlen) {
    if (!co || !ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_qtl_nominal needs a cohort and a phenotype table\n");
    *out = nullptr;
    std::lock_guard<std::mutex> lock(co->mu);
    QtlArgs a; int rc = qtl_args(a, ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, window, err, errlen);
    if (rc != RGX_OK) return rc;
    NominalRun run(co, a, err, errlen);
    rc = run.prepare();
    if (rc == RGX_OK) rc = run.plan();
    if (rc == RGX_OK) rc = run.pairs();
    if (rc == RGX_OK) rc = run.finish(out);
    return run.done(rc);
}

extern "C" int rgx_cohort_qtl_nominal_host(const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants, const uint32_t *var_tid,
                                           const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates, uint32_t window,
                                           rgx_qtl_result **out, char *err, size_t errlen) {
    if (!ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_qtl_nominal_host needs a phenotype table\n");
    *out = nullptr;
    const double t0 = now_ms();
    QtlArgs a; int rc = qtl_args(a, ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, window, err, errlen);
    if (rc != RGX_OK) return rc;
    QtlHost h;
    rc = qtl_host_prepare(a, h, err, errlen);
    if (rc != RGX_OK) return rc;
    const uint64_t K = ph->n_rows, P = h.P; const uint32_t S = ph->n_samples, V = n_variants;
    const std::vector<double> &Y = h.Y, &G = h.G, &yy = h.yy, &gg = h.gg;
    const std::vector<uint32_t> &u_var = h.u_var, &lo = h.lo, &cnt = h.cnt;
    if (P > kQtlMaxPairs) return too_many_pairs(P, err, errlen);
    rgx_qtl_result *q = qtl_alloc(K, S, V, n_cov, P, false);
    if (!q) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the result of %llu pairs\n", (unsigned long long)P);
    qtl_result_fill(q, h);
    uint32_t p = 0;
    for (uint64_t k = 0; k < K; ++k) {
        q->pair_begin[k] = p; q->best[k] = RGX_NO_PAIR;
        const double *y = Y.data() + k * S;
        uint64_t best_bits = 0;
        for (uint32_t i = 0; i < cnt[k]; ++i, ++p) {
            const uint32_t v = u_var[lo[k] + i]; const double *g = G.data() + (size_t)v * S;
            double acc = 0.0;
            for (uint32_t s = 0; s < S; ++s) acc = qtl_fma(y[s], g[s], acc);
            q->pair_variant[p] = v; q->r[p] = qtl_r(acc, yy[k], gg[v]); q->slope[p] = qtl_slope(acc, gg[v]);
            const uint64_t bits = qtl_abs_bits(q->r[p]);
            if (q->best[k] == RGX_NO_PAIR || bits > best_bits) { best_bits = bits; q->best[k] = p; }
        }
    }
    q->pair_begin[K] = p;
    count_verdicts(q);
    const double t1 = now_ms();
    q->ms_residual = h.t_pairs - h.t_res; q->ms_pairs = t1 - h.t_pairs; q->ms_qtl = t1 - t0;
    *out = q;
    return RGX_OK;
}

// ---- text ---------------------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t rgx_cohort_format_qtl(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_table *ph, const rgx_qtl_result *q,
                                        const uint32_t *var_pos, const char *const *variant_id, char *buf, size_t cap) {
    if (!qtl_text_args_ok(m, cl, ph, q, var_pos, variant_id)) return 0;
    return format_twice(buf, cap, [&](TextOut &o) {
        o.put("phenotype_id\tvariant_id\tdistance\tr\tslope\tslope_se\ttstat\tpval_nominal\tis_best\n");
        for (uint64_t k = 0; q && k < q->n_rows; ++k) {
            const uint32_t i = ph->row[k];
            for (uint32_t p = q->pair_begin[k]; p < q->pair_begin[k + 1]; ++p) {
                const uint32_t v = q->pair_variant[p];
                const double t = rgx_qtl_tstat(q->r[p], q->dof);
                put_intron_id(o, m, cl, i); o.put("\t", 1);
                o.put(variant_id[v]);
                o.fmt("\t%lld\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\t%d\n", (long long)var_pos[v] - (long long)m->start[i], q->r[p], q->slope[p],
                      q->slope[p] / t, t, rgx_qtl_pvalue(t, q->dof), q->best[k] == p ? 1 : 0);
            }
        }
    });
}
