// cohort_qtl_trans.cpp -- the trans-sQTL scan of the cohort's phenotype table: rgx_cohort_qtl_trans (device), its host twin
// rgx_cohort_qtl_trans_host and the text (contract in include/regtools_amd.h; tensorQTL's map_trans, which the reference does not contain).
// Device side: qtl_trans_kernels.hip behind QtlPrep's shared stages (qtl_run.h, qtl_prep.cpp); arithmetic: qtl_core.h; rgx_qtl_r_threshold:
// qtl_stats.cpp.
//   QtlPrep: inputs in HBM -> residuals Y, G with yy, gg and the verdicts -> the usable variants compacted -> Yt, Gt sample-major
//   -> one workgroup per tile of 64 rows x 64 usable variants, ALL of them: its hits and its pairs that met -> the scans of the hits and of the
//   tiles with hits, H and n_tested as 64-bit sums -> ONE wait for H, n_tested, the hit tiles and the flags -> one workgroup per tile with hits:
//   (row, usable variant, r, slope) tile-major -> a stable sort on the row -> the hits in order, hit_begin -> the copies back
#include "qtl_run.h"

#include <cmath>

namespace {

struct TransArgs { double r_min; int exclude_cis; uint32_t exclude_window; uint64_t max_hits; };

rgx_qtl_trans_result *trans_alloc(uint64_t K, uint32_t S, uint32_t V, uint32_t n_cov, uint64_t H, bool pinned) {
    rgx_qtl_trans_result *q = result_alloc<rgx_qtl_trans_result>(pinned, [&](rgx_qtl_trans_result &r, BlockTake &take) {
        take(r.yy, K); take(r.gg, V); take(r.r, H); take(r.slope, H); take(r.hit_begin, K + 1); take(r.hit_variant, H); take(r.variant_verdict, V);
    });
    if (q) { qtl_result_head(q, K, S, V, n_cov); q->n_hits = H; }
    return q;
}

// what the host can judge of the trans scan's own arguments, the same for the device and the twin
int check_trans(const TransArgs &x, char *err, size_t errlen) {
    if (!(x.r_min >= 0.0 && x.r_min <= 1.0)) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the trans scan's r_min is %g, outside 0 .. 1\n", x.r_min);
    return RGX_OK;
}
uint64_t hit_limit(const TransArgs &x) { return x.max_hits && x.max_hits < kQtlMaxPairs ? x.max_hits : kQtlMaxPairs; }
int too_many_hits(uint64_t H, uint64_t limit, char *err, size_t errlen) {
    return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: %llu pairs reach the threshold; the trans scan was told to keep at most %llu\n",
                (unsigned long long)H, (unsigned long long)limit);
}

// The device run: QtlPrep's shared stages with the trans scan's own behind them.
struct TransRun : QtlPrep {
    TransArgs x;
    Events<3> ev_hits;                                         // totals done, emit begins, hits in order
    uint32_t n_vt = 0, n_tiles = 0, n_hit_tiles = 0, band = 4;
    uint64_t H = 0, n_tested = 0;
    QtlTransTiles tiles{};
    unsigned long long *totals = nullptr;
    uint32_t *tile_hits = nullptr, *tile_tested = nullptr, *tile_flag = nullptr, *tile_off = nullptr, *tile_place = nullptr, *hit_tile = nullptr,
             *n_hit = nullptr, *tile_tmp = nullptr;
    double *r = nullptr, *slope = nullptr; uint32_t *hit_variant = nullptr, *hit_begin = nullptr;

    TransRun(rgx_cohort *co, const QtlArgs &a, const TransArgs &x_, char *err, size_t errlen)
        : QtlPrep(co, "qtl trans", a, /*want_Yt=*/true, 0, err, errlen), x(x_) {}

    // 4. every tile's hits, the scans and the totals; the call's one wait in front of its results
    int count() {
        n_vt = (V + kQtlTile - 1) / kQtlTile;
        if ((uint64_t)n_blocks * n_vt > kQtlMaxTiles) return fail(err, errlen, RGX_ERR_ARG,
            "regtools_amd: %llu tiles of 64 rows and 64 variants; the trans scan takes at most 2^31 - 1\n", (unsigned long long)n_blocks * n_vt);
        n_tiles = n_blocks * n_vt;
        if (const char *b = getenv("REGTOOLS_AMD_TRANS_BAND")) band = (uint32_t)std::min(64l, std::max(0l, atol(b)));
        HIP_TRY(ev_hits.create());
        const size_t n_tmp = scan_tmp_words(n_tiles);
        if (int rc = grow(co->qx_tiles, 64 + (6 * (size_t)n_tiles + 2 + n_tmp) * 4 + 256,
                          "regtools_amd: no device memory for %u tiles of the trans scan\n", n_tiles)) return rc;
        // first writers: totals k_qtl_trans_totals (words 0 .. 4; 5 .. 7 left, never read); tile_hits, tile_tested, tile_flag k_qtl_trans_count
        // (one workgroup per tile through trans_tile_of, a tile behind the last usable variant gets three zeros); tile_place, tile_off the scans
        // (whole); hit_tile k_qtl_trans_hit_tiles [0, *n_hit), the rest left and not read: the emit's grid is *n_hit; n_hit[0] the scan, n_hit[1]
        // left, never read; tile_tmp: the scans' scratch
        Carve w = carve(co->qx_tiles);
        totals = (unsigned long long *)w.u64(8);
        tile_hits = w.u32(n_tiles); tile_tested = w.u32(n_tiles); tile_flag = w.u32(n_tiles); tile_off = w.u32(n_tiles); tile_place = w.u32(n_tiles);
        hit_tile = w.u32(n_tiles); n_hit = w.u32(2); tile_tmp = w.u32(n_tmp);
        CARVE_TRY(w, "trans sQTL tile");
        if (int rc = carved(w, "trans sQTL tile")) return rc;
        uint64_t r_min_bits = qtl_abs_bits(x.r_min);
        tiles = QtlTransTiles{Yt, ldy, Gt, ldg, S, K, n_blocks, n_vt, regions, yy, u_gg, u_key,
                              n_usable(), r_min_bits, x.exclude_cis ? 1u : 0u, x.exclude_window};
        launch_qtl_trans_count(tiles, band, tile_hits, tile_tested, tile_flag, st);
        mark("tile counts");
        launch_scan_u32(tile_flag, tile_place, n_tiles, n_hit, tile_tmp, st);
        launch_qtl_trans_hit_tiles(tile_flag, tile_place, n_tiles, hit_tile, st);
        launch_scan_u32(tile_hits, tile_off, n_tiles, nullptr, tile_tmp, st);
        launch_qtl_trans_totals(tile_hits, tile_tested, n_tiles, n_hit, flag(), n_usable(), totals, st);
        HIP_TRY(hipEventRecord(ev_hits[0], st));
        uint64_t h[5];
        HIP_TRY(hipMemcpyAsync(h, totals, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        mark("scans + totals");
        if (int rc = bad_flags((const uint32_t *)(h + 3), K, err, errlen)) return rc;
        H = h[0]; n_tested = h[1]; n_hit_tiles = (uint32_t)h[2];
        if (H > hit_limit(x)) return too_many_hits(H, hit_limit(x), err, errlen);
        return RGX_OK;
    }
    // 5. the tiles with hits again, then the hits in the contract's order
    int emit() {
        const uint32_t n = (uint32_t)H;
        uint32_t row_bits = 0;
        while (row_bits < 32 && (K - 1) >> row_bits) ++row_bits;
        const size_t n_rtmp = row_bits ? radix_tmp_words(n) : 0;
        if (int rc = grow(co->qt_out, (size_t)H * (4 * 8 + 6 * 4) + ((size_t)K + 1 + n_rtmp) * 4 + 256, "regtools_amd: no device memory for %llu hits\n",
                            (unsigned long long)H)) return rc;
        // first writers: hit_row, hit_u, hit_r, hit_slope k_qtl_trans_emit (every hit has one place); perm the radix passes; row_sorted,
        // hit_variant, r, slope k_qtl_trans_gather (whole); hit_begin k_qtl_trans_begin (whole); rtmp: the passes' scratch
        Carve o = carve(co->qt_out);
        double *hit_r = o.take<double>(H), *hit_slope = o.take<double>(H);
        r = o.take<double>(H); slope = o.take<double>(H);
        uint32_t *hit_row = o.u32(H), *hit_u = o.u32(H), *perm[2] = {o.u32(H), o.u32(H)}, *row_sorted = o.u32(H);
        hit_variant = o.u32(H); hit_begin = o.u32((size_t)K + 1);
        uint32_t *rtmp = o.u32(n_rtmp);
        CARVE_TRY(o, "trans sQTL hit");
        if (int rc = carved(o, "trans sQTL hit")) return rc;
        HIP_TRY(hipEventRecord(ev_hits[1], st));
        launch_qtl_trans_emit(tiles, hit_tile, n_hit_tiles, tile_off, hit_row, hit_u, hit_r, hit_slope, st);
        mark("hit tiles");
        // tile-major, and inside a row the tiles come in ascending variant order: a stable sort on the row alone gives the contract's order
        const uint32_t *order = nullptr;
        for (uint32_t shift = 0, pass = 0; shift < row_bits; shift += 8, ++pass) {
            launch_radix_pass(hit_row, shift, std::min(8u, row_bits - shift), order, perm[pass & 1], n, rtmp, st);
            order = perm[pass & 1];
        }
        launch_qtl_trans_order(order, n, hit_row, hit_u, hit_r, hit_slope, u_var, K, row_sorted, hit_variant, r, slope, hit_begin, st);
        HIP_TRY(hipEventRecord(ev_hits[2], st));
        mark("hits in order");
        return RGX_OK;
    }
    // 6. the copies back, one wait
    int finish(rgx_qtl_trans_result **out) {
        rgx_qtl_trans_result *q = trans_alloc(K, S, V, a.n_cov, H, /*pinned=*/true);
        if (!q) { (void)hipStreamSynchronize(st); return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no memory for the result of %llu hits\n",
            (unsigned long long)H); }
        CopyBack back{st};
        copy_back(back, q);
        back(q->hit_begin, hit_begin, ((size_t)K + 1) * 4); back(q->hit_variant, hit_variant, (size_t)H * 4); back(q->r, r, (size_t)H * 8);
        back(q->slope, slope, (size_t)H * 8);
        float ms_res = 0, ms_count = 0, ms_emit = 0;
        const int rc = wait(back, {{ev[0], ev[1], &ms_res}, {ev[1], ev_hits[0], &ms_count}, {ev_hits[1], ev_hits[2], &ms_emit}}, "trans sQTL scan");
        if (rc != RGX_OK) { rgx_cohort_qtl_trans_free(q); return rc; }
        count_verdicts(q);
        q->n_tested = n_tested; q->n_tiles = n_tiles; q->n_hit_tiles = n_hit_tiles;
        q->ms_residual = ms_res; q->ms_count = ms_count; q->ms_emit = ms_emit; q->ms_trans = now_ms() - t0;
        *out = q;
        return RGX_OK;
    }
};

}  // namespace

extern "C" void rgx_cohort_qtl_trans_free(rgx_qtl_trans_result *q) { result_free(q); }

extern "C" int rgx_cohort_qtl_trans(rgx_cohort *co, const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants,
                                    const uint32_t *var_tid, const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates,
                                    double r_min, int exclude_cis, uint32_t exclude_window, uint64_t max_hits, rgx_qtl_trans_result **out, char *err,
                                    size_t errlen) {
    if (!co || !ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_qtl_trans needs a cohort and a phenotype table\n");
    *out = nullptr;
    std::lock_guard<std::mutex> lock(co->mu);
    QtlArgs a; const TransArgs x{r_min, exclude_cis, exclude_window, max_hits};
    int rc = qtl_args(a, ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, exclude_window, err, errlen);
    if (rc == RGX_OK) rc = check_trans(x, err, errlen);
    if (rc != RGX_OK) return rc;
    TransRun t(co, a, x, err, errlen);
    rc = t.prepare();
    if (rc == RGX_OK) rc = t.count();
    if (rc == RGX_OK) rc = t.emit();
    if (rc == RGX_OK) rc = t.finish(out);
    return t.done(rc);
}

extern "C" int rgx_cohort_qtl_trans_host(const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants, const uint32_t *var_tid,
                                         const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates, double r_min,
                                         int exclude_cis, uint32_t exclude_window, uint64_t max_hits, rgx_qtl_trans_result **out, char *err,
                                         size_t errlen) {
    if (!ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_qtl_trans_host needs a phenotype table\n");
    *out = nullptr;
    const double t0 = now_ms();
    QtlArgs a; const TransArgs x{r_min, exclude_cis, exclude_window, max_hits};
    int rc = qtl_args(a, ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, exclude_window, err, errlen);
    if (rc == RGX_OK) rc = check_trans(x, err, errlen);
    if (rc != RGX_OK) return rc;
    QtlHost h;
    rc = qtl_host_prepare(a, h, err, errlen);
    if (rc != RGX_OK) return rc;
    const uint64_t K = ph->n_rows, r_min_bits = qtl_abs_bits(r_min); const uint32_t S = ph->n_samples, V = n_variants, U = (uint32_t)h.u_var.size();
    struct Hit { uint32_t v; double r, slope; };
    std::vector<std::vector<Hit>> hits;
    std::vector<uint64_t> met;
    try {
        hits.resize(K); met.assign(K, 0);
        WorkerPool pool(K * (uint64_t)U * S < (1u << 20) ? 1 : qtl_host_threads());
        pool.run((size_t)K, [&](size_t k) {
            if (!qtl_enough(h.yy[k], S)) return;
            const rgx_qtl_region &g = regions[k];
            const double *y = h.Y.data() + k * S;
            // eight variants side by side, each its own chain in ascending s: the same bits as one after the other, with the FMAs overlapping
            constexpr uint32_t kSide = 8;
            for (uint32_t u0 = 0; u0 < U; u0 += kSide) {
                const uint32_t n = std::min(kSide, U - u0);
                const double *x8[kSide]; double acc[kSide];
                for (uint32_t j = 0; j < kSide; ++j) { x8[j] = h.G.data() + (size_t)h.u_var[u0 + (j < n ? j : 0)] * S; acc[j] = 0.0; }
                for (uint32_t s = 0; s < S; ++s) for (uint32_t j = 0; j < kSide; ++j) acc[j] = qtl_fma(y[s], x8[j][s], acc[j]);
                for (uint32_t j = 0; j < n; ++j) {
                    const uint32_t v = h.u_var[u0 + j];
                    if (exclude_cis && qtl_key_is_cis(h.u_key[u0 + j], g.tid, g.start, g.end, exclude_window)) continue;
                    ++met[k];
                    const double r = qtl_r(acc[j], h.yy[k], h.gg[v]);
                    if (qtl_abs_bits(r) >= r_min_bits) hits[k].push_back(Hit{v, r, qtl_slope(acc[j], h.gg[v])});
                }
            }
        });
    } catch (const std::exception &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory or threads for the trans scan\n"); }
    uint64_t H = 0, n_tested = 0;
    for (uint64_t k = 0; k < K; ++k) { H += hits[k].size(); n_tested += met[k]; }
    if (H > hit_limit(x)) return too_many_hits(H, hit_limit(x), err, errlen);
    rgx_qtl_trans_result *q = trans_alloc(K, S, V, n_cov, H, false);
    if (!q) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the result of %llu hits\n", (unsigned long long)H);
    qtl_result_fill(q, h);
    uint32_t p = 0;
    for (uint64_t k = 0; k < K; ++k) {
        q->hit_begin[k] = p;
        for (const Hit &hit : hits[k]) { q->hit_variant[p] = hit.v; q->r[p] = hit.r; q->slope[p] = hit.slope; ++p; }
    }
    q->hit_begin[K] = p;
    count_verdicts(q);
    q->n_tested = n_tested;
    const double t1 = now_ms();
    q->ms_residual = h.t_pairs - h.t_res; q->ms_count = t1 - h.t_pairs; q->ms_trans = t1 - t0;
    *out = q;
    return RGX_OK;
}

// ---- text ---------------------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t rgx_cohort_format_qtl_trans(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_table *ph,
                                              const rgx_qtl_trans_result *q, const uint32_t *var_pos, const char *const *variant_id, char *buf,
                                              size_t cap) {
    if (!qtl_text_args_ok(m, cl, ph, q, var_pos, variant_id)) return 0;
    return format_twice(buf, cap, [&](TextOut &o) {
        o.put("phenotype_id\tvariant_id\tr\tslope\tslope_se\ttstat\tpval\n");
        for (uint64_t k = 0; q && k < q->n_rows; ++k) {
            const uint32_t i = ph->row[k];
            for (uint32_t p = q->hit_begin[k]; p < q->hit_begin[k + 1]; ++p) {
                const double t = rgx_qtl_tstat(q->r[p], q->dof);
                put_intron_id(o, m, cl, i); o.put("\t", 1);
                o.put(variant_id[q->hit_variant[p]]);
                o.fmt("\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\n", q->r[p], q->slope[p], q->slope[p] / t, t, rgx_qtl_pvalue(t, q->dof));
            }
        }
    });
}
