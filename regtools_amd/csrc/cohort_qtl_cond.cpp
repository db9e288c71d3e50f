// cohort_qtl_cond.cpp -- the conditional permutation pass of the cohort's cis-sQTL scan: rgx_cohort_qtl_permute_conditional (device) and its host
// twin rgx_cohort_qtl_permute_conditional_host (contract in include/regtools_amd.h; tensorQTL's map_independent and QTLtools' conditional pass
// build on such a pass; the reference does not contain one).  Device side: qtl_cond_kernels.hip behind QtlPrep's shared stages and PermRun's
// permutations in HBM (qtl_run.h); arithmetic: qtl_core.h; the beta approximation of one series: qtl_stats.cpp's qtl_series_finish.
//   QtlPrep: residuals Y, G -> usable variants -> Gt -> per row its range  |  PermRun: the permutations sample-major in HBM
//   -> the series in HBM, their places by a scan of the rows' counts -> a wave per series: basis z, y', yy', status -> a wave per place: beta, gg'
//   -> one workgroup per (series, 64 permutations): perm_r -> a wave per series: n_cis and the best pair of permutation 0
//   -> ONE wait, the copies back -> on the host: n_ge, p_perm, the beta approximation with the series' own dof
// The planes of beta and gg' are sized on the host from the variants cis to each row, usable or not -- at or above the device's count -- so the
// offsets need no count[] at home and the call keeps to one wait.
// Behind it in this file: the forward-backward pass, rgx_cohort_qtl_independent and its twin -- indep_run, the decisions, over ONE CondRun on the
// device (round 0 is PermRun's products and finish; every further round series_launch + finish) or over the two public host twins -- and the text.
#include "qtl_run.h"

#include <cmath>

double host_dot64(const double *a, const double *b, uint32_t S);                 // qtl_prep.cpp

namespace {

struct CondArgs { uint32_t N; const uint32_t *row, *begin, *var; uint32_t M; size_t cap; };

rgx_qtl_cond_result *cond_alloc(const QtlArgs &a, uint32_t B, const CondArgs &s, bool pinned) {
    const uint64_t K = a.ph->n_rows; const uint32_t V = a.V; const size_t N = s.N;
    rgx_qtl_cond_result *q = result_alloc<rgx_qtl_cond_result>(pinned, [&](rgx_qtl_cond_result &r, BlockTake &take) {
        take(r.yy, K); take(r.gg, V); take(r.yy_cond, N); take(r.perm_r, N * ((size_t)B + 1)); take(r.best_r, N); take(r.best_slope, N);
        take(r.p_perm, N); take(r.beta_shape1, N); take(r.beta_shape2, N); take(r.p_beta, N); take(r.series_row, N); take(r.cond_begin, N + 1);
        take(r.cond_variant, s.M); take(r.dof, N); take(r.n_window, N); take(r.n_cis, N); take(r.best_variant, N); take(r.n_ge, N);
        take(r.variant_verdict, V); take(r.cond_status, N); take(r.beta_status, N);
    });
    if (!q) return nullptr;
    q->n_rows = K; q->n_samples = a.ph->n_samples; q->n_variants = V; q->n_cov = a.n_cov; q->n_perm = B; q->n_series = s.N; q->n_cond = s.M;
    memcpy(q->series_row, s.row, N * 4);
    for (size_t c = 0; c <= N; ++c) q->cond_begin[c] = s.begin[c] - s.begin[0];
    if (s.M) memcpy(q->cond_variant, s.var + s.begin[0], (size_t)s.M * 4);
    for (size_t c = 0; c < N; ++c) q->dof[c] = q->n_samples - a.n_cov - 2 - (s.begin[c + 1] - s.begin[c]);
    return q;
}

// The series as the host can judge them, the same for the device and the twin; s.cap = the sum over the series of the variants cis to their row
int check_cond(const QtlArgs &a, uint32_t B, uint32_t n_series, const uint32_t *series_row, const uint32_t *cond_begin, const uint32_t *cond_variant,
               CondArgs &s, char *err, size_t errlen) {
    const uint64_t K = a.ph->n_rows; const uint32_t S = a.ph->n_samples, V = a.V;
    if (!n_series) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the conditional pass needs at least one series\n");
    if (!series_row || !cond_begin || !cond_variant) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: the conditional pass needs its series' rows and the variants they are conditioned on\n");
    if ((uint64_t)n_series * ((uint64_t)B + 1) > kQtlMaxPairs) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: %u series x %u permutations and the identity; the conditional pass takes at most 2^32 - 2^16 of them\n", n_series, B);
    std::vector<uint64_t> key;
    try { key.resize(V); }
    catch (const std::bad_alloc &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the keys of %u variants\n", V); }
    for (uint32_t v = 0; v < V; ++v) key[v] = qtl_key(a.var_tid[v], a.var_pos[v]);
    uint64_t cap = 0;
    for (uint32_t c = 0; c < n_series; ++c) {
        const uint32_t k = series_row[c], m = cond_begin[c + 1] - cond_begin[c];
        if (k >= K) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: series %u names row %u of a table of %llu rows\n", c, k, (unsigned long long)K);
        if (cond_begin[c + 1] < cond_begin[c] || !m || m > kQtlMaxCond) return fail(err, errlen, RGX_ERR_ARG,
            "regtools_amd: series %u is conditioned on %u variants; a series takes 1 to %u\n", c, m, kQtlMaxCond);
        if ((uint64_t)S < (uint64_t)a.n_cov + 3 + m) return fail(err, errlen, RGX_ERR_ARG,
            "regtools_amd: %u samples leave no degree of freedom behind an intercept, %u covariates, the %u variants of series %u and the genotype\n",
            S, a.n_cov, m, c);
        const rgx_qtl_region &g = a.regions[k];
        const uint32_t *cv = cond_variant + cond_begin[c];
        for (uint32_t j = 0; j < m; ++j) {
            if (cv[j] >= V) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: series %u is conditioned on variant %u of %u\n", c, cv[j], V);
            for (uint32_t i = 0; i < j; ++i) if (cv[i] == cv[j]) return fail(err, errlen, RGX_ERR_ARG,
                "regtools_amd: series %u is conditioned on variant %u twice\n", c, cv[j]);
            if (!qtl_key_is_cis(key[cv[j]], g.tid, g.start, g.end, a.window)) return fail(err, errlen, RGX_ERR_ARG,
                "regtools_amd: variant %u, which series %u is conditioned on, is not cis to its row %u\n", cv[j], c, k);
        }
        const uint32_t first = qtl_bound(key.data(), V, qtl_key_first(g.tid, g.start, a.window), false);
        const uint32_t last = qtl_bound(key.data(), V, qtl_key_last(g.tid, g.end, a.window), true);
        cap += last - first;                                 // (last > first: the conditioning variants lie between them)
    }
    if (cap > kQtlMaxPairs) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: the series' rows have %llu cis variants in all; the conditional pass takes at most 2^32 - 2^16\n", (unsigned long long)cap);
    s = CondArgs{n_series, series_row, cond_begin, cond_variant, cond_begin[n_series] - cond_begin[0], (size_t)cap};
    return RGX_OK;
}

int not_usable(uint32_t c, uint32_t v, bool known, char *err, size_t errlen) {
    if (known) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: variant %u, which series %u is conditioned on, is constant or explained by the covariates\n", v, c);
    return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: a variant a series is conditioned on is constant or explained by the covariates\n");
}

// the statistics, the tile count of the device, then qtl_series_finish for every series with its own dof, sixteen a task among the host's threads;
// q's arrays from steps (1)-(6), its lists, cond_status, n_window, n_cis, perm_r and best_* are in place
int cond_finish(rgx_qtl_cond_result *q, bool device, char *err, size_t errlen) {
    const uint64_t N = q->n_series; const uint32_t B = q->n_perm;
    count_verdicts(q);
    const uint64_t p_tiles = ((uint64_t)B + 1 + kQtlTile - 1) / kQtlTile;
    for (uint64_t c = 0; c < N; ++c) {
        q->n_collinear += q->cond_status[c] == 1; q->n_flat_series += q->cond_status[c] == 2; q->n_pairs += q->n_cis[c];
        if (device && !q->cond_status[c]) q->n_tiles += p_tiles * (((uint64_t)q->n_window[c] + kQtlTile - 1) / kQtlTile);
    }
    const double t0 = now_ms();
    try {
        WorkerPool pool(N * B < 4096 ? 1 : qtl_host_threads());
        const uint64_t chunk = 16, n_tasks = (N + chunk - 1) / chunk;
        pool.run((size_t)n_tasks, [&](size_t task) {
            std::vector<double> p(B);
            for (uint64_t c = task * chunk; c < N && c < (task + 1) * chunk; ++c)
                qtl_series_finish(q->perm_r + c * ((size_t)B + 1), B, q->best_r[c], q->dof[c], q->n_cis[c] != 0, p.data(), q->n_ge[c], q->p_perm[c],
                                  q->beta_shape1[c], q->beta_shape2[c], q->p_beta[c], q->beta_status[c]);
        });
    } catch (const std::exception &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory or threads for the beta approximation\n"); }
    q->ms_beta = now_ms() - t0;
    return RGX_OK;
}

// The twin's series c: the basis, the row, the places and the products.  Returns the variant that is not usable, or RGX_NO_PAIR
uint32_t cond_host_series(const QtlHost &h, uint32_t S, uint32_t B, const uint16_t *perm, const CondArgs &sr, uint32_t c, rgx_qtl_cond_result *q) {
    const uint32_t k = sr.row[c], m = sr.begin[c + 1] - sr.begin[c]; const uint32_t *cv = sr.var + sr.begin[c];
    double *series = q->perm_r + (size_t)c * ((size_t)B + 1);
    for (uint32_t b = 0; b <= B; ++b) series[b] = 0.0;
    q->cond_status[c] = 0; q->yy_cond[c] = 0.0; q->n_window[c] = h.cnt[k]; q->n_cis[c] = 0;
    q->best_variant[c] = RGX_NO_PAIR; q->best_r[c] = 0.0; q->best_slope[c] = 0.0;
    std::vector<double> z((size_t)m * S), x(S), y(S);
    for (uint32_t j = 0; j < m; ++j) {
        if (h.verdict[cv[j]]) return cv[j];
        memcpy(x.data(), h.G.data() + (size_t)cv[j] * S, (size_t)S * 8);
        for (int pass = 0; pass < 2; ++pass) for (uint32_t i = 0; i < j; ++i) {
            const double *zi = z.data() + (size_t)i * S;
            const double d = host_dot64(x.data(), zi, S);
            for (uint32_t s = 0; s < S; ++s) x[s] = qtl_project(d, zi[s], x[s]);
        }
        const double nn = host_dot64(x.data(), x.data(), S);
        if (!qtl_enough(nn, S)) { q->cond_status[c] = 1; return RGX_NO_PAIR; }
        for (uint32_t s = 0; s < S; ++s) z[(size_t)j * S + s] = qtl_unit(x[s], nn);
    }
    memcpy(y.data(), h.Y.data() + (size_t)k * S, (size_t)S * 8);
    for (uint32_t j = 0; j < m; ++j) {
        const double *zj = z.data() + (size_t)j * S;
        const double d = host_dot64(y.data(), zj, S);
        for (uint32_t s = 0; s < S; ++s) y[s] = qtl_project(d, zj[s], y[s]);
    }
    const double y2 = q->yy_cond[c] = host_dot64(y.data(), y.data(), S);
    if (!qtl_enough(y2, S)) { q->cond_status[c] = 2; return RGX_NO_PAIR; }
    // the places that take part: the input variant, gg' and the m betas
    std::vector<uint32_t> var; std::vector<double> g2, beta;
    for (uint32_t i = 0; i < h.cnt[k]; ++i) {
        const uint32_t v = h.u_var[h.lo[k] + i];
        double bt[kQtlMaxCond];
        memcpy(x.data(), h.G.data() + (size_t)v * S, (size_t)S * 8);
        for (uint32_t j = 0; j < m; ++j) {
            const double *zj = z.data() + (size_t)j * S;
            bt[j] = host_dot64(x.data(), zj, S);
            for (uint32_t s = 0; s < S; ++s) x[s] = qtl_project(bt[j], zj[s], x[s]);
        }
        const double ss = host_dot64(x.data(), x.data(), S);
        if (!qtl_enough(ss, S)) continue;
        var.push_back(v); g2.push_back(ss); beta.insert(beta.end(), bt, bt + m);
    }
    q->n_cis[c] = (uint32_t)var.size();
    std::vector<double> yp(S);
    uint64_t top0 = 0;
    for (uint32_t b = 0; b <= B && !var.empty(); ++b) {
        const uint16_t *pb = perm + (size_t)b * S;
        for (uint32_t s = 0; s < S; ++s) yp[s] = y[pb[s]];
        double alpha[kQtlMaxCond];
        for (uint32_t j = 0; j < m; ++j) {
            const double *zj = z.data() + (size_t)j * S;
            double acc = 0.0;
            for (uint32_t s = 0; s < S; ++s) acc = qtl_fma(yp[s], zj[s], acc);
            alpha[j] = acc;
        }
        uint64_t top = 0;
        for (size_t i = 0; i < var.size(); ++i) {            // in ascending variant order: a strictly larger |r| alone replaces
            const double *g = h.G.data() + (size_t)var[i] * S;
            double dot = 0.0;
            for (uint32_t s = 0; s < S; ++s) dot = qtl_fma(yp[s], g[s], dot);
            for (uint32_t j = 0; j < m; ++j) dot = qtl_project(alpha[j], beta[i * m + j], dot);
            const double r = qtl_r(dot, y2, g2[i]);
            const uint64_t bits = qtl_abs_bits(r);
            if (!b && (q->best_variant[c] == RGX_NO_PAIR || bits > top0)) {
                top0 = bits; q->best_variant[c] = var[i]; q->best_r[c] = r; q->best_slope[c] = qtl_slope(dot, g2[i]);
            }
            if (bits > top) top = bits;
        }
        memcpy(series + b, &top, 8);
    }
    return RGX_NO_PAIR;
}

// The device run: PermRun's stages up to the permutations in HBM, then the series' own
struct CondRun : PermRun {
    CondArgs sr; Events<3> ev_cond;                            // preparation begins, products begin, best done
    QtlCond d{}; uint32_t *cflag = nullptr, *d_best_u = nullptr, *d_best_variant = nullptr, *d_n_cis = nullptr, *d_n_window = nullptr;
    double *d_perm_r = nullptr, *d_best_r = nullptr, *d_best_slope = nullptr;
    std::vector<uint32_t> rel;                                  // cond_begin from 0, as the device and the result hold it

    CondRun(rgx_cohort *co, const QtlArgs &a, uint32_t B_, const uint16_t *perm_, const CondArgs &sr_, char *err, size_t errlen)
        : PermRun(co, a, B_, perm_, sr_.N, "series", nullptr, err, errlen), sr(sr_) { name = "qtl conditional"; }
    // (the forward-backward pass: PermRun's series are the table's rows, round 0; every later round sets sr)
    CondRun(rgx_cohort *co, const QtlArgs &a, uint32_t B_, const uint16_t *perm_, char *err, size_t errlen)
        : PermRun(co, a, B_, perm_, (uint32_t)a.ph->n_rows, "rows", nullptr, err, errlen), sr{} { name = "qtl independent"; }
    int launch() { int rc = prepare(); if (rc == RGX_OK) rc = plan_launch(); if (rc == RGX_OK) rc = stage_perms(); if (rc == RGX_OK) rc = series_launch(); return rc; }

    // the series in HBM, their places, the preparation, the products and the best pairs, enqueued: no wait
    int series_launch() {
        const size_t N = sr.N, M = sr.M, cap = sr.cap, n_out = N * ((size_t)B + 1), n_tmp = scan_tmp_words((uint32_t)N + 1);
        const char *no_memory = "regtools_amd: no device memory for %u conditional series, %zu places and %u permutations\n";
        if ((uint64_t)sr.N * (ldp / kQtlTile) > 0x7fffffffull) return fail(err, errlen, RGX_ERR_ARG,
            "regtools_amd: %u series x %zu blocks of 64 permutations are more than 2^31 - 1 workgroups\n", sr.N, ldp / kQtlTile);
        if (int rc = grow(co->qc_in, (2 * N + 1 + M) * 4 + 256, no_memory, sr.N, cap, B)) return rc;
        if (int rc = grow(co->qc_ws, ((N * kQtlMaxCond + N) * S + 3 * N + (kQtlMaxCond + 1) * cap + n_out) * 8 + (6 * N + 6 + n_tmp) * 4 + N + 256,
                          no_memory, sr.N, cap, B)) return rc;
        Carve in = carve(co->qc_in);                          // (every array written whole by its upload)
        uint32_t *row = in.u32(N), *begin = in.u32(N + 1), *var = in.u32(M);
        CARVE_TRY(in, "conditional series");
        if (int rc = carved(in, "conditional series")) return rc;
        // Cut anew by every round of the forward-backward pass; no round reads what the one before left.  First writers: z k_qtl_cond_basis, the
        // m vectors of a series that is not collinear (the rest left: every reader stops at m or at a status); yc, yyc, status the same kernel
        // (yc left for a collinear series, whose status keeps every reader away); beta, ggc k_qtl_cond_beta, the places [0, pb[N]) of series
        // with status 0 and the planes j < m (the rest left: the readers go by status and m); perm_r, best_u k_qtl_perm_cond (whole); best_r,
        // best_slope, best_variant, n_cis, n_window k_qtl_cond_best (whole); cnt k_qtl_cond_counts (whole, cnt[N] = 0); pb, total[0] the scan
        // (total[1] left, never read); cflag the memset below; scan_tmp: the scan's scratch
        Carve w = carve(co->qc_ws);
        d.N = sr.N; d.S = S; d.series_row = row; d.cond_begin = begin; d.cond_variant = var; d.lo = lo; d.count = count; d.u_var = u_var; d.cap = cap;
        d.z = w.take<double>(N * kQtlMaxCond * S); d.yc = w.take<double>(N * S); d.yyc = w.take<double>(N);
        d.beta = w.take<double>(kQtlMaxCond * cap); d.ggc = w.take<double>(cap);
        d_perm_r = w.take<double>(n_out); d_best_r = w.take<double>(N); d_best_slope = w.take<double>(N);
        uint32_t *cnt = w.u32(N + 1), *pb = w.u32(N + 1);
        d_best_u = w.u32(N); d_best_variant = w.u32(N); d_n_cis = w.u32(N); d_n_window = w.u32(N); cflag = w.u32(2);
        uint32_t *total = w.u32(2), *scan_tmp = w.u32(n_tmp);
        d.status = w.u8(N); d.pb = pb;
        CARVE_TRY(w, "conditional sQTL");
        if (int rc = carved(w, "conditional sQTL")) return rc;
        rel.resize(N + 1);
        for (size_t c = 0; c <= N; ++c) rel[c] = sr.begin[c] - sr.begin[0];
        HIP_TRY(hipMemcpyAsync(row, sr.row, N * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(begin, rel.data(), (N + 1) * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(var, sr.var + sr.begin[0], M * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(cflag, 0, 8, st));
        mark("series in HBM");
        if (!ev_cond[0]) { HIP_TRY(ev_cond.create()); }
        HIP_TRY(hipEventRecord(ev_cond[0], st));
        launch_qtl_cond_counts(d, cnt, st);
        launch_scan_u32(cnt, pb, (uint32_t)N + 1, total, scan_tmp, st);
        launch_qtl_cond_prepare(d, Y, G, verdict, cflag, st);
        mark("basis, rows, beta and gg'");
        HIP_TRY(hipEventRecord(ev_cond[1], st));
        launch_qtl_perm_cond(d, d_permT, ldp, B + 1, Gt, ldg, d_perm_r, d_best_u, st);
        mark("conditioned permuted products");
        launch_qtl_cond_best(d, G, d_best_u, d_best_variant, d_best_r, d_best_slope, d_n_cis, d_n_window, st);
        HIP_TRY(hipEventRecord(ev_cond[2], st));
        mark("best pairs");
        return RGX_OK;
    }

    // the copies back into q behind the call's ONE wait, then the host's part (cond_finish); q stays the caller's
    int finish(rgx_qtl_cond_result *q) {
        const size_t N = sr.N;
        uint64_t h[4] = {0, 0, 0, 0}; uint32_t cf[2] = {0, 0};
        CopyBack back{st};
        copy_back(back, q);
        back(q->perm_r, d_perm_r, N * ((size_t)B + 1) * 8); back(q->best_r, d_best_r, N * 8); back(q->best_slope, d_best_slope, N * 8);
        back(q->yy_cond, d.yyc, N * 8); back(q->best_variant, d_best_variant, N * 4); back(q->n_cis, d_n_cis, N * 4);
        back(q->n_window, d_n_window, N * 4); back(q->cond_status, d.status, N); back(h, head, 32); back(cf, cflag, 8);
        float ms_res = 0, ms_prep = 0, ms_pr = 0;
        int rc = wait(back, {{ev[0], ev[1], &ms_res}, {ev_cond[0], ev_cond[1], &ms_prep}, {ev_cond[1], ev_cond[2], &ms_pr}},
                      "conditional sQTL permutation pass (one wait: the places are sized on the host)");
        if (rc != RGX_OK) return rc;
        rc = bad_flags((const uint32_t *)(h + 2), K, err, errlen);
        if (rc == RGX_OK && cf[0]) rc = not_usable(0, 0, false, err, errlen);
        if (rc != RGX_OK) return rc;
        rc = cond_finish(q, /*device=*/true, err, errlen);
        if (rc != RGX_OK) return rc;
        q->ms_residual = ms_res; q->ms_prepare = ms_prep; q->ms_products = ms_pr; q->ms_cond = now_ms() - t0;
        return RGX_OK;
    }
};

}  // namespace

extern "C" void rgx_cohort_qtl_cond_free(rgx_qtl_cond_result *q) { result_free(q); }

extern "C" int rgx_cohort_qtl_permute_conditional(rgx_cohort *co, const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants,
                                                  const uint32_t *var_tid, const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov,
                                                  const double *covariates, uint32_t window, uint32_t n_perm, const uint16_t *perm, uint32_t n_series,
                                                  const uint32_t *series_row, const uint32_t *cond_begin, const uint32_t *cond_variant,
                                                  rgx_qtl_cond_result **out, char *err, size_t errlen) {
    if (!co || !ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_qtl_permute_conditional needs a cohort and a phenotype table\n");
    *out = nullptr;
    std::lock_guard<std::mutex> lock(co->mu);
    QtlArgs a; CondArgs s{};
    int rc = qtl_args(a, ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, window, err, errlen);
    if (rc == RGX_OK) rc = check_cond(a, n_perm, n_series, series_row, cond_begin, cond_variant, s, err, errlen);
    if (rc == RGX_OK) rc = check_perm(1, "series", ph->n_samples, n_perm, perm, err, errlen);
    if (rc != RGX_OK) return rc;
    CondRun p(co, a, n_perm, perm, s, err, errlen);
    rc = p.launch();
    rgx_qtl_cond_result *q = nullptr;
    if (rc == RGX_OK && !(q = cond_alloc(a, n_perm, s, /*pinned=*/true))) rc = p.no_result();
    if (rc == RGX_OK) rc = p.finish(q);
    if (p.done(rc) != RGX_OK) { rgx_cohort_qtl_cond_free(q); return rc; }
    *out = q;
    return RGX_OK;
}

extern "C" int rgx_cohort_qtl_permute_conditional_host(const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants,
                                                       const uint32_t *var_tid, const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov,
                                                       const double *covariates, uint32_t window, uint32_t n_perm, const uint16_t *perm,
                                                       uint32_t n_series, const uint32_t *series_row, const uint32_t *cond_begin,
                                                       const uint32_t *cond_variant, rgx_qtl_cond_result **out, char *err, size_t errlen) {
    if (!ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_qtl_permute_conditional_host needs a phenotype table\n");
    *out = nullptr;
    const double t0 = now_ms();
    QtlArgs a; CondArgs s{};
    int rc = qtl_args(a, ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, window, err, errlen);
    if (rc == RGX_OK) rc = check_cond(a, n_perm, n_series, series_row, cond_begin, cond_variant, s, err, errlen);
    if (rc == RGX_OK) rc = check_perm(1, "series", ph->n_samples, n_perm, perm, err, errlen);
    if (rc != RGX_OK) return rc;
    QtlHost h;
    rc = qtl_host_prepare(a, h, err, errlen);
    if (rc != RGX_OK) return rc;
    const uint32_t S = ph->n_samples, B = n_perm;
    rgx_qtl_cond_result *q = cond_alloc(a, B, s, false);
    if (!q) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the result of %u series and %u permutations\n", n_series, B);
    qtl_result_fill(q, h);
    std::vector<uint32_t> bad(s.N, RGX_NO_PAIR);
    try {
        WorkerPool pool((uint64_t)s.cap * ((uint64_t)B + 1) * S < (1u << 20) ? 1 : qtl_host_threads());
        pool.run(s.N, [&](size_t c) { bad[c] = cond_host_series(h, S, B, perm, s, (uint32_t)c, q); });
    } catch (const std::exception &) { rgx_cohort_qtl_cond_free(q); return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory or threads for the conditional pass\n"); }
    for (uint32_t c = 0; c < s.N; ++c) if (bad[c] != RGX_NO_PAIR) { rgx_cohort_qtl_cond_free(q); return not_usable(c, bad[c], true, err, errlen); }
    const double t1 = now_ms();
    rc = cond_finish(q, /*device=*/false, err, errlen);
    if (rc != RGX_OK) { rgx_cohort_qtl_cond_free(q); return rc; }
    q->ms_residual = h.t_pairs - h.t_res; q->ms_products = t1 - h.t_pairs; q->ms_cond = now_ms() - t0;
    *out = q;
    return RGX_OK;
}

// ---- the forward-backward pass --------------------------------------------------------------------------------------------------------------------
namespace {

struct Signal { uint32_t variant, rank, n_cond, dof, n_cis; double r, slope, p_perm, shape1, shape2, p_beta; uint8_t status; };
template <class R> Signal signal_of(const R *q, size_t i, uint32_t rank, uint32_t n_cond, uint32_t dof) {
    return {q->best_variant[i], rank, n_cond, dof, q->n_cis[i], q->best_r[i], q->best_slope[i], q->p_perm[i], q->beta_shape1[i], q->beta_shape2[i],
            q->p_beta[i], q->beta_status[i]};
}
// the contract's OK: pairs, a fit, and the fit's p at or below the threshold
template <class R> bool signal_ok(const R *q, size_t i, double p_threshold) {
    return q->n_cis[i] && q->beta_status[i] != 2 && q->p_beta[i] <= p_threshold;
}
struct SeriesLists {
    std::vector<uint32_t> row, begin{0}, var;
    void add(uint32_t k, const std::vector<uint32_t> &signals, size_t without) {
        row.push_back(k);
        for (size_t j = 0; j < signals.size(); ++j) if (j != without) var.push_back(signals[j]);
        begin.push_back((uint32_t)var.size());
    }
};
template <class R, void (*Free)(R *)> struct Holder { R *q = nullptr; ~Holder() { Free(q); } };

rgx_qtl_indep_result *indep_alloc(uint64_t K, size_t n) {
    return result_alloc<rgx_qtl_indep_result>(false, [&](rgx_qtl_indep_result &r, BlockTake &take) {
        take(r.r, n); take(r.slope, n); take(r.p_perm, n); take(r.beta_shape1, n); take(r.beta_shape2, n); take(r.p_beta, n);
        take(r.sig_begin, K + 1); take(r.variant, n); take(r.rank, n); take(r.n_cond, n); take(r.dof, n); take(r.n_cis, n);
        take(r.capped, K); take(r.beta_status, n);
    });
}

// The decisions of the contract, for the device path and the twin alike.  pass.perm(&q0) runs round 0; pass.cond(lists, &qc) one conditional pass.
template <class P> int indep_run(P &pass, const QtlArgs &a, uint32_t B, double p_threshold, uint32_t max_signals, rgx_qtl_indep_result **out,
                                 char *err, size_t errlen) {
    const double t0 = now_ms();
    const uint64_t K = a.ph->n_rows; const uint32_t S = a.ph->n_samples, room = S - a.n_cov - 3;
    Holder<rgx_qtl_perm_result, rgx_cohort_qtl_perm_free> first;
    int rc = pass.perm(&first.q);
    if (rc != RGX_OK) return rc;
    const rgx_qtl_perm_result *q0 = first.q;
    std::vector<std::vector<uint32_t>> fwd(K); std::vector<std::vector<Signal>> kept(K);
    std::vector<uint8_t> active(K, 0), capped(K, 0);
    uint64_t n_entered = 0, n_series_total = 0, n_capped = 0; uint32_t n_rounds = 0;
    auto settle = [&](uint64_t k) {                             // behind a new signal: another round, or capped
        const size_t n = fwd[k].size();
        active[k] = n < max_signals && n <= room;
        if (!active[k]) { capped[k] = 1; ++n_capped; }
    };
    for (uint64_t k = 0; k < K; ++k) if (signal_ok(q0, k, p_threshold)) { fwd[k].push_back(q0->best_variant[k]); ++n_entered; settle(k); }
    const double t1 = now_ms();
    for (;;) {
        SeriesLists l;
        for (uint64_t k = 0; k < K; ++k) if (active[k]) l.add((uint32_t)k, fwd[k], fwd[k].size());
        if (l.row.empty()) break;
        Holder<rgx_qtl_cond_result, rgx_cohort_qtl_cond_free> round;
        rc = pass.cond(l, &round.q);
        if (rc != RGX_OK) return rc;
        ++n_rounds; n_series_total += l.row.size();
        for (size_t c = 0; c < l.row.size(); ++c) {
            const uint32_t k = l.row[c];
            if (signal_ok(round.q, c, p_threshold)) { fwd[k].push_back(round.q->best_variant[c]); settle(k); }
            else active[k] = 0;
        }
    }
    const double t2 = now_ms();
    SeriesLists l;
    for (uint64_t k = 0; k < K; ++k) {
        if (fwd[k].size() == 1) kept[k].push_back(signal_of(q0, k, 1, 0, q0->dof));
        for (size_t i = 0; fwd[k].size() >= 2 && i < fwd[k].size(); ++i) l.add((uint32_t)k, fwd[k], i);
    }
    if (!l.row.empty()) {
        Holder<rgx_qtl_cond_result, rgx_cohort_qtl_cond_free> back;
        rc = pass.cond(l, &back.q);
        if (rc != RGX_OK) return rc;
        n_series_total += l.row.size();
        for (size_t c = 0, i = 0; c < l.row.size(); ++c) {
            const uint32_t k = l.row[c];
            i = c && l.row[c - 1] == k ? i + 1 : 0;
            if (!signal_ok(back.q, c, p_threshold)) continue;
            bool again = false;
            for (const Signal &s : kept[k]) again |= s.variant == back.q->best_variant[c];
            if (!again) kept[k].push_back(signal_of(back.q, c, (uint32_t)i + 1, (uint32_t)fwd[k].size() - 1, back.q->dof[c]));
        }
    }
    size_t n = 0;
    for (uint64_t k = 0; k < K; ++k) n += kept[k].size();
    if (n > 0xffffffffull) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: %zu signals are more than the result's 2^32 - 1\n", n);
    rgx_qtl_indep_result *q = indep_alloc(K, n);
    if (!q) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for %zu signals of %llu rows\n", n, (unsigned long long)K);
    q->n_rows = K; q->n_samples = S; q->n_variants = a.V; q->n_cov = a.n_cov; q->n_perm = B; q->max_signals = max_signals;
    q->p_threshold = p_threshold; q->n_signals = n; q->n_entered = n_entered; q->n_forward_rounds = n_rounds; q->n_series_total = n_series_total;
    q->n_capped = n_capped;
    size_t at = 0;
    for (uint64_t k = 0; k < K; ++k) {
        q->sig_begin[k] = (uint32_t)at; q->capped[k] = capped[k];
        for (const Signal &s : kept[k]) {
            q->variant[at] = s.variant; q->rank[at] = s.rank; q->n_cond[at] = s.n_cond; q->dof[at] = s.dof; q->n_cis[at] = s.n_cis; q->r[at] = s.r;
            q->slope[at] = s.slope; q->p_perm[at] = s.p_perm; q->beta_shape1[at] = s.shape1; q->beta_shape2[at] = s.shape2; q->p_beta[at] = s.p_beta;
            q->beta_status[at] = s.status; ++at;
        }
    }
    q->sig_begin[K] = (uint32_t)at;
    const double t3 = now_ms();
    q->ms_round0 = t1 - t0; q->ms_forward = t2 - t1; q->ms_backward = t3 - t2; q->ms_indep = t3 - t0;
    *out = q;
    return RGX_OK;
}

int check_indep(double p_threshold, uint32_t max_signals, char *err, size_t errlen) {
    if (!(p_threshold > 0.0 && p_threshold <= 1.0)) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: the threshold of the independent signals lies in (0, 1]; %g was given\n", p_threshold);
    if (!max_signals || max_signals > kQtlMaxCond) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: a row takes 1 to %u independent signals; %u were asked for\n", kQtlMaxCond, max_signals);
    return RGX_OK;
}

// the device's passes: ONE CondRun, its preparation and permutations shared by every round
struct DevicePasses {
    CondRun &p; const QtlArgs &a;
    int perm(rgx_qtl_perm_result **q) {
        int rc = p.prepare();
        if (rc == RGX_OK) rc = p.plan_launch();
        if (rc == RGX_OK) rc = p.products();
        if (rc == RGX_OK && !(*q = perm_alloc(a.ph->n_rows, a.ph->n_samples, a.V, a.n_cov, p.B, /*pinned=*/true))) rc = p.no_result();
        if (rc == RGX_OK) rc = p.PermRun::finish(*q);
        return rc;
    }
    int cond(const SeriesLists &l, rgx_qtl_cond_result **q) {
        int rc = check_cond(a, p.B, (uint32_t)l.row.size(), l.row.data(), l.begin.data(), l.var.data(), p.sr, p.err, p.errlen);
        if (rc == RGX_OK) rc = p.series_launch();
        if (rc == RGX_OK && !(*q = cond_alloc(a, p.B, p.sr, /*pinned=*/true))) rc = p.no_result();
        if (rc == RGX_OK) rc = p.finish(*q);
        return rc;
    }
};
struct HostPasses {
    const QtlArgs &a; uint32_t B; const uint16_t *perms; char *err; size_t errlen;
    int perm(rgx_qtl_perm_result **q) {
        return rgx_cohort_qtl_permute_host(a.ph, a.regions, a.V, a.var_tid, a.var_pos, a.dosage, a.n_cov, a.cov, a.window, B, perms, q, err, errlen);
    }
    int cond(const SeriesLists &l, rgx_qtl_cond_result **q) {
        return rgx_cohort_qtl_permute_conditional_host(a.ph, a.regions, a.V, a.var_tid, a.var_pos, a.dosage, a.n_cov, a.cov, a.window, B, perms,
                                                       (uint32_t)l.row.size(), l.row.data(), l.begin.data(), l.var.data(), q, err, errlen);
    }
};

}  // namespace

extern "C" void rgx_cohort_qtl_indep_free(rgx_qtl_indep_result *q) { result_free(q); }

extern "C" int rgx_cohort_qtl_independent(rgx_cohort *co, const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants,
                                          const uint32_t *var_tid, const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov,
                                          const double *covariates, uint32_t window, uint32_t n_perm, const uint16_t *perm, double p_threshold,
                                          uint32_t max_signals, rgx_qtl_indep_result **out, char *err, size_t errlen) {
    if (!co || !ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_qtl_independent needs a cohort and a phenotype table\n");
    *out = nullptr;
    std::lock_guard<std::mutex> lock(co->mu);
    QtlArgs a; int rc = qtl_args(a, ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, window, err, errlen);
    if (rc == RGX_OK) rc = check_perm(ph->n_rows, "rows", ph->n_samples, n_perm, perm, err, errlen);
    if (rc == RGX_OK) rc = check_indep(p_threshold, max_signals, err, errlen);
    if (rc != RGX_OK) return rc;
    CondRun p(co, a, n_perm, perm, err, errlen);
    DevicePasses pass{p, a};
    return p.done(indep_run(pass, a, n_perm, p_threshold, max_signals, out, err, errlen));
}

extern "C" int rgx_cohort_qtl_independent_host(const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants, const uint32_t *var_tid,
                                               const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates,
                                               uint32_t window, uint32_t n_perm, const uint16_t *perm, double p_threshold, uint32_t max_signals,
                                               rgx_qtl_indep_result **out, char *err, size_t errlen) {
    if (!ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_qtl_independent_host needs a phenotype table\n");
    *out = nullptr;
    QtlArgs a; int rc = qtl_args(a, ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, window, err, errlen);
    if (rc == RGX_OK) rc = check_perm(ph->n_rows, "rows", ph->n_samples, n_perm, perm, err, errlen);
    if (rc == RGX_OK) rc = check_indep(p_threshold, max_signals, err, errlen);
    if (rc != RGX_OK) return rc;
    HostPasses pass{a, n_perm, perm, err, errlen};
    return indep_run(pass, a, n_perm, p_threshold, max_signals, out, err, errlen);
}

// ---- text ---------------------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t rgx_cohort_format_qtl_indep(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_table *ph,
                                              const rgx_qtl_indep_result *q, const uint32_t *var_pos, const char *const *variant_id, char *buf,
                                              size_t cap) {
    if (!qtl_text_args_ok(m, cl, ph, q, var_pos, variant_id)) return 0;
    return format_twice(buf, cap, [&](TextOut &o) {
        o.put("phenotype_id\tnum_var\tbeta_shape1\tbeta_shape2\tdof\tvariant_id\tdistance\tr\tslope\tslope_se\ttstat\tpval_nominal\t"
              "pval_perm\tpval_beta\trank\tn_cond\n");
        for (uint64_t k = 0; q && k < q->n_rows; ++k) for (uint32_t s = q->sig_begin[k]; s < q->sig_begin[k + 1]; ++s) {
            const uint32_t i = ph->row[k], v = q->variant[s];
            const double t = rgx_qtl_tstat(q->r[s], q->dof[s]);
            put_intron_id(o, m, cl, i);
            o.fmt("\t%u\t", q->n_cis[s]);
            o.g17(q->beta_shape1[s], '\t'); o.g17(q->beta_shape2[s], '\t');
            o.fmt("%u\t", q->dof[s]);
            o.put(variant_id[v]);
            o.fmt("\t%lld\t", (long long)var_pos[v] - (long long)m->start[i]);
            o.g17(q->r[s], '\t'); o.g17(q->slope[s], '\t'); o.g17(q->slope[s] / t, '\t'); o.g17(t, '\t');
            o.g17(rgx_qtl_pvalue(t, q->dof[s]), '\t'); o.g17(q->p_perm[s], '\t'); o.g17(q->p_beta[s], '\t');
            o.fmt("%u\t%u\n", q->rank[s], q->n_cond[s]);
        }
    });
}
