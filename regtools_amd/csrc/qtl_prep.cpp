// qtl_prep.cpp -- what all four sQTL calls do first (contract in include/regtools_amd.h; declarations in qtl_run.h): the checks of the arguments,
// the host half -- the basis, dot64 and residual as a wave runs them, the twins' steps (1)-(6) -- and QtlPrep, the device stages every run begins
// with.  Device side: qtl_kernels.hip; arithmetic: qtl_core.h.
//   on the host, for the device path and the twin alike: the quantile table T and the orthonormal basis Q of intercept + covariates
//   rank2, T, Q, regions, variants and dosages in HBM -> residuals Y, G row-major with yy, gg and the verdicts -> the usable variants compacted
//   -> Yt (where wanted) and Gt sample-major -> per row its range of usable variants, per 64 rows the tiles: enqueued, no wait
#include "qtl_run.h"

#include <cmath>

// the arguments the host can judge, the same for the device and the twin
static int check_qtl(const QtlArgs &a, char *err, size_t errlen) {
    const uint64_t K = a.ph->n_rows; const uint32_t S = a.ph->n_samples;
    if (!K || K > 0x7fffffffull) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the sQTL scan needs a table of 1 to 2^31 - 1 rows; this one has %llu\n",
        (unsigned long long)K);
    if (a.V > 0x7fffffffu) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the sQTL scan takes at most 2^31 - 1 variants; %u were given\n", a.V);
    if (S > kQtlMaxSamples) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the sQTL scan takes at most %u samples; the table has %u\n",
        kQtlMaxSamples, S);
    if ((uint64_t)S < (uint64_t)a.n_cov + 3) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: %u samples leave no degree of freedom behind an intercept, %u covariates and the genotype\n", S, a.n_cov);
    if (!a.ph->rank2 || !a.regions || (a.V && (!a.var_tid || !a.var_pos || !a.dosage)) || (a.n_cov && !a.cov)) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: the sQTL scan needs ranks, regions, variants with dosages and the covariates it was told of\n");
    for (uint32_t v = 1; v < a.V; ++v) if (qtl_key(a.var_tid[v - 1], a.var_pos[v - 1]) > qtl_key(a.var_tid[v], a.var_pos[v])) return fail(err, errlen,
        RGX_ERR_ARG, "regtools_amd: variant %u (contig %u, position %u) lies in front of variant %u (contig %u, position %u)\n", v, a.var_tid[v],
        a.var_pos[v], v - 1, a.var_tid[v - 1], a.var_pos[v - 1]);
    return RGX_OK;
}
int qtl_args(QtlArgs &a, const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t V, const uint32_t *var_tid, const uint32_t *var_pos,
             const int8_t *dosage, uint32_t n_cov, const double *cov, uint32_t window, char *err, size_t errlen) {
    a = QtlArgs{ph, regions, V, var_tid, var_pos, dosage, n_cov, cov, window}; return check_qtl(a, err, errlen);
}
int bad_flags(const uint32_t *flag, uint64_t K, char *err, size_t errlen) {
    if (flag[kQtlFlagDosage]) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: a dosage is none of 0, 1, 2 and -1\n");
    if (flag[kQtlFlagRank]) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the phenotype table holds a rank2 outside 2 .. %llu\n",
        (unsigned long long)(2 * K));
    return RGX_OK;
}

// ---- the host part, shared by the device path and the twin ------------------------------------------------------------------------------------
// Q (C x S) = the orthonormal basis of the intercept and the covariates: modified Gram-Schmidt, each projection pass done twice
int qtl_basis(uint32_t S, uint32_t n_cov, const double *cov, std::vector<double> &Q, char *err, size_t errlen) {
    RGX_FP_EXACT
    const uint32_t C = n_cov + 1;
    Q.assign((size_t)C * S, 0.0);
    for (uint32_t j = 0; j < C; ++j) {
        double *v = Q.data() + (size_t)j * S;
        double b2 = 0.0;
        for (uint32_t s = 0; s < S; ++s) { v[s] = j ? cov[(size_t)(j - 1) * S + s] : 1.0; b2 += v[s] * v[s]; }
        for (int pass = 0; pass < 2; ++pass) for (uint32_t i = 0; i < j; ++i) {
            const double *q = Q.data() + (size_t)i * S;
            double d = 0.0;
            for (uint32_t s = 0; s < S; ++s) d += v[s] * q[s];
            for (uint32_t s = 0; s < S; ++s) v[s] = v[s] - d * q[s];
        }
        double v2 = 0.0;
        for (uint32_t s = 0; s < S; ++s) v2 += v[s] * v[s];
        const double norm = sqrt(v2);
        if (!(norm > 1e-10 * sqrt(b2))) return fail(err, errlen, RGX_ERR_ARG,
            "regtools_amd: covariate %u is a combination of the intercept and the covariates before it\n", j);
        for (uint32_t s = 0; s < S; ++s) v[s] = v[s] / norm;
    }
    return RGX_OK;
}

// the contract's dot64 and residual, as the wave runs them
double host_dot64(const double *a, const double *b, uint32_t S) {
    double P[64];
    for (uint32_t l = 0; l < 64; ++l) P[l] = 0.0;
    for (uint32_t s = 0; s < S; ++s) P[s % 64] = qtl_fma(a[s], b[s], P[s % 64]);
    for (uint32_t off = 32; off; off >>= 1) for (uint32_t l = 0; l < off; ++l) P[l] = qtl_add(P[l], P[l + off]);
    return P[0];
}
double host_residual(double *x, uint32_t S, const double *Q, uint32_t C) {
    for (uint32_t j = 0; j < C; ++j) {
        const double *q = Q + (size_t)j * S;
        const double d = host_dot64(x, q, S);
        for (uint32_t s = 0; s < S; ++s) x[s] = qtl_project(d, q[s], x[s]);
    }
    return host_dot64(x, x, S);
}

size_t qtl_host_threads() { return std::min<size_t>(16, std::max<size_t>(1, std::thread::hardware_concurrency())); }

// steps (1)-(6) of the contract on the host (qtl_run.h)
int qtl_host_prepare(const QtlArgs &a, QtlHost &h, char *err, size_t errlen) {
    const uint64_t K = a.ph->n_rows; const uint32_t S = a.ph->n_samples, V = a.V, C = a.n_cov + 1;
    std::vector<double> &T = h.T, &Q = h.Q, &Y = h.Y, &G = h.G, &yy = h.yy, &gg = h.gg; std::vector<uint8_t> &verdict = h.verdict;
    std::vector<uint32_t> &u_var = h.u_var, &lo = h.lo, &cnt = h.cnt; std::vector<uint64_t> &u_key = h.u_key;
    try {
        pheno_quantile_table(K, T);
        Y.resize((size_t)K * S); G.resize((size_t)V * S); yy.resize(K); gg.resize(V); verdict.resize(V); lo.resize(K); cnt.resize(K);
    } catch (const std::bad_alloc &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the residuals of %llu rows and %u variants\n",
        (unsigned long long)K, V); }
    const int rc = qtl_basis(S, a.n_cov, a.cov, Q, err, errlen);
    if (rc != RGX_OK) return rc;
    h.t_res = now_ms();
    uint32_t flag[2] = {0, 0};
    for (uint64_t k = 0; k < K; ++k) {
        double *x = Y.data() + k * S;
        for (uint32_t s = 0; s < S; ++s) {
            const uint32_t r = a.ph->rank2[k * S + s];
            if (!pca_rank_ok(r, K)) { flag[kQtlFlagRank] = 1; return bad_flags(flag, K, err, errlen); }
            x[s] = T[r - 2];
        }
        yy[k] = host_residual(x, S, Q.data(), C);
    }
    for (uint32_t v = 0; v < V; ++v) {
        const int8_t *row = a.dosage + (size_t)v * S; double *x = G.data() + (size_t)v * S;
        uint32_t n = 0, sum = 0; int mn = 3, mx = -1;
        for (uint32_t s = 0; s < S; ++s) {
            const int8_t d = row[s];
            if (!qtl_dosage_ok(d)) { flag[kQtlFlagDosage] = 1; return bad_flags(flag, K, err, errlen); }
            if (d < 0) continue;
            ++n; sum += (uint32_t)d; mn = std::min<int>(mn, d); mx = std::max<int>(mx, d);
        }
        if (!n || mn == mx) { gg[v] = 0.0; verdict[v] = 1; continue; }
        const double mean = qtl_mean(sum, n);
        for (uint32_t s = 0; s < S; ++s) x[s] = row[s] >= 0 ? (double)row[s] : mean;
        gg[v] = host_residual(x, S, Q.data(), C);
        verdict[v] = qtl_enough(gg[v], S) ? 0 : 2;
        if (!verdict[v]) { u_var.push_back(v); u_key.push_back(qtl_key(a.var_tid[v], a.var_pos[v])); }
    }
    h.t_pairs = now_ms();
    uint64_t &P = h.P; P = 0;
    for (uint64_t k = 0; k < K; ++k) {
        lo[k] = cnt[k] = 0;
        if (!qtl_enough(yy[k], S)) continue;
        const auto first = std::lower_bound(u_key.begin(), u_key.end(), qtl_key_first(a.regions[k].tid, a.regions[k].start, a.window));
        const auto last = std::upper_bound(u_key.begin(), u_key.end(), qtl_key_last(a.regions[k].tid, a.regions[k].end, a.window));
        if (last <= first) continue;
        lo[k] = (uint32_t)(first - u_key.begin()); cnt[k] = (uint32_t)(last - first); P += cnt[k];
    }
    return RGX_OK;
}

// ---- QtlPrep: the device stages every sQTL run begins with (qtl_run.h) -----------------------------------------------------------------------------
QtlPrep::QtlPrep(rgx_cohort *co_, const char *name_, const QtlArgs &a_, bool want_Yt_, size_t own_words_, char *err_, size_t errlen_)
    : CohortRun(co_, name_, err_, errlen_), a(a_), want_Yt(want_Yt_), own_words(own_words_), K((uint32_t)a_.ph->n_rows), S(a_.ph->n_samples),
      V(a_.V), C(a_.n_cov + 1), n_blocks((K + kQtlTile - 1) / kQtlTile), ldy((size_t)n_blocks * kQtlTile),
      ldg(((size_t)a_.V + kQtlTile - 1) / kQtlTile * kQtlTile + kQtlTile) {}

int QtlPrep::open() {
    if (int rc = enter()) return rc;
    try { pheno_quantile_table(K, T); }
    catch (const std::bad_alloc &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the %llu quantiles\n", (unsigned long long)(2ull * K - 1)); }
    if (int rc = qtl_basis(S, a.n_cov, a.cov, Q, err, errlen)) return rc;
    mark("quantile table + basis");
    HIP_TRY(ev.create());
    const size_t n_T = 2 * (size_t)K - 1, n_Q = (size_t)C * S, n_ks = (size_t)K * S, n_vs = (size_t)V * S;
    if (int rc = grow(co->qt_in, (n_T + n_Q) * 8 + (n_ks + 3 * (size_t)K + 2 * (size_t)V) * 4 + n_vs + 256,
              "regtools_amd: no device memory for a table of %u rows, %u variants and %u samples\n", K, V, S)) return rc;
    Carve u = carve(co->qt_in);                               // (every array written whole by its upload; vt, vp and the dosages have no bytes without variants)
    double *t_up = u.take<double>(n_T), *q_up = u.take<double>(n_Q);
    uint32_t *r_up = u.u32(n_ks), *g_up = u.u32(3 * (size_t)K), *vt_up = u.u32(V), *vp_up = u.u32(V); int8_t *d_up = u.take<int8_t>(n_vs);
    CARVE_TRY(u, "sQTL input");
    if (int rc = carved(u, "sQTL input")) return rc;
    const size_t n_scan = std::max<size_t>(std::max<size_t>((size_t)K + 1, V), (size_t)n_blocks + 1);
    if (int rc = grow(co->qt_rows, (n_ks + n_vs + K + 2 * (size_t)V) * 8 + (size_t)V * 8 + 32 +
                           (3 * (size_t)V + 2 * (size_t)K + 1 + 2 * (size_t)n_blocks + 1 + own_words + scan_tmp_words((uint32_t)n_scan)) * 4 + V + 256,
              "regtools_amd: no device memory for the residuals of %u rows and %u variants\n", K, V)) return rc;
    // first writers: Y, yy k_qtl_residual_pheno (whole); G k_qtl_residual_geno, but for the rows of constant variants, which are read only through
    // u_var; gg, usable, verdict the same kernel (whole); place the scan (whole); u_var, u_key, u_gg k_qtl_compact [0, U), the rest left and read
    // only below *n_usable or inside [lo, lo + count); head the memset below, then the scan (n_usable), the residual kernels (flags) and k_qtl_totals;
    // lo, count k_qtl_plan (whole, count[K] = 0); blk_lo, tile_count k_qtl_tiles (whole, tile_count[n_blocks] = 0); own: the deriving run's; tmp:
    // the scans' scratch, written by each scan in front of its reads
    Carve w = carve(co->qt_rows);
    Y = w.take<double>(n_ks); G = w.take<double>(n_vs); yy = w.take<double>(K); gg = w.take<double>(V); u_gg = w.take<double>(V);
    u_key = w.u64(V); head = w.u64(4);
    usable = w.u32(V); place = w.u32(V); u_var = w.u32(V); lo = w.u32(K); count = w.u32((size_t)K + 1);
    blk_lo = w.u32(n_blocks); tile_count = w.u32((size_t)n_blocks + 1); own = w.u32(own_words);
    tmp = w.u32(scan_tmp_words((uint32_t)n_scan)); verdict = w.u8(V);
    CARVE_TRY(w, "sQTL row");
    if (int rc = carved(w, "sQTL row")) return rc;
    const size_t ldy_used = want_Yt ? ldy : 0;
    if (int rc = grow(co->qt_t, (size_t)S * (ldy_used + ldg) * 8 + 256,
              "regtools_amd: no device memory for the sample-major residuals of %u rows and %u variants\n", K, V)) return rc;
    // first writers: Yt and Gt k_qtl_transpose, every word of S x ld with +0.0 in the pad columns
    Carve t = carve(co->qt_t);
    Yt = t.take<double>((size_t)S * ldy_used); Gt = t.take<double>((size_t)S * ldg);
    CARVE_TRY(t, "sQTL panel");
    if (int rc = carved(t, "sQTL panel")) return rc;
    HIP_TRY(hipEventRecord(ev[0], st));
    HIP_TRY(hipMemcpyAsync(r_up, a.ph->rank2, n_ks * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(t_up, T.data(), n_T * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(q_up, Q.data(), n_Q * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(g_up, a.regions, (size_t)K * 12, hipMemcpyHostToDevice, st));
    if (V) {
        HIP_TRY(hipMemcpyAsync(vt_up, a.var_tid, (size_t)V * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(vp_up, a.var_pos, (size_t)V * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_up, a.dosage, n_vs, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemsetAsync(head, 0, 32, st));
    d_T = t_up; d_Q = q_up; rank2 = r_up; regions = g_up; var_tid = vt_up; var_pos = vp_up; dosage = d_up;
    mark("inputs in HBM");
    return RGX_OK;
}
int QtlPrep::residuals() {
    launch_qtl_residual_pheno(rank2, d_T, K, S, d_Q, C, Y, yy, flag(), st);
    launch_qtl_residual_geno(dosage, V, S, d_Q, C, G, gg, verdict, usable, flag(), st);
    mark("residuals");
    return RGX_OK;
}
int QtlPrep::compact() {
    launch_scan_u32(usable, place, V, n_usable(), tmp, st);
    launch_qtl_compact(usable, place, V, var_tid, var_pos, gg, u_var, u_key, u_gg, st);
    if (want_Yt) launch_qtl_transpose(Y, nullptr, nullptr, K, S, ldy, Yt, st);
    launch_qtl_transpose(G, u_var, n_usable(), 0, S, ldg, Gt, st);
    HIP_TRY(hipEventRecord(ev[1], st));
    mark("compaction + transposes");
    return RGX_OK;
}
int QtlPrep::plan_launch() {
    launch_qtl_plan(regions, K, S, yy, u_key, n_usable(), a.window, lo, count, blk_lo, tile_count, (unsigned long long *)head, st);
    return RGX_OK;
}
int QtlPrep::wait(CopyBack &back, std::initializer_list<Interval> intervals, const char *where) {
    guards_back(back);
    hipError_t e_ = back.wait();
    for (const Interval &i : intervals) if (e_ == hipSuccess) e_ = hipEventElapsedTime(i.ms, i.from, i.to);
    if (e_ != hipSuccess) return fail(err, errlen, RGX_ERR_DEVICE, "HIP error %s in the %s\n", hipGetErrorString(e_), where);
    mark("copies");
    return guards_check();
}
