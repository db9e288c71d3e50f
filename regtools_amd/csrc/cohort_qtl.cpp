// cohort_qtl.cpp -- the nominal cis-sQTL scan of the cohort's phenotype table: rgx_cohort_qtl_nominal (device), its host twin
// rgx_cohort_qtl_nominal_host, the t and p functions, the text, and rgx_genotypes_load, which reads the dosages from a VCF or BCF (contract in
// include/regtools_amd.h; the nominal pass of FastQTL and tensorQTL, which the reference does not contain).  Device side: qtl_kernels.hip;
// arithmetic: qtl_core.h.
//   QtlRun, the device stages, is declared in qtl_run.h, which the permutation pass (cohort_qtl_perm.cpp) shares.
//   on the host, for the device path and the twin alike: the quantile table T and the orthonormal basis Q of intercept + covariates
//   rank2, T, Q, regions, variants and dosages in HBM -> residuals Y, G row-major with yy, gg and the verdicts -> the usable variants compacted
//   -> Yt, Gt sample-major -> per row its range of usable variants, per 64 rows the tiles -> ONE wait for P and the tile count
//   -> one workgroup per tile: r, slope, pair_variant -> per row the best pair -> the copies back
#include "qtl_run.h"

#include <cmath>

namespace {

rgx_qtl_result *qtl_alloc(uint64_t K, uint32_t S, uint32_t V, uint32_t n_cov, uint64_t P, bool pinned) {
    rgx_qtl_result *q = result_alloc<rgx_qtl_result>(pinned, [&](rgx_qtl_result &r, BlockTake &take) {
        take(r.yy, K); take(r.gg, V); take(r.r, P); take(r.slope, P); take(r.pair_begin, K + 1); take(r.pair_variant, P); take(r.best, K);
        take(r.variant_verdict, V);
    });
    if (!q) return nullptr;
    q->n_rows = K; q->n_samples = S; q->n_variants = V; q->n_cov = n_cov; q->dof = S - n_cov - 2; q->n_pairs = P;
    return q;
}

int too_many_pairs(uint64_t P, char *err, size_t errlen) {
    return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: %llu pairs of a row and a variant; the sQTL scan takes at most 2^32 - 2^16\n", (unsigned long long)P);
}

}  // namespace

// the arguments the host can judge, the same for the device and the twin
int check_qtl(const QtlArgs &a, char *err, size_t errlen) {
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

// steps (1)-(6) of the contract on the host (qtl_run.h)
int qtl_host_prepare(const QtlArgs &a, QtlHost &h, char *err, size_t errlen) {
    const rgx_pheno_table *ph = a.ph; const rgx_qtl_region *regions = a.regions; const uint32_t *var_tid = a.var_tid, *var_pos = a.var_pos;
    const int8_t *dosage = a.dosage; const uint32_t window = a.window;
    const uint64_t K = ph->n_rows; const uint32_t S = ph->n_samples, V = a.V, C = a.n_cov + 1;
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
            const uint32_t r = ph->rank2[k * S + s];
            if (!pca_rank_ok(r, K)) { flag[kQtlFlagRank] = 1; return bad_flags(flag, K, err, errlen); }
            x[s] = T[r - 2];
        }
        yy[k] = host_residual(x, S, Q.data(), C);
    }
    for (uint32_t v = 0; v < V; ++v) {
        const int8_t *row = dosage + (size_t)v * S; double *x = G.data() + (size_t)v * S;
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
        if (!verdict[v]) { u_var.push_back(v); u_key.push_back(qtl_key(var_tid[v], var_pos[v])); }
    }
    h.t_pairs = now_ms();
    uint64_t &P = h.P; P = 0;
    for (uint64_t k = 0; k < K; ++k) {
        lo[k] = cnt[k] = 0;
        if (!qtl_enough(yy[k], S)) continue;
        const auto first = std::lower_bound(u_key.begin(), u_key.end(), qtl_key_first(regions[k].tid, regions[k].start, window));
        const auto last = std::upper_bound(u_key.begin(), u_key.end(), qtl_key_last(regions[k].tid, regions[k].end, window));
        if (last <= first) continue;
        lo[k] = (uint32_t)(first - u_key.begin()); cnt[k] = (uint32_t)(last - first); P += cnt[k];
    }
    return RGX_OK;
}

// ---- the nominal scan's own stages of QtlRun (the shared ones: qtl_run.h) ---------------------------------------------------------------------
// 4. the rows' ranges and the tiles; the call's one wait in front of its results: P, the tile count, the flags
int QtlRun::plan() {
    plan_launch();
    launch_scan_u32(count, pair_begin, K + 1, nullptr, tmp, st);
    launch_scan_u32(tile_count, tile_begin, n_blocks + 1, nullptr, tmp, st);
    uint64_t h[4];
    HIP_TRY(hipMemcpyAsync(h, head, 32, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    mark("plan");
    const uint32_t *f = (const uint32_t *)(h + 2);
    const int rc = bad_flags(f, K, err, errlen);
    if (rc != RGX_OK) return rc;
    P = h[0]; n_tiles = h[1];
    if (P > kQtlMaxPairs) return too_many_pairs(P, err, errlen);
    if (n_tiles > kQtlMaxTiles) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: %llu tiles of 64 rows and 64 variants; the sQTL scan takes at most 2^31 - 1 (rows far out of position order)\n",
        (unsigned long long)n_tiles);
    if (co->qt_out.ensure((size_t)P * 20 + (size_t)K * 4 + 256) != hipSuccess) { (void)hipGetLastError();
        return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no device memory for %llu pairs\n", (unsigned long long)P); }
    Carve o(co->qt_out);
    r = o.take<double>(P); slope = o.take<double>(P); pair_variant = o.u32(P); best = o.u32(K);
    CARVE_TRY(o, "sQTL pair");
    return RGX_OK;
}
// 5. one workgroup per tile, then a wave per row
int QtlRun::pairs() {
    HIP_TRY(hipEventRecord(ev[2], st));
    launch_qtl_pairs(Yt, ldy, Gt, ldg, S, K, (uint32_t)n_tiles, tile_begin, blk_lo, lo, count, pair_begin, yy, u_gg, u_var, r, slope, pair_variant, st);
    mark("pair products");
    launch_qtl_best(r, pair_begin, K, best, st);
    HIP_TRY(hipEventRecord(ev[3], st));
    mark("best pairs");
    return RGX_OK;
}
// 6. the copies back, one wait
int QtlRun::finish(rgx_qtl_result **out) {
    rgx_qtl_result *q = qtl_alloc(K, S, V, a.n_cov, P, /*pinned=*/true);
    if (!q) { (void)hipStreamSynchronize(st); return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no memory for the result of %llu pairs\n",
        (unsigned long long)P); }
    CopyBack back{st};
    back(q->yy, yy, (size_t)K * 8); back(q->gg, gg, (size_t)V * 8); back(q->variant_verdict, verdict, V);
    back(q->pair_begin, pair_begin, ((size_t)K + 1) * 4); back(q->r, r, (size_t)P * 8); back(q->slope, slope, (size_t)P * 8);
    back(q->pair_variant, pair_variant, (size_t)P * 4); back(q->best, best, (size_t)K * 4);
    hipError_t e_ = back.wait();
    float ms_res = 0, ms_pr = 0;
    if (e_ == hipSuccess) e_ = hipEventElapsedTime(&ms_res, ev[0], ev[1]);
    if (e_ == hipSuccess) e_ = hipEventElapsedTime(&ms_pr, ev[2], ev[3]);
    if (e_ != hipSuccess) { rgx_cohort_qtl_free(q); return fail(err, errlen, RGX_ERR_DEVICE, "HIP error %s in the sQTL scan\n", hipGetErrorString(e_)); }
    mark("copies");
    count_verdicts(q);
    q->n_tiles = n_tiles;
    q->ms_residual = ms_res; q->ms_pairs = ms_pr; q->ms_qtl = now_ms() - t0;
    *out = q;
    return RGX_OK;
}

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
    const QtlArgs a{ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, window};
    int rc = check_qtl(a, err, errlen);
    if (rc != RGX_OK) return rc;
    QtlRun run(co, a, err, errlen);
    rc = run.open();
    if (rc == RGX_OK) rc = run.residuals();
    if (rc == RGX_OK) rc = run.compact();
    if (rc == RGX_OK) rc = run.plan();
    if (rc == RGX_OK) rc = run.pairs();
    if (rc == RGX_OK) rc = run.finish(out);
    if (rc != RGX_OK && run.st) (void)hipStreamSynchronize(run.st);   // (the uploads read the caller's arrays and this run's T and Q)
    return rc;
}

extern "C" int rgx_cohort_qtl_nominal_host(const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants, const uint32_t *var_tid,
                                           const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates, uint32_t window,
                                           rgx_qtl_result **out, char *err, size_t errlen) {
    if (!ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_qtl_nominal_host needs a phenotype table\n");
    *out = nullptr;
    const double t0 = now_ms();
    const QtlArgs a{ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, window};
    int rc = check_qtl(a, err, errlen);
    if (rc != RGX_OK) return rc;
    QtlHost h;
    rc = qtl_host_prepare(a, h, err, errlen);
    if (rc != RGX_OK) return rc;
    const uint64_t K = ph->n_rows, P = h.P; const uint32_t S = ph->n_samples, V = n_variants;
    const std::vector<double> &Y = h.Y, &G = h.G, &yy = h.yy, &gg = h.gg; const std::vector<uint8_t> &verdict = h.verdict;
    const std::vector<uint32_t> &u_var = h.u_var, &lo = h.lo, &cnt = h.cnt;
    if (P > kQtlMaxPairs) return too_many_pairs(P, err, errlen);
    rgx_qtl_result *q = qtl_alloc(K, S, V, n_cov, P, false);
    if (!q) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the result of %llu pairs\n", (unsigned long long)P);
    memcpy(q->yy, yy.data(), K * 8);
    if (V) { memcpy(q->gg, gg.data(), (size_t)V * 8); memcpy(q->variant_verdict, verdict.data(), V); }
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

// ---- t and p, on the host ---------------------------------------------------------------------------------------------------------------------------
extern "C" double rgx_qtl_tstat(double r, uint32_t dof) {
    RGX_FP_EXACT
    const double u = 1.0 - r * r;
    if (u <= 0.0) return copysign(INFINITY, r);
    return r * sqrt((double)dof / u);
}

// the continued fraction of the incomplete beta function (Lentz's method, modified: Thompson and Barnett 1986), in the widest type the host has
long double qtl_beta_cf(long double a, long double b, long double x) {
    const long double tiny = 1e-300L, eps = 1e-19L;
    long double c = 1.0L, d = 1.0L - (a + b) * x / (a + 1.0L);
    if (fabsl(d) < tiny) d = tiny;
    d = 1.0L / d;
    long double h = d;
    for (int m = 1; m <= 10000; ++m) {
        const long double m2 = 2.0L * m;
        long double num = m * (b - m) * x / ((a + m2 - 1.0L) * (a + m2));
        d = 1.0L + num * d; if (fabsl(d) < tiny) d = tiny;
        c = 1.0L + num / c; if (fabsl(c) < tiny) c = tiny;
        d = 1.0L / d; h *= d * c;
        num = -(a + m) * (a + b + m) * x / ((a + m2) * (a + m2 + 1.0L));
        d = 1.0L + num * d; if (fabsl(d) < tiny) d = tiny;
        c = 1.0L + num / c; if (fabsl(c) < tiny) c = tiny;
        d = 1.0L / d;
        const long double del = d * c;
        h *= del;
        if (fabsl(del - 1.0L) < eps) break;
    }
    return h;
}
namespace {
// Gamma(n / 2 + 1 / 2) / (Gamma(n / 2) Gamma(1 / 2)) = 1 / B(n / 2, 1 / 2), by the recurrence over n - 2 from n = 1 (1 / pi) or n = 2 (1 / 2)
long double inv_beta_half(uint32_t n) {
    long double v = n % 2 ? 1.0L / 3.14159265358979323846264338327950288L : 0.5L;
    for (uint32_t i = n % 2 ? 1 : 2; i < n; i += 2) v *= (long double)(i + 1) / (long double)i;       // (a -> a + 1 multiplies by (a + 1/2) / a, a = i / 2)
    return v;
}
}  // namespace

extern "C" double rgx_qtl_pvalue(double t, uint32_t dof) {
    if (t != t || !dof) return NAN;
    if (std::isinf(t)) return 0.0;
    if (t == 0.0) return 1.0;
    const long double n = dof, a = 0.5L * n, b = 0.5L, t2 = (long double)t * (long double)t;
    const long double x = n / (n + t2), y = t2 / (n + t2);             // (y = 1 - x without the cancellation)
    // x^a y^b / B(a, b), with log x = -log1p(t^2 / n)
    const long double front = expl(-a * log1pl(t2 / n)) * sqrtl(y) * inv_beta_half(dof);
    long double p;
    if (x < (a + 1.0L) / (a + b + 2.0L)) p = front * qtl_beta_cf(a, b, x) / a;
    else p = 1.0L - front * qtl_beta_cf(b, a, y) / b;
    return (double)(p < 0.0L ? 0.0L : p > 1.0L ? 1.0L : p);
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

// ---- genotypes from a VCF / BCF -------------------------------------------------------------------------------------------------------------------
namespace {
struct GenoBox { rgx_genotypes g; std::vector<uint32_t> tid, pos; std::vector<int8_t> dosage; std::vector<std::string> id; std::vector<char *> id_ptr; };

// the dosages of one record's GT values (kInts, v.count per file sample) for the cohort's samples; col[s] = the file's column of cohort sample s
void gt_dosages(const VcfValue &v, const std::vector<uint32_t> &col, int8_t *out) {
    const int32_t no_more = v.width == 1 ? -127 : v.width == 2 ? -32767 : INT32_MIN + 1;
    for (size_t s = 0; s < col.size(); ++s) {
        const int32_t *a = v.ints.data() + (size_t)col[s] * (size_t)v.count;
        int ploidy = 0, alt = 0; bool missing = false;
        for (; ploidy < v.count && a[ploidy] != no_more; ++ploidy) {
            const int32_t allele = (a[ploidy] >> 1) - 1;
            if (allele < 0 || allele > 1) missing = true; else alt += allele;
        }
        out[s] = ploidy == 2 && !missing ? (int8_t)alt : (int8_t)-1;
    }
}
}  // namespace

extern "C" void rgx_genotypes_free(rgx_genotypes *g) { delete (GenoBox *)g; }                  // g is the first member

extern "C" int rgx_genotypes_load(const char *path, const rgx_cohort_matrix *m, rgx_genotypes **out, char *err, size_t errlen) {
    if (!path || !m || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_genotypes_load needs a path and a matrix\n");
    *out = nullptr;
    try {
        VcfText vcf;
        const std::string why = vcf.load(path, /*annotating=*/false);
        if (!why.empty()) return fail(err, errlen, RGX_ERR_OPEN, "%s", why.c_str());
        const std::vector<std::string> &have = vcf.hdr.sample_names();
        std::unordered_map<std::string, uint32_t> column;
        for (size_t j = have.size(); j-- > 0;) column[have[j]] = (uint32_t)j;            // (the first of equal names)
        const uint32_t S = m->n_samples;
        std::vector<uint32_t> col(S);
        for (uint32_t s = 0; s < S; ++s) {
            auto it = column.find(m->sample_name[s]);
            if (it == column.end()) return fail(err, errlen, RGX_ERR_ARG, "Sample %s has no genotypes in %s\n", m->sample_name[s], path);
            col[s] = it->second;
        }
        std::unordered_map<std::string, uint32_t> contig;
        for (int32_t t = m->n_ref; t-- > 0;) contig[m->ref_name[t]] = (uint32_t)t;
        std::unique_ptr<GenoBox> box(new GenoBox());
        rgx_genotypes &g = box->g;
        memset(&g, 0, sizeof g);
        VcfDictionary h = vcf.hdr;
        h.silence();
        struct Kept { uint32_t tid, pos; std::string id; std::vector<int8_t> d; };
        std::vector<Kept> kept;
        for (size_t i = 0; i < vcf.recs.size(); ++i) {
            VcfRecord r;
            if (vcf.typed(i, h, r) != ReadResult::kOk) break;
            ++g.n_records;
            auto c = contig.find(vcf.recs[i].chrom);
            if (c == contig.end()) { ++g.n_unknown_contig; continue; }
            if (r.alleles.size() != 2) { ++g.n_multiallelic; continue; }
            const VcfValue *gt = nullptr;
            for (const VcfRecord::Tagged &f : r.fields) if (h.id_name(f.key) == "GT" && f.v.store == VcfValue::kInts && f.v.count > 0) gt = &f.v;
            if (!gt || (size_t)r.n_samples < have.size() || gt->ints.size() < have.size() * (size_t)gt->count) { ++g.n_no_gt; continue; }
            Kept k;
            k.tid = c->second; k.pos = vcf.recs[i].pos0 + 1;
            k.id = !r.id.empty() && r.id != "." ? r.id : vcf.recs[i].chrom + ":" + std::to_string(k.pos) + ":" + r.alleles[0] + ":" + r.alleles[1];
            k.d.resize(S);
            gt_dosages(*gt, col, k.d.data());
            kept.push_back(std::move(k));
        }
        std::vector<uint32_t> order(kept.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = (uint32_t)i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            return qtl_key(kept[a].tid, kept[a].pos) < qtl_key(kept[b].tid, kept[b].pos); });
        const size_t V = kept.size();
        box->tid.resize(V); box->pos.resize(V); box->dosage.resize(V * S); box->id.resize(V); box->id_ptr.resize(V);
        for (size_t v = 0; v < V; ++v) {
            Kept &k = kept[order[v]];
            box->tid[v] = k.tid; box->pos[v] = k.pos; box->id[v] = std::move(k.id); box->id_ptr[v] = &box->id[v][0];
            if (S) memcpy(box->dosage.data() + v * S, k.d.data(), S);
        }
        g.n_variants = (uint32_t)V; g.n_samples = S;
        g.tid = box->tid.data(); g.pos = box->pos.data(); g.dosage = box->dosage.data(); g.id = box->id_ptr.data();
        *out = &box.release()->g;
        return RGX_OK;
    } catch (const std::bad_alloc &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the genotypes of %s\n", path); }
}
