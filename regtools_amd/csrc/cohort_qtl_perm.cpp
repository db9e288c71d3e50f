// cohort_qtl_perm.cpp -- the permutation pass of the cohort's cis-sQTL scan: rgx_cohort_qtl_permute (device), its host twin
// rgx_cohort_qtl_permute_host, rgx_qtl_permutations, the digamma, trigamma and incomplete beta functions, the beta fit and the text (contract in
// include/regtools_amd.h; FastQTL's --permute and tensorQTL's map_cis, which the reference does not contain).  Device side: qtl_perm_kernels.hip
// behind QtlRun's shared stages (qtl_run.h); arithmetic: qtl_core.h.  What is defined here over SERIES -- PermRun, perm_finish, the twin's
// qtl_series_products -- is the grouped pass's too (cohort_qtl_group.cpp), where a series is a group; here it is table row k alone.
//   QtlRun: inputs in HBM -> residuals Y, G with yy, gg and the verdicts -> the usable variants compacted -> Gt sample-major -> per row its range
//   -> the permutations sample-major in HBM -> one workgroup per (row, 64 permutations): perm_r -> a thread per row: the best pair of permutation 0
//   -> ONE wait, the copies back -> on the host: n_ge, p_perm, the beta approximation
#include "qtl_run.h"

#include <cfloat>
#include <cmath>

namespace {

rgx_qtl_perm_result *perm_alloc(uint64_t K, uint32_t S, uint32_t V, uint32_t n_cov, uint32_t B, bool pinned) {
    rgx_qtl_perm_result *q = result_alloc<rgx_qtl_perm_result>(pinned, [&](rgx_qtl_perm_result &r, BlockTake &take) {
        take(r.yy, K); take(r.gg, V); take(r.perm_r, K * ((size_t)B + 1)); take(r.best_r, K); take(r.best_slope, K); take(r.p_perm, K);
        take(r.beta_shape1, K); take(r.beta_shape2, K); take(r.p_beta, K); take(r.n_cis, K); take(r.best_variant, K); take(r.n_ge, K);
        take(r.variant_verdict, V); take(r.beta_status, K);
    });
    if (!q) return nullptr;
    q->n_rows = K; q->n_samples = S; q->n_variants = V; q->n_cov = n_cov; q->dof = S - n_cov - 2; q->n_perm = B;
    return q;
}

}  // namespace

// what the host can judge of the permutations, the same for the device and the twin; n_series of `series` (rows, groups) get B + 1 values each
int check_perm(uint64_t n_series, const char *series, uint32_t S, uint32_t B, const uint16_t *perm, char *err, size_t errlen) {
    if (!B || B > 65535u) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the permutation pass takes 1 to 65535 permutations; %u were asked for\n", B);
    if (!perm) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the permutation pass needs its permutations\n");
    if (n_series * ((uint64_t)B + 1) > kQtlMaxPairs) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: %llu %s x %u permutations and the identity; the permutation pass takes at most 2^32 - 2^16 of them\n",
        (unsigned long long)n_series, series, B);
    for (uint32_t s = 0; s < S; ++s) if (perm[s] != s) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: row 0 of the permutations is not the identity (sample %u stands at %u)\n", (uint32_t)perm[s], s);
    std::vector<uint8_t> seen(S);
    for (uint32_t b = 1; b <= B; ++b) {
        std::fill(seen.begin(), seen.end(), 0);
        const uint16_t *row = perm + (size_t)b * S;
        for (uint32_t s = 0; s < S; ++s) {
            if (row[s] >= S || seen[row[s]]) return fail(err, errlen, RGX_ERR_ARG,
                "regtools_amd: row %u of the permutations is no permutation of 0 .. %u (index %u at %u)\n", b, S - 1, (uint32_t)row[s], s);
            seen[row[s]] = 1;
        }
    }
    return RGX_OK;
}

size_t qtl_host_threads() { return std::min<size_t>(16, std::max<size_t>(1, std::thread::hardware_concurrency())); }

namespace {

long double digamma_l(long double x) {
    long double acc = 0.0L;
    for (; x < 32.0L; x += 1.0L) acc -= 1.0L / x;
    const long double i2 = 1.0L / (x * x);
    // sum B_2n / (2n x^2n), n = 1 .. 8
    const long double series = i2 * (1.0L / 12 - i2 * (1.0L / 120 - i2 * (1.0L / 252 - i2 * (1.0L / 240 - i2 * (1.0L / 132 - i2 * (691.0L / 32760 -
                               i2 * (1.0L / 12 - i2 * (3617.0L / 8160))))))));
    return acc + logl(x) - 0.5L / x - series;
}
long double trigamma_l(long double x) {
    long double acc = 0.0L;
    for (; x < 32.0L; x += 1.0L) acc += 1.0L / (x * x);
    const long double i2 = 1.0L / (x * x);
    // sum B_2n / x^(2n + 1), n = 1 .. 8
    const long double series = i2 * (1.0L / 6 - i2 * (1.0L / 30 - i2 * (1.0L / 42 - i2 * (1.0L / 30 - i2 * (5.0L / 66 - i2 * (691.0L / 2730 -
                               i2 * (7.0L / 6 - i2 * (3617.0L / 510))))))));
    return acc + 1.0L / x + 0.5L * i2 + series / x;
}
long double betainc_l(long double x, long double a, long double b) {
    if (x <= 0.0L) return 0.0L;
    if (x >= 1.0L) return 1.0L;
    const long double y = 1.0L - x;                                     // (exact: x is a double)
    const long double front = expl(a * logl(x) + b * log1pl(-x) - lgammal(a) - lgammal(b) + lgammal(a + b));
    long double p;
    if (x < (a + 1.0L) / (a + b + 2.0L)) p = front * qtl_beta_cf(a, b, x) / a;
    else p = 1.0L - front * qtl_beta_cf(b, a, y) / b;
    return p < 0.0L ? 0.0L : p > 1.0L ? 1.0L : p;
}

int beta_fit_l(const double *p, uint32_t n, long double &a, long double &b) {
    a = b = NAN;
    if (n < 2) return 2;
    long double sum = 0.0L, l1 = 0.0L, l2 = 0.0L;
    for (uint32_t i = 0; i < n; ++i) { sum += p[i]; l1 += logl((long double)p[i]); l2 += log1pl(-(long double)p[i]); }
    const long double m = sum / n;
    long double ss = 0.0L;
    for (uint32_t i = 0; i < n; ++i) { const long double d = (long double)p[i] - m; ss += d * d; }
    const long double v = ss / n;
    if (!(v > 0.0L)) return 2;
    const long double a0 = m * (m * (1.0L - m) / v - 1.0L), b0 = a0 * (1.0L / m - 1.0L);
    if (!(a0 > 0.0L) || !(b0 > 0.0L) || std::isinf(a0) || std::isinf(b0)) return 2;
    l1 /= n; l2 /= n;
    a = a0; b = b0;
    for (int step = 0; step < 100; ++step) {
        const long double pab = digamma_l(a + b), tab = trigamma_l(a + b);
        const long double g1 = digamma_l(a) - pab - l1, g2 = digamma_l(b) - pab - l2;
        const long double j11 = trigamma_l(a) - tab, j22 = trigamma_l(b) - tab, j12 = -tab;
        const long double det = j11 * j22 - j12 * j12;
        long double da = -(j22 * g1 - j12 * g2) / det, db = -(j11 * g2 - j12 * g1) / det;
        if (da != da || db != db || std::isinf(da) || std::isinf(db)) break;
        for (int h = 0; h < 200 && (!(a + da > 0.0L) || !(b + db > 0.0L)); ++h) { da *= 0.5L; db *= 0.5L; }
        if (!(a + da > 0.0L) || !(b + db > 0.0L)) break;
        const bool done = fabsl(da) < 1e-12L * a && fabsl(db) < 1e-12L * b;
        a += da; b += db;
        if (done) return 0;
    }
    a = a0; b = b0;
    return 1;
}

}  // namespace

// One series of B + 1 |r| values (a row's, a group's): n_ge and p_perm, then -- when the series has pairs -- the beta approximation of the p of
// b = 1 .. B and p_beta at best_r.  p: room for B doubles.  The sums are in ascending b, so the result does not depend on who runs it.
void qtl_series_finish(const double *row, uint32_t B, double best_r, uint32_t dof, bool has_pairs, double *p, uint32_t &n_ge_out, double &p_perm,
                       double &shape1, double &shape2, double &p_beta, uint8_t &status) {
    const uint64_t top = qtl_abs_bits(row[0]);
    uint32_t n_ge = 0;
    for (uint32_t b = 1; b <= B; ++b) n_ge += qtl_abs_bits(row[b]) >= top;
    n_ge_out = n_ge;
    p_perm = (double)(n_ge + 1) / (double)(B + 1);
    shape1 = shape2 = p_beta = NAN; status = 2;
    if (!has_pairs) return;
    for (uint32_t b = 1; b <= B; ++b) {
        const double pb = rgx_qtl_pvalue(rgx_qtl_tstat(row[b], dof), dof);
        p[b - 1] = pb < DBL_MIN ? DBL_MIN : pb > 1.0 - 0x1p-53 ? 1.0 - 0x1p-53 : pb;
    }
    long double a, b2;
    status = (uint8_t)beta_fit_l(p, B, a, b2);
    if (status == 2) return;
    shape1 = (double)a; shape2 = (double)b2;
    const double x = rgx_qtl_pvalue(rgx_qtl_tstat(best_r, dof), dof);
    p_beta = (double)betainc_l(x, shape1, shape2);
}

void qtl_series_products(const QtlHost &h, uint32_t S, uint32_t B, const uint16_t *perm, const uint32_t *rows, uint32_t n, double *series,
                         uint32_t *best_row, uint32_t &best_variant, double &best_r, double &best_slope) {
    std::vector<double> yp(S);
    std::vector<uint64_t> top((size_t)B + 1, 0);
    if (best_row) *best_row = RGX_NO_PAIR;
    best_variant = RGX_NO_PAIR; best_r = 0.0; best_slope = 0.0;
    // members in ascending row, variants in ascending order: a strictly larger |r| alone replaces, so the earliest of equals stays
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t k = rows[i];
        const double *y = h.Y.data() + (size_t)k * S;
        for (uint32_t b = 0; b <= B && h.cnt[k]; ++b) {
            const uint16_t *pb = perm + (size_t)b * S;
            for (uint32_t s = 0; s < S; ++s) yp[s] = y[pb[s]];
            for (uint32_t j = 0; j < h.cnt[k]; ++j) {
                const uint32_t v = h.u_var[h.lo[k] + j]; const double *x = h.G.data() + (size_t)v * S;
                double acc = 0.0;
                for (uint32_t s = 0; s < S; ++s) acc = qtl_fma(yp[s], x[s], acc);
                const double r = qtl_r(acc, h.yy[k], h.gg[v]);
                const uint64_t bits = qtl_abs_bits(r);
                if (!b && (best_variant == RGX_NO_PAIR || bits > top[0])) {
                    if (best_row) *best_row = k;
                    best_variant = v; best_r = r; best_slope = qtl_slope(acc, h.gg[v]);
                }
                if (bits > top[b]) top[b] = bits;
            }
        }
    }
    memcpy(series, top.data(), ((size_t)B + 1) * 8);
}

template <class R> int perm_finish(R *q, bool device, char *err, size_t errlen) {
    const Series sr = series_of(q);
    const uint64_t N = sr.n; const uint32_t B = q->n_perm, dof = q->dof;
    count_verdicts(q);
    const uint64_t p_tiles = ((uint64_t)B + 1 + kQtlTile - 1) / kQtlTile;
    for (uint64_t g = 0; g < N; ++g) {
        const uint32_t m_end = sr.begin ? sr.begin[g + 1] : (uint32_t)g + 1;
        uint64_t n = 0;
        for (uint32_t m = sr.begin ? sr.begin[g] : (uint32_t)g; m < m_end; ++m) {
            const uint32_t c = q->n_cis[sr.row ? sr.row[m] : m];
            n += c;
            if (device) q->n_tiles += p_tiles * (((uint64_t)c + kQtlTile - 1) / kQtlTile);
        }
        if (sr.pairs) { sr.pairs[g] = n; q->n_pairs += n; }
    }
    const double t0 = now_ms();
    try {
        WorkerPool pool(N * B < 4096 ? 1 : qtl_host_threads());
        const uint64_t chunk = 16, n_tasks = (N + chunk - 1) / chunk;
        pool.run((size_t)n_tasks, [&](size_t task) {
            std::vector<double> p(B);
            for (uint64_t g = task * chunk; g < N && g < (task + 1) * chunk; ++g)
                qtl_series_finish(q->perm_r + g * ((size_t)B + 1), B, q->best_r[g], dof, (sr.pairs ? sr.pairs[g] : q->n_cis[g]) != 0, p.data(),
                                  q->n_ge[g], q->p_perm[g], q->beta_shape1[g], q->beta_shape2[g], q->p_beta[g], q->beta_status[g]);
        });
    } catch (const std::exception &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory or threads for the beta approximation\n"); }
    q->ms_beta = now_ms() - t0;
    return RGX_OK;
}
template int perm_finish(rgx_qtl_perm_result *, bool, char *, size_t);
template int perm_finish(rgx_qtl_group_result *, bool, char *, size_t);

int PermRun::launch() {
    int rc = run.open();
    if (rc == RGX_OK) rc = run.residuals();
    if (rc == RGX_OK) rc = run.compact();
    if (rc == RGX_OK) rc = run.plan_launch();
    if (rc == RGX_OK) rc = products();
    return rc;
}

int PermRun::products() {
    rgx_cohort *co = run.co; char *err = run.err; const size_t errlen = run.errlen; hipStream_t st = run.st;
    const uint32_t S = run.S, N = n_series;
    if ((uint64_t)N * (ldp / kQtlTile) > 0x7fffffffull) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: %u %s x %zu blocks of 64 permutations are more than 2^31 - 1 workgroups\n", N, series, ldp / kQtlTile);
    try { permT.assign((size_t)S * ldp, 0); }
    catch (const std::bad_alloc &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for %u permutations of %u samples\n", B, S); }
    for (uint32_t b = 0; b <= B; ++b) for (uint32_t s = 0; s < S; ++s) permT[(size_t)s * ldp + b] = perm[(size_t)b * S + s];
    const size_t n_out = (size_t)N * ((size_t)B + 1), n_begin = mem ? (size_t)N + 1 : 0, n_mem = mem ? mem->row.size() : 0;
    if (co->qp_in.ensure(permT.size() * 2 + (n_begin + n_mem) * 4 + 256) != hipSuccess ||
        co->qp_out.ensure(n_out * 8 + (size_t)N * (mem ? 28 : 24) + 256) != hipSuccess) {
        (void)hipGetLastError();
        return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no device memory for %u permutations of %u %s\n", B, N, series); }
    Carve in(co->qp_in);
    d_permT = in.take<uint16_t>(permT.size());
    if (mem) { d_begin = in.u32(n_begin); d_row = in.u32(n_mem); }
    CARVE_TRY(in, mem ? "grouped sQTL permutation" : "sQTL permutation");
    Carve o(co->qp_out);
    perm_r = o.take<double>(n_out); best_r = o.take<double>(N); best_slope = o.take<double>(N); best_u = o.u32(N); best_variant = o.u32(N);
    if (mem) best_row = o.u32(N);
    CARVE_TRY(o, mem ? "grouped sQTL permutation result" : "sQTL permutation result");
    HIP_TRY(hipMemcpyAsync(d_permT, permT.data(), permT.size() * 2, hipMemcpyHostToDevice, st));
    if (mem) { HIP_TRY(hipMemcpyAsync(d_begin, mem->begin.data(), n_begin * 4, hipMemcpyHostToDevice, st)); }
    if (n_mem) { HIP_TRY(hipMemcpyAsync(d_row, mem->row.data(), n_mem * 4, hipMemcpyHostToDevice, st)); }
    run.mark(mem ? "members + permutations in HBM" : "permutations in HBM");
    HIP_TRY(hipEventRecord(run.ev[2], st));
    // (without lists all three of d_begin, d_row and best_row are null: series g is table row g alone)
    launch_qtl_perm(run.Y, N, S, d_permT, ldp, B + 1, run.Gt, run.ldg, run.lo, run.count, run.yy, run.u_gg, d_begin, d_row, perm_r, best_row, best_u,
                    st);
    run.mark(mem ? "grouped permuted products" : "permuted products");
    launch_qtl_perm_best(run.Y, run.G, N, S, best_row, best_u, run.u_var, run.yy, run.gg, best_variant, best_r, best_slope, st);
    HIP_TRY(hipEventRecord(run.ev[3], st));
    run.mark("best pairs");
    return RGX_OK;
}

int PermRun::no_result() {
    return fail(run.err, run.errlen, RGX_ERR_DEVICE, "regtools_amd: no memory for the result of %u %s and %u permutations\n", n_series, series, B);
}

template <class R> int PermRun::finish(R *q) {
    char *err = run.err; const size_t errlen = run.errlen; hipStream_t st = run.st;
    const uint32_t K = run.K, V = run.V; const size_t N = n_series;
    uint64_t h[4] = {0, 0, 0, 0};
    CopyBack back{st};
    back(q->yy, run.yy, (size_t)K * 8); back(q->gg, run.gg, (size_t)V * 8); back(q->variant_verdict, run.verdict, V);
    back(q->n_cis, run.count, (size_t)K * 4); back(q->perm_r, perm_r, N * ((size_t)B + 1) * 8); back(q->best_r, best_r, N * 8);
    back(q->best_slope, best_slope, N * 8);
    if (mem) back(series_of(q).best_row, best_row, N * 4);
    back(q->best_variant, best_variant, N * 4); back(h, run.head, 32);
    hipError_t e_ = back.wait();
    float ms_res = 0, ms_pr = 0;
    if (e_ == hipSuccess) e_ = hipEventElapsedTime(&ms_res, run.ev[0], run.ev[1]);
    if (e_ == hipSuccess) e_ = hipEventElapsedTime(&ms_pr, run.ev[2], run.ev[3]);
    if (e_ != hipSuccess) return fail(err, errlen, RGX_ERR_DEVICE, "HIP error %s in the %ssQTL permutation pass\n", hipGetErrorString(e_),
                                      mem ? "grouped " : "");
    run.mark("copies");
    int rc = bad_flags((const uint32_t *)(h + 2), K, err, errlen);
    if (rc != RGX_OK) return rc;
    if (!mem) q->n_pairs = h[0];                                      // (the grouped result's is the sum over its groups: perm_finish)
    rc = perm_finish(q, /*device=*/true, err, errlen);
    if (rc != RGX_OK) return rc;
    q->ms_residual = ms_res; q->ms_products = ms_pr; q->ms_perm = now_ms() - run.t0;
    return RGX_OK;
}
template int PermRun::finish(rgx_qtl_perm_result *);
template int PermRun::finish(rgx_qtl_group_result *);

extern "C" void rgx_cohort_qtl_perm_free(rgx_qtl_perm_result *q) { result_free(q); }

extern "C" int rgx_qtl_permutations(uint32_t n_samples, uint32_t n_perm, uint64_t seed, uint16_t *out, char *err, size_t errlen) {
    const uint32_t S = n_samples;
    if (!S || S > 65536u || n_perm > 65535u || !out) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: rgx_qtl_permutations takes 1 to 65536 samples, at most 65535 permutations and room for them\n");
    uint64_t z = seed;
    auto next = [&]() {
        z += 0x9E3779B97F4A7C15ull;
        uint64_t x = z;
        x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ x >> 27) * 0x94D049BB133111EBull;
        return x ^ x >> 31;
    };
    for (uint32_t b = 0; b <= n_perm; ++b) {
        uint16_t *p = out + (size_t)b * S;
        for (uint32_t s = 0; s < S; ++s) p[s] = (uint16_t)s;
        if (!b) continue;
        for (uint32_t i = S - 1; i >= 1; --i) {
            const uint32_t j = (uint32_t)(((unsigned __int128)next() * (i + 1)) >> 64);
            std::swap(p[i], p[j]);
        }
    }
    return RGX_OK;
}

extern "C" double rgx_qtl_digamma(double x) { return x > 0.0 ? (double)digamma_l(x) : NAN; }
extern "C" double rgx_qtl_trigamma(double x) { return x > 0.0 ? (double)trigamma_l(x) : NAN; }
extern "C" double rgx_qtl_betainc(double x, double a, double b) {
    if (!(a > 0.0) || !(b > 0.0) || !(x >= 0.0) || !(x <= 1.0) || std::isinf(a) || std::isinf(b)) return NAN;
    return (double)betainc_l(x, a, b);
}
extern "C" int rgx_qtl_beta_fit(const double *p, uint32_t n, double *shape1, double *shape2) {
    long double a = NAN, b = NAN;
    int status = 2;
    if (p) {
        bool inside = true;
        for (uint32_t i = 0; i < n; ++i) inside = inside && p[i] > 0.0 && p[i] < 1.0;
        if (inside) status = beta_fit_l(p, n, a, b);
    }
    if (shape1) *shape1 = (double)a;
    if (shape2) *shape2 = (double)b;
    return status;
}

extern "C" int rgx_cohort_qtl_permute(rgx_cohort *co, const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants,
                                      const uint32_t *var_tid, const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates,
                                      uint32_t window, uint32_t n_perm, const uint16_t *perm, rgx_qtl_perm_result **out, char *err, size_t errlen) {
    if (!co || !ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_qtl_permute needs a cohort and a phenotype table\n");
    *out = nullptr;
    std::lock_guard<std::mutex> lock(co->mu);
    const QtlArgs a{ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, window};
    int rc = check_qtl(a, err, errlen);
    if (rc == RGX_OK) rc = check_perm(ph->n_rows, "rows", ph->n_samples, n_perm, perm, err, errlen);
    if (rc != RGX_OK) return rc;
    PermRun p(co, a, n_perm, perm, (uint32_t)ph->n_rows, "rows", nullptr, err, errlen);
    rc = p.launch();
    rgx_qtl_perm_result *q = nullptr;
    if (rc == RGX_OK && !(q = perm_alloc(ph->n_rows, ph->n_samples, n_variants, n_cov, n_perm, /*pinned=*/true))) rc = p.no_result();
    if (rc == RGX_OK) rc = p.finish(q);
    if (rc != RGX_OK) {
        if (p.run.st) (void)hipStreamSynchronize(p.run.st);            // (the copies read the caller's arrays and this run's T, Q and permT, and write q)
        rgx_cohort_qtl_perm_free(q);
        return rc;
    }
    *out = q;
    return RGX_OK;
}

extern "C" int rgx_cohort_qtl_permute_host(const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants, const uint32_t *var_tid,
                                           const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates, uint32_t window,
                                           uint32_t n_perm, const uint16_t *perm, rgx_qtl_perm_result **out, char *err, size_t errlen) {
    if (!ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_qtl_permute_host needs a phenotype table\n");
    *out = nullptr;
    const double t0 = now_ms();
    const QtlArgs a{ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, window};
    int rc = check_qtl(a, err, errlen);
    if (rc == RGX_OK) rc = check_perm(ph->n_rows, "rows", ph->n_samples, n_perm, perm, err, errlen);
    if (rc != RGX_OK) return rc;
    QtlHost h;
    rc = qtl_host_prepare(a, h, err, errlen);
    if (rc != RGX_OK) return rc;
    const uint64_t K = ph->n_rows; const uint32_t S = ph->n_samples, V = n_variants, B = n_perm;
    rgx_qtl_perm_result *q = perm_alloc(K, S, V, n_cov, B, false);
    if (!q) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the result of %llu rows and %u permutations\n", (unsigned long long)K, B);
    memcpy(q->yy, h.yy.data(), K * 8);
    memcpy(q->n_cis, h.cnt.data(), K * 4);
    if (V) { memcpy(q->gg, h.gg.data(), (size_t)V * 8); memcpy(q->variant_verdict, h.verdict.data(), V); }
    q->n_pairs = h.P;
    try {
        WorkerPool pool(h.P * ((uint64_t)B + 1) * S < (1u << 20) ? 1 : qtl_host_threads());
        pool.run((size_t)K, [&](size_t k) {
            const uint32_t row = (uint32_t)k;
            qtl_series_products(h, S, B, perm, &row, 1, q->perm_r + k * ((size_t)B + 1), nullptr, q->best_variant[k], q->best_r[k], q->best_slope[k]);
        });
    } catch (const std::exception &) { rgx_cohort_qtl_perm_free(q); return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory or threads for the permutation pass\n"); }
    const double t1 = now_ms();
    rc = perm_finish(q, /*device=*/false, err, errlen);
    if (rc != RGX_OK) { rgx_cohort_qtl_perm_free(q); return rc; }
    q->ms_residual = h.t_pairs - h.t_res; q->ms_products = t1 - h.t_pairs; q->ms_perm = now_ms() - t0;
    *out = q;
    return RGX_OK;
}

// ---- text ---------------------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t rgx_cohort_format_qtl_perm(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_table *ph,
                                             const rgx_qtl_perm_result *q, const uint32_t *var_pos, const char *const *variant_id, char *buf, size_t cap) {
    if (!qtl_text_args_ok(m, cl, ph, q, var_pos, variant_id)) return 0;
    return format_twice(buf, cap, [&](TextOut &o) {
        o.put("phenotype_id\tnum_var\tbeta_shape1\tbeta_shape2\tdof\tvariant_id\tdistance\tr\tslope\tslope_se\ttstat\tpval_nominal\t"
              "pval_perm\tpval_beta\n");
        for (uint64_t k = 0; q && k < q->n_rows; ++k) {
            if (!q->n_cis[k]) continue;
            const uint32_t i = ph->row[k], v = q->best_variant[k];
            const double t = rgx_qtl_tstat(q->best_r[k], q->dof);
            put_intron_id(o, m, cl, i);
            o.fmt("\t%u\t", q->n_cis[k]);
            o.g17(q->beta_shape1[k], '\t'); o.g17(q->beta_shape2[k], '\t');
            o.fmt("%u\t", q->dof);
            o.put(variant_id[v]);
            o.fmt("\t%lld\t", (long long)var_pos[v] - (long long)m->start[i]);
            o.g17(q->best_r[k], '\t'); o.g17(q->best_slope[k], '\t'); o.g17(q->best_slope[k] / t, '\t'); o.g17(t, '\t');
            o.g17(rgx_qtl_pvalue(t, q->dof), '\t'); o.g17(q->p_perm[k], '\t'); o.g17(q->p_beta[k], '\n');
        }
    });
}
