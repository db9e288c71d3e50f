// cohort_pcs.cpp -- the principal components of the cohort's phenotype table: rgx_cohort_pheno_pcs (device), its host twin
// rgx_cohort_pheno_pcs_host and the text (contract in include/regtools_amd.h; modelled on the .PCs file of LeafCutter's
// prepare_phenotype_table.py, which the reference does not contain).  Device side: pca_kernels.hip; arithmetic: pca_core.h.
//   rank2 + the quantile table T in HBM -> per (tile pair, chunk of rows) the partial Gram tile and column sums -> the chunks added in order
//   -> ONE copy back -> on the host, for the device path and the twin alike: covariance, cyclic Jacobi, order, signs
#include "cohort_internal.h"
#include "pca_core.h"

#include <cmath>
#include <numeric>

namespace {

// gram, col_sum and the flag's slot are ONE array of S * S + S + 1 doubles with no padding between them: the device writes that piece (PcsRun::open
// carves pc_out in the same order) and finish copies it back in one call, and S * S * 8 is no multiple of 16 for odd S.  So the three are derived
// from the one array, not taken apart; the host part's results lie behind it.
rgx_pheno_pcs *pcs_alloc(uint64_t K, uint32_t S, uint32_t n_pcs, bool pinned) {
    rgx_pheno_pcs *p = result_alloc<rgx_pheno_pcs>(pinned, [&](rgx_pheno_pcs &r, BlockTake &take) {
        take(r.gram, (size_t)S * S + S + 1); take(r.variance, S); take(r.component, (size_t)n_pcs * S);
    });
    if (!p) return nullptr;
    p->n_rows = K; p->n_samples = S; p->n_pcs = n_pcs;
    p->col_sum = p->gram + (size_t)S * S;
    return p;
}
uint32_t *pcs_flag(rgx_pheno_pcs *p) { return (uint32_t *)(p->col_sum + p->n_samples); }

// the arguments the host can judge, the same for the device and the twin
int check_pcs(const rgx_pheno_table *ph, uint32_t n_pcs, char *err, size_t errlen) {
    const uint64_t K = ph->n_rows; const uint32_t S = ph->n_samples;
    if (K < 2 || K > 0x7fffffffull) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: principal components need a table of 2 to 2^31 - 1 rows; this one has %llu\n",
        (unsigned long long)K);
    if (!S || S > kPcaMaxSamples) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: principal components take 1 to %u samples; the table has %u\n",
        kPcaMaxSamples, S);
    if (!n_pcs || n_pcs > std::min<uint64_t>(K, S)) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: %u components asked of a table of %llu rows and %u samples\n", n_pcs, (unsigned long long)K, S);
    if (!ph->rank2) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the phenotype table has no ranks\n");
    return RGX_OK;
}
int bad_rank(uint64_t K, char *err, size_t errlen) {
    return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the phenotype table holds a rank2 outside 2 .. %llu\n", (unsigned long long)(2 * K));
}

// T[r - 2] = rgx_pheno_quantile(r, K) for r = 2 .. 2 K.  The function is odd around the middle rank K + 1 to the last bit (cohort_pheno.cpp), so
// the upper half is the lower one's negation -- the same doubles as 2 K - 1 calls, for K of them.
void quantile_table(uint64_t K, std::vector<double> &T) {
    T.resize(2 * K - 1);
    for (uint64_t r = 2; r <= K + 1; ++r) T[r - 2] = rgx_pheno_quantile((uint32_t)r, K);
    for (uint64_t r = K + 2; r <= 2 * K; ++r) T[r - 2] = -T[2 * K - r];         // (the mirror of r is 2 K + 2 - r)
}

// ---- the host part, shared by the device path and the twin ------------------------------------------------------------------------------------
// Cyclic Jacobi in Rutishauser's form (Handbook for Automatic Computation II, contribution II/1) on the full symmetric n x n matrix a, which it
// destroys: d = the diagonal it ends with, row i of vt = the unit eigenvector of d[i].  A rotation updates rows p and q, which lie contiguous, and
// mirrors them into the columns.  false: no convergence in 100 sweeps (not seen).
bool jacobi_eigen(double *a, uint32_t n, double *vt, double *d) {
    RGX_FP_EXACT
    for (size_t i = 0; i < (size_t)n * n; ++i) vt[i] = 0.0;
    for (uint32_t i = 0; i < n; ++i) vt[(size_t)i * n + i] = 1.0;
    bool done = false;
    for (uint32_t sweep = 0; sweep < 100 && !done; ++sweep) {
        double off = 0.0;
        for (uint32_t p = 0; p < n; ++p) for (uint32_t q = p + 1; q < n; ++q) off += fabs(a[(size_t)p * n + q]);
        if (off == 0.0) { done = true; break; }
        const double thresh = sweep < 3 ? 0.2 * off / ((double)n * (double)n) : 0.0;
        for (uint32_t p = 0; p + 1 < n; ++p) {
            double *rp = a + (size_t)p * n, *vp = vt + (size_t)p * n;
            for (uint32_t q = p + 1; q < n; ++q) {
                double *rq = a + (size_t)q * n, *vq = vt + (size_t)q * n;
                const double apq = rp[q], g = 100.0 * fabs(apq), dp = rp[p], dq = rq[q];
                if (sweep > 3 && fabs(dp) + g == fabs(dp) && fabs(dq) + g == fabs(dq)) { rp[q] = 0.0; rq[p] = 0.0; continue; }
                if (!(fabs(apq) > thresh)) continue;
                const double h = dq - dp;
                double t;
                if (fabs(h) + g == fabs(h)) t = apq / h;
                else {
                    const double theta = 0.5 * h / apq;
                    t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
                    if (theta < 0.0) t = -t;
                }
                const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
                for (uint32_t k = 0; k < n; ++k) {
                    const double x = rp[k], y = rq[k];
                    rp[k] = x - s * (y + x * tau); rq[k] = y + s * (x - y * tau);
                }
                rp[p] = dp - t * apq; rq[q] = dq + t * apq; rp[q] = 0.0; rq[p] = 0.0;
                for (uint32_t k = 0; k < n; ++k) { a[(size_t)k * n + p] = rp[k]; a[(size_t)k * n + q] = rq[k]; }
                for (uint32_t k = 0; k < n; ++k) {
                    const double x = vp[k], y = vq[k];
                    vp[k] = x - s * (y + x * tau); vq[k] = y + s * (x - y * tau);
                }
            }
        }
    }
    for (uint32_t i = 0; i < n; ++i) d[i] = a[(size_t)i * n + i];
    return done;
}

// gram and col_sum -> variance (all S eigenvalues of the covariance, descending) and the first n_pcs components, signed
int pcs_host_part(rgx_pheno_pcs *p, char *err, size_t errlen) {
    RGX_FP_EXACT
    const uint32_t S = p->n_samples;
    const uint64_t K = p->n_rows;
    std::vector<double> cov, vt, d;
    try { cov.resize((size_t)S * S); vt.resize((size_t)S * S); d.resize(S); }
    catch (const std::bad_alloc &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the covariance of %u samples\n", S); }
    for (uint32_t s = 0; s < S; ++s) for (uint32_t t = s; t < S; ++t)
        cov[(size_t)s * S + t] = cov[(size_t)t * S + s] = pca_cov(p->gram[(size_t)s * S + t], p->col_sum[s], p->col_sum[t], K);
    if (!jacobi_eigen(cov.data(), S, vt.data(), d.data())) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: the eigenvalues of the covariance of %u samples did not settle in 100 sweeps\n", S);
    std::vector<uint32_t> order(S);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return d[a] > d[b]; });
    for (uint32_t i = 0; i < S; ++i) p->variance[i] = d[order[i]];
    for (uint32_t i = 0; i < p->n_pcs; ++i) {
        const double *v = vt.data() + (size_t)order[i] * S;
        double norm2 = 0.0; uint32_t big = 0;
        for (uint32_t s = 0; s < S; ++s) { norm2 += v[s] * v[s]; if (fabs(v[s]) > fabs(v[big])) big = s; }
        const double scale = (v[big] < 0.0 ? -1.0 : 1.0) / sqrt(norm2);                      // (unit length; the largest entry, the first of equals, positive)
        double *out = p->component + (size_t)i * S;
        for (uint32_t s = 0; s < S; ++s) out[s] = v[s] * scale;
    }
    return RGX_OK;
}

// One device run, as the stages rgx_cohort_pheno_pcs is made of.  The caller holds the cohort's lock and has checked the arguments; every stage
// enqueues on the cohort's stream and returns RGX_OK or the failed call's code.
struct PcsRun : CohortRun {
    const rgx_pheno_table *ph; uint32_t n_pcs; double t_gram = 0;
    uint64_t K; uint32_t S, n_tiles, n_chunks;
    std::vector<double> T;
    const uint32_t *rank2 = nullptr; const double *d_T = nullptr;
    double *part = nullptr, *col_part = nullptr, *gram = nullptr, *col_sum = nullptr; uint32_t *bad = nullptr;

    PcsRun(rgx_cohort *co_, const rgx_pheno_table *ph_, uint32_t n_pcs_, char *err_, size_t errlen_)
        : CohortRun(co_, "pheno pcs", err_, errlen_), ph(ph_), n_pcs(n_pcs_), K(ph_->n_rows), S(ph_->n_samples),
          n_tiles((ph_->n_samples + kPcaTile - 1) / kPcaTile), n_chunks(pca_n_chunks(ph_->n_rows)) {}

    // 1. the quantile table (host), then rank2 and the table in HBM and the workspaces
    int open() {
        if (int rc = enter()) return rc;
        try { quantile_table(K, T); }
        catch (const std::bad_alloc &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the %llu quantiles\n", (unsigned long long)(2 * K - 1)); }
        mark("quantile table");
        t_gram = now_ms();
        const size_t n_entries = (size_t)K * S, n_T = (size_t)(2 * K - 1);
        if (int rc = grow(co->pc_in, n_T * 8 + n_entries * 4 + 256, "regtools_amd: no device memory for a table of %llu rows and %u samples\n",
                  (unsigned long long)K, S)) return rc;
        Carve u = carve(co->pc_in);                          // (both arrays written whole by their uploads)
        double *t_up = u.take<double>(n_T); uint32_t *r_up = u.u32(n_entries);
        CARVE_TRY(u, "principal component input");
        if (int rc = carved(u, "principal component input")) return rc;
        HIP_TRY(hipMemcpyAsync(r_up, ph->rank2, n_entries * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t_up, T.data(), n_T * 8, hipMemcpyHostToDevice, st));
        rank2 = r_up; d_T = t_up;
        const size_t n_pairs = (size_t)n_tiles * (n_tiles + 1) / 2, tile = (size_t)kPcaTile * kPcaTile, S_pad = (size_t)n_tiles * kPcaTile;
        if (int rc = grow(co->pc_part, (n_pairs * n_chunks * tile + (size_t)n_chunks * S_pad) * 8 + 256,
                  "regtools_amd: no device memory for the %u chunk partials of %u samples\n", n_chunks, S)) return rc;
        // first writers: part and col_part k_pca_gram, every (tile pair, chunk) partial and every chunk's S_pad column sums; k_pca_reduce reads
        // them all
        Carve w = carve(co->pc_part);
        part = w.take<double>(n_pairs * n_chunks * tile); col_part = w.take<double>((size_t)n_chunks * S_pad);
        CARVE_TRY(w, "principal component partials");
        if (int rc = carved(w, "principal component partials")) return rc;
        if (int rc = grow(co->pc_out, ((size_t)S * S + S + 1) * 8 + 256, "regtools_amd: no device memory for the Gram matrix of %u samples\n", S)) return rc;
        // first writers: gram (both triangles) and col_sum k_pca_reduce (whole); the flag word the memset below, then k_pca_gram
        Carve o = carve(co->pc_out);                         // (in the order of the result's block: one copy takes the three)
        gram = o.take<double>((size_t)S * S); col_sum = o.take<double>(S); bad = (uint32_t *)o.take<double>(1);
        CARVE_TRY(o, "principal component output");
        if (int rc = carved(o, "principal component output")) return rc;
        HIP_TRY(hipMemsetAsync(bad, 0, 8, st));
        mark("rank2 + quantiles in HBM");
        return RGX_OK;
    }
    // 2. one partial per (tile pair, chunk)
    int gram_partials() { launch_pca_gram(rank2, d_T, K, S, part, col_part, bad, st); mark("gram partials"); return RGX_OK; }
    // 3. the chunks in order: both triangles and the column sums
    int reduce() { launch_pca_reduce(part, col_part, K, S, gram, col_sum, st); mark("chunk reduction"); return RGX_OK; }
    // 4. one copy back, one wait, the host part
    int finish(rgx_pheno_pcs **out) {
        rgx_pheno_pcs *p = pcs_alloc(K, S, n_pcs, /*pinned=*/true);
        if (!p) { (void)hipStreamSynchronize(st); return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no memory for the principal components\n"); }
        CopyBack back{st};
        guards_back(back);
        back(p->gram, gram, ((size_t)S * S + S + 1) * 8);                // (gram, col_sum and the flag: pcs_alloc)
        const hipError_t e_ = back.wait();
        if (e_ != hipSuccess) { rgx_cohort_pheno_pcs_free(p); return fail(err, errlen, RGX_ERR_DEVICE, "HIP error %s building the Gram matrix\n",
            hipGetErrorString(e_)); }
        mark("copy");
        if (int rc = guards_check()) { rgx_cohort_pheno_pcs_free(p); return rc; }
        if (*pcs_flag(p)) { rgx_cohort_pheno_pcs_free(p); return bad_rank(K, err, errlen); }
        const double t1 = now_ms();
        p->ms_gram = t1 - t_gram;
        const int rc = pcs_host_part(p, err, errlen);
        if (rc != RGX_OK) { rgx_cohort_pheno_pcs_free(p); return rc; }
        const double t2 = now_ms();
        p->ms_eigen = t2 - t1; p->ms_pcs = t2 - t0;
        *out = p;
        return RGX_OK;
    }
};

// ---- the twin's Gram matrix ---------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kTwinRows = 32;           // rows whose quantiles are looked up together: an output row stays in cache for all of them

// rows [k0, k1) of one chunk into acc (S x S, upper triangle) and col; false: a rank2 that is no rank.  Every element takes its rows in ascending
// order, whatever the blocking.
static inline __attribute__((always_inline)) bool twin_rows(const uint32_t *rank2, const double *T, uint64_t K, uint32_t S, uint64_t k0, uint64_t k1,
                                                            double *q, double *acc, double *col) {
    for (uint64_t b0 = k0; b0 < k1; b0 += kTwinRows) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(kTwinRows, k1 - b0);
        for (uint32_t i = 0; i < nb; ++i) for (uint32_t s = 0; s < S; ++s) {
            const uint32_t r = rank2[(b0 + i) * S + s];
            if (!pca_rank_ok(r, K)) return false;
            q[(size_t)i * S + s] = T[r - 2];
        }
        for (uint32_t s = 0; s < S; ++s) {
            double *row = acc + (size_t)s * S, c = col[s];
            for (uint32_t i = 0; i < nb; ++i) {
                const double *qi = q + (size_t)i * S; const double a = qi[s];
                c = pca_add(c, a);
                for (uint32_t t = s; t < S; ++t) row[t] = pca_fma(a, qi[t], row[t]);
            }
            col[s] = c;
        }
    }
    return true;
}
// the same loop with the processor's own fused multiply-add where it has one (the result is that of std::fma: one rounding)
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("avx2,fma"))) bool twin_rows_fma(const uint32_t *rank2, const double *T, uint64_t K, uint32_t S, uint64_t k0, uint64_t k1, double *q,
                                                       double *acc, double *col) { return twin_rows(rank2, T, K, S, k0, k1, q, acc, col); }
bool have_fma() { return __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma"); }
#else
bool twin_rows_fma(const uint32_t *rank2, const double *T, uint64_t K, uint32_t S, uint64_t k0, uint64_t k1, double *q, double *acc, double *col) {
    return twin_rows(rank2, T, K, S, k0, k1, q, acc, col); }
bool have_fma() { return false; }
#endif
bool twin_rows_plain(const uint32_t *rank2, const double *T, uint64_t K, uint32_t S, uint64_t k0, uint64_t k1, double *q, double *acc, double *col) {
    return twin_rows(rank2, T, K, S, k0, k1, q, acc, col); }

}  // namespace

void pheno_quantile_table(uint64_t K, std::vector<double> &T) { quantile_table(K, T); }

extern "C" void rgx_cohort_pheno_pcs_free(rgx_pheno_pcs *pcs) { result_free(pcs); }

extern "C" int rgx_cohort_pheno_pcs(rgx_cohort *co, const rgx_pheno_table *ph, uint32_t n_pcs, rgx_pheno_pcs **out, char *err, size_t errlen) {
    if (!co || !ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_pheno_pcs needs a cohort and a phenotype table\n");
    *out = nullptr;
    std::lock_guard<std::mutex> lock(co->mu);
    int rc = check_pcs(ph, n_pcs, err, errlen);
    if (rc != RGX_OK) return rc;
    PcsRun run(co, ph, n_pcs, err, errlen);
    rc = run.open();
    if (rc == RGX_OK) rc = run.gram_partials();
    if (rc == RGX_OK) rc = run.reduce();
    if (rc == RGX_OK) rc = run.finish(out);
    else if (run.st) (void)hipStreamSynchronize(run.st);              // (the uploads read the caller's table and this run's T)
    return rc;
}

extern "C" int rgx_cohort_pheno_pcs_host(const rgx_pheno_table *ph, uint32_t n_pcs, rgx_pheno_pcs **out, char *err, size_t errlen) {
    if (!ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_pheno_pcs_host needs a phenotype table\n");
    *out = nullptr;
    const double t0 = now_ms();
    int rc = check_pcs(ph, n_pcs, err, errlen);
    if (rc != RGX_OK) return rc;
    const uint64_t K = ph->n_rows; const uint32_t S = ph->n_samples, n_chunks = pca_n_chunks(K);
    const uint64_t L = pca_chunk_rows(K, n_chunks);
    std::vector<double> T, q, acc, col;
    try { quantile_table(K, T); q.resize((size_t)kTwinRows * S); acc.resize((size_t)S * S); col.resize(S); }
    catch (const std::bad_alloc &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the Gram matrix of %u samples\n", S); }
    rgx_pheno_pcs *p = pcs_alloc(K, S, n_pcs, false);
    if (!p) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the principal components\n");
    const double t_gram = now_ms();
    for (size_t i = 0; i < (size_t)S * S; ++i) p->gram[i] = 0.0;
    for (uint32_t s = 0; s < S; ++s) p->col_sum[s] = 0.0;
    const auto rows = have_fma() ? twin_rows_fma : twin_rows_plain;
    for (uint32_t j = 0; j < n_chunks; ++j) {
        std::fill(acc.begin(), acc.end(), 0.0); std::fill(col.begin(), col.end(), 0.0);
        if (!rows(ph->rank2, T.data(), K, S, (uint64_t)j * L, std::min<uint64_t>(K, (uint64_t)(j + 1) * L), q.data(), acc.data(), col.data())) {
            rgx_cohort_pheno_pcs_free(p); return bad_rank(K, err, errlen); }
        for (uint32_t s = 0; s < S; ++s) {
            p->col_sum[s] = pca_add(p->col_sum[s], col[s]);
            for (uint32_t t = s; t < S; ++t) p->gram[(size_t)s * S + t] = pca_add(p->gram[(size_t)s * S + t], acc[(size_t)s * S + t]);
        }
    }
    for (uint32_t s = 0; s < S; ++s) for (uint32_t t = s + 1; t < S; ++t) p->gram[(size_t)t * S + s] = p->gram[(size_t)s * S + t];
    const double t1 = now_ms();
    p->ms_gram = t1 - t_gram;
    rc = pcs_host_part(p, err, errlen);
    if (rc != RGX_OK) { rgx_cohort_pheno_pcs_free(p); return rc; }
    const double t2 = now_ms();
    p->ms_eigen = t2 - t1; p->ms_pcs = t2 - t0;
    *out = p;
    return RGX_OK;
}

// ---- text: LeafCutter's .PCs layout ---------------------------------------------------------------------------------------------------------------
extern "C" size_t rgx_cohort_format_pheno_pcs(const rgx_cohort_matrix *m, const rgx_pheno_pcs *pcs, char *buf, size_t cap) {
    if (!m || (pcs && pcs->n_samples != m->n_samples)) return 0;
    return format_twice(buf, cap, [&](TextOut &o) {
        o.put("id");
        for (uint32_t g = 0; g < m->n_samples; ++g) { o.put("\t", 1); o.put(m->sample_name[g]); }
        o.put("\n", 1);
        for (uint32_t i = 0; pcs && i < pcs->n_pcs; ++i) {
            o.u(i + 1);
            for (uint32_t g = 0; g < m->n_samples; ++g) o.fmt("\t%.17g", pcs->component[(size_t)i * m->n_samples + g]);
            o.put("\n", 1);
        }
    });
}
