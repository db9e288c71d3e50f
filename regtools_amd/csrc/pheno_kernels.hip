// pheno_kernels.hip -- device half of the cohort's splicing phenotype table (rgx_cohort_phenotypes, cohort_pheno.cpp; contract in
// include/regtools_amd.h; per-entry arithmetic in pheno_core.h, which the host twin runs too).  The reference has no counterpart.
// A row's sums run in the contract's fixed order: sample s goes to partial s % 64 -- lane s % 64 of the row's wave, ascending s -- and the
// partials are halved with __shfl_down from 32 down to 1.  With at most 8 samples a row takes 8 lanes: partials 8 .. 63 are +0.0, adding them is
// exact, and the halving from 4 down gives the same bits.  No atomics, no LDS: every word has one writer, and the dense table behind the row
// filters is ordered by ONE stable radix sort of its entries (cohort_pheno.cpp), whose tie runs give the ranks.
// 256 threads per workgroup, wave64, bounded by HBM and by the binary searches into a row's CSR ranges (which stay in L2).
#include "kernels.h"
#include "pheno_core.h"

namespace rgx {

namespace {

template <uint32_t LANES> __device__ __forceinline__ double pheno_halve(double p) {
#pragma unroll
    for (uint32_t off = LANES / 2; off; off >>= 1) p = pheno_add(p, __shfl_down(p, off, LANES));
    return __shfl(p, 0, LANES);                              // (lane 0 of the group holds P[0]: every lane of the row gets it)
}

__device__ __forceinline__ PhenoRow pheno_row(const PhenoIn &in, uint32_t row, uint32_t c) {
    PhenoRow r;
    r.col_sample = in.col_sample; r.val_count = in.val_count; r.cs_sample = in.cs_sample; r.cs_total = in.cs_total;
    r.e0 = in.row_begin[row]; r.e1 = in.row_begin[row + 1]; r.d0 = in.cs_begin[c]; r.d1 = in.cs_begin[c + 1];
    return r;
}

}  // namespace

// One matrix row per group of LANES lanes (64, or 8 when there are at most 8 samples): missing samples, mean and sd in the contract's order, and
// the row filters.  Two passes over the row's samples: the sum, then the squared deviations from its mean.  A row without a cluster is neither
// kept nor counted.  Lane 0 of the group is the only writer of the row's words.
template <uint32_t LANES>
__global__ __launch_bounds__(256) void k_pheno_row_stats(PhenoIn in, uint32_t n, uint32_t n_samples, uint32_t na_num, uint32_t na_den, double min_sd,
                                                         uint32_t *__restrict__ n_na, double *__restrict__ mean, double *__restrict__ sd,
                                                         uint32_t *__restrict__ keep, uint32_t *__restrict__ drop_na) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t l = threadIdx.x % LANES;
    if (t / LANES >= n) return;                             // (LANES divides the wave: a row's lanes leave together)
    const uint32_t row = (uint32_t)(t / LANES);
    const uint32_t c = in.cluster[row];
    if (c == 0xffffffffu) { if (!l) { keep[row] = 0; drop_na[row] = 0; } return; }
    const PhenoRow r = pheno_row(in, row, c);
    double p = 0.0;
    uint32_t miss = 0;
    for (uint32_t s = l; s < n_samples; s += LANES) {
        const uint64_t den = r.den(s);
        if (!den) ++miss; else p = pheno_add(p, pheno_ratio(r.num(s), den));
    }
#pragma unroll
    for (uint32_t off = LANES / 2; off; off >>= 1) miss += __shfl_down(miss, off, LANES);
    miss = __shfl(miss, 0, LANES);
    double mu = 0.0, dev = 0.0;
    if (miss < n_samples) {                                 // (the same for every lane of the row)
        mu = pheno_mean(pheno_halve<LANES>(p), n_samples - miss);
        double q = 0.0;
        for (uint32_t s = l; s < n_samples; s += LANES) {
            const uint64_t den = r.den(s);
            if (den) q = pheno_add(q, pheno_sq_dev(pheno_ratio(r.num(s), den), mu));
        }
        dev = pheno_sd(pheno_halve<LANES>(q), n_samples);
    }
    if (l) return;
    const uint32_t verdict = pheno_verdict(miss, n_samples, na_num, na_den, dev, min_sd);
    n_na[row] = miss; mean[row] = mu; sd[row] = dev; keep[row] = verdict == 0; drop_na[row] = verdict == 1;
}

// the kept rows side by side, in matrix order: pos = exclusive scan of keep
__global__ __launch_bounds__(256) void k_pheno_scatter(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ n_na,
                                                       const double *__restrict__ mean, const double *__restrict__ sd, uint32_t n,
                                                       uint32_t *__restrict__ o_row, uint32_t *__restrict__ o_n_na, double *__restrict__ o_mean,
                                                       double *__restrict__ o_sd) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const uint32_t k = pos[i];
    o_row[k] = i; o_n_na[k] = n_na[i]; o_mean[k] = mean[i]; o_sd[k] = sd[i];
}

// Entry e = k * n_samples + s of the dense table of the kept rows: the order-preserving key of its z (low and high word) and its sample.  One kept
// row per group of LANES lanes; consecutive lanes write consecutive entries.
template <uint32_t LANES>
__global__ __launch_bounds__(256) void k_pheno_z(PhenoIn in, const uint32_t *__restrict__ o_row, const double *__restrict__ o_mean,
                                                 const double *__restrict__ o_sd, uint32_t n_kept, uint32_t n_samples, uint32_t *__restrict__ z_lo,
                                                 uint32_t *__restrict__ z_hi, uint32_t *__restrict__ e_sample) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t l = threadIdx.x % LANES;
    if (t / LANES >= n_kept) return;
    const uint32_t k = (uint32_t)(t / LANES), row = o_row[k];
    const PhenoRow r = pheno_row(in, row, in.cluster[row]);
    const double mu = o_mean[k], dev = o_sd[k];
    for (uint32_t s = l; s < n_samples; s += LANES) {
        const uint64_t den = r.den(s);
        const uint64_t key = pheno_key(den ? pheno_z(pheno_ratio(r.num(s), den), mu, dev) : 0.0);
        const uint32_t e = k * n_samples + s;               // (below 2^32 - 2^16: checked by the caller)
        z_lo[e] = (uint32_t)key; z_hi[e] = (uint32_t)(key >> 32); e_sample[e] = s;
    }
}

// perm = the entries in stable order of (sample, z): the table is dense, so sample s owns the sorted positions [s * n_kept, (s + 1) * n_kept).
// head[j] = 1 where position j starts a column or a new value of z.
__global__ __launch_bounds__(256) void k_pheno_tie_heads(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ z_lo,
                                                         const uint32_t *__restrict__ z_hi, uint32_t n, uint32_t n_kept, uint32_t *__restrict__ head) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    uint32_t h = 1;
    if (j % n_kept) { const uint32_t a = perm[j], b = perm[j - 1]; h = (z_lo[a] != z_lo[b] || z_hi[a] != z_hi[b]) ? 1u : 0u; }
    head[j] = h;
}

// rank2 of the entry at sorted position j: first + last 1-based place of its run of equal values inside its column (run_start as
// k_cohort_row_start leaves it).  Written through the permutation: entry perm[j] = kept row * n_samples + sample, one writer per word.
__global__ __launch_bounds__(256) void k_pheno_rank(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ head,
                                                    const uint32_t *__restrict__ seg_excl, const uint32_t *__restrict__ run_start, uint32_t n,
                                                    uint32_t n_kept, uint32_t *__restrict__ rank2) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t run = seg_excl[j] + head[j] - 1, col0 = j / n_kept * n_kept;
    rank2[perm[j]] = (run_start[run] - col0 + 1) + (run_start[run + 1] - col0);
}

static inline dim3 pheno_grid(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

void launch_pheno_row_stats(PhenoIn in, uint32_t n, uint32_t n_samples, uint32_t na_num, uint32_t na_den, double min_sd, uint32_t *n_na, double *mean,
                            double *sd, uint32_t *keep, uint32_t *drop_na, hipStream_t st) {
    if (!n) return;
    if (n_samples <= 8) hipLaunchKernelGGL(k_pheno_row_stats<8>, pheno_grid((uint64_t)n * 8), dim3(256), 0, st, in, n, n_samples, na_num, na_den, min_sd,
                                           n_na, mean, sd, keep, drop_na);
    else hipLaunchKernelGGL(k_pheno_row_stats<64>, pheno_grid((uint64_t)n * 64), dim3(256), 0, st, in, n, n_samples, na_num, na_den, min_sd, n_na, mean,
                            sd, keep, drop_na);
}
void launch_pheno_scatter(const uint32_t *keep, const uint32_t *pos, const uint32_t *n_na, const double *mean, const double *sd, uint32_t n,
                          uint32_t *o_row, uint32_t *o_n_na, double *o_mean, double *o_sd, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_pheno_scatter, pheno_grid(n), dim3(256), 0, st, keep, pos, n_na, mean, sd, n, o_row, o_n_na, o_mean, o_sd);
}
void launch_pheno_z(PhenoIn in, const uint32_t *o_row, const double *o_mean, const double *o_sd, uint32_t n_kept, uint32_t n_samples, uint32_t *z_lo,
                    uint32_t *z_hi, uint32_t *e_sample, hipStream_t st) {
    if (!n_kept || !n_samples) return;
    if (n_samples <= 8) hipLaunchKernelGGL(k_pheno_z<8>, pheno_grid((uint64_t)n_kept * 8), dim3(256), 0, st, in, o_row, o_mean, o_sd, n_kept, n_samples,
                                           z_lo, z_hi, e_sample);
    else hipLaunchKernelGGL(k_pheno_z<64>, pheno_grid((uint64_t)n_kept * 64), dim3(256), 0, st, in, o_row, o_mean, o_sd, n_kept, n_samples, z_lo, z_hi,
                            e_sample);
}
void launch_pheno_tie_heads(const uint32_t *perm, const uint32_t *z_lo, const uint32_t *z_hi, uint32_t n, uint32_t n_kept, uint32_t *head,
                            hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_pheno_tie_heads, pheno_grid(n), dim3(256), 0, st, perm, z_lo, z_hi, n, n_kept, head);
}
void launch_pheno_rank(const uint32_t *perm, const uint32_t *head, const uint32_t *seg_excl, const uint32_t *run_start, uint32_t n, uint32_t n_kept,
                       uint32_t *rank2, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_pheno_rank, pheno_grid(n), dim3(256), 0, st, perm, head, seg_excl, run_start, n, n_kept, rank2);
}

}  // namespace rgx
