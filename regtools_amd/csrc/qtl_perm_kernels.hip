// qtl_perm_kernels.hip -- device half of the cis-sQTL permutation pass (rgx_cohort_qtl_permute, cohort_qtl_perm.cpp; contract in
// include/regtools_amd.h; arithmetic in qtl_core.h, which the host twin runs too).  The residuals, the compaction, the G transpose and the plan are
// qtl_kernels.hip's; the reference has no counterpart.
//   k_qtl_perm       one workgroup per (row k, 64 consecutive permutations): k_qtl_pairs's tile and inner loop with permutations where it has rows.
//                 The row's residual Y[k] sits in LDS (S doubles); the A panel of a slab is gathered from it, A[kk][j] = Ylds[permT[s0 + kk][b0 + j]],
//                 through the sample-major permutation matrix, whose leading dimension is a multiple of 64 padded with index 0, so that consecutive
//                 lanes load consecutive permutations' indices; the B panel comes from Gt as in k_qtl_pairs.  Every chain is the contract's acc =
//                 fma(Y[k][perm[b][s]], G[v][s], acc) in ascending s from +0.0, one thread from s = 0 to S - 1.  The workgroup walks ALL tiles of 64
//                 usable variants of its row's cis range and keeps per permutation the largest |r| bits with the earliest u in registers; the 16
//                 lanes that share a permutation reduce by shuffles and one of them stores perm_r[k][b]: no atomics, no pair ever stored.  A row
//                 without pairs stores +0.0 and leaves.
//   k_qtl_perm_best  a thread per row: the one chain of the winning pair of permutation 0 again, from the row-major residuals: best_variant, best_r,
//                 best_slope -- the chain, qtl_r and qtl_slope of k_qtl_pairs, so the bits are the nominal scan's.
// Every word has one writer.  256 threads per workgroup, wave64, FP64 vector FMAs.
#include "kernels.h"
#include "qtl_core.h"

namespace rgx {

namespace {
constexpr uint32_t kSlab = 16;               // samples per trip through LDS
constexpr uint32_t kPerThread = kSlab * kQtlTile / 256;   // a thread's entries of one panel of one slab
constexpr uint32_t kNoU = 0xffffffffu;
}  // namespace

// Y: K x S row-major; permT: S rows of ldp uint16, ldp a multiple of 64 at or above B + 1, index 0 behind B; Gt: S rows of ldg doubles, ldg at or
// above U + 63, zero behind U.  n_ptiles = ldp / 64; the grid is K * n_ptiles.  Dynamic LDS: S doubles.
__global__ __launch_bounds__(256) void k_qtl_perm(const double *__restrict__ Y, uint32_t S, const uint16_t *__restrict__ permT, size_t ldp,
                                                  uint32_t n_ptiles, uint32_t n_perm1, const double *__restrict__ Gt, size_t ldg,
                                                  const uint32_t *__restrict__ lo, const uint32_t *__restrict__ count,
                                                  const double *__restrict__ yy, const double *__restrict__ u_gg, double *__restrict__ perm_r,
                                                  uint32_t *__restrict__ best_u) {
    extern __shared__ __attribute__((aligned(16))) double y_lds[];
    __shared__ __attribute__((aligned(16))) double A[kSlab][kQtlTile];
    __shared__ __attribute__((aligned(16))) double B[kSlab][kQtlTile];
    const uint32_t tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
    const uint32_t k = blockIdx.x / n_ptiles, b0 = (blockIdx.x % n_ptiles) * kQtlTile;
    const uint32_t first = lo[k], n = count[k];
    double *out = perm_r + (size_t)k * n_perm1;
    if (!n) {                                                // (the same for the whole workgroup)
        if (tid < kQtlTile && b0 + tid < n_perm1) out[b0 + tid] = 0.0;
        if (!b0 && !tid) best_u[k] = kNoU;
        return;
    }
    for (uint32_t s = tid; s < S; s += 256) y_lds[s] = Y[(size_t)k * S + s];
    __syncthreads();
    const double y2 = yy[k];
    const uint16_t *pa = permT + b0 + tid % kQtlTile;

    unsigned long long top[4]; uint32_t top_u[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) { top[i] = 0; top_u[i] = kNoU; }

    for (uint32_t v0 = first; v0 - first < n; v0 += kQtlTile) {
        const double *gb = Gt + v0 + tid % kQtlTile;
        double acc[4][4];
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) acc[i][j] = 0.0;

        uint32_t ia[kPerThread]; double vb[kPerThread];
        auto gather = [&](uint32_t s0) {
#pragma unroll
            for (uint32_t j = 0; j < kPerThread; ++j) {
                const uint32_t s = s0 + tid / kQtlTile + 4 * j;
                ia[j] = s < S ? pa[(size_t)s * ldp] : 0; vb[j] = s < S ? gb[(size_t)s * ldg] : 0.0;
            }
        };
        gather(0);
        for (uint32_t s0 = 0; s0 < S; s0 += kSlab) {
#pragma unroll
            for (uint32_t j = 0; j < kPerThread; ++j) {
                A[tid / kQtlTile + 4 * j][tid % kQtlTile] = y_lds[ia[j]]; B[tid / kQtlTile + 4 * j][tid % kQtlTile] = vb[j];
            }
            __syncthreads();
            if (s0 + kSlab < S) gather(s0 + kSlab);          // (the same for the whole workgroup)
            const uint32_t rows = S - s0 < kSlab ? S - s0 : kSlab;
            auto step = [&](uint32_t kk) {
                const double2 a0 = *(const double2 *)&A[kk][2 * ty], a1 = *(const double2 *)&A[kk][32 + 2 * ty];
                const double2 c0 = *(const double2 *)&B[kk][2 * tx], c1 = *(const double2 *)&B[kk][32 + 2 * tx];
                const double a[4] = {a0.x, a0.y, a1.x, a1.y}, c[4] = {c0.x, c0.y, c1.x, c1.y};
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i)
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) acc[i][j] = qtl_fma(a[i], c[j], acc[i][j]);
            };
            if (rows == kSlab) {
#pragma unroll
                for (uint32_t kk = 0; kk < kSlab; ++kk) step(kk);
            } else {                                         // (its own loop: a padded step would turn an acc of -0.0 into +0.0)
                for (uint32_t kk = 0; kk < rows; ++kk) step(kk);
            }
            __syncthreads();
        }

        // u ascends with j inside a thread and with v0: a strictly larger |r| alone replaces, so the earliest of equals stays
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t u = v0 + (j < 2 ? 0 : 32) + 2 * tx + (j & 1);
            if (u - first >= n) continue;
            const double g2 = u_gg[u];
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                const unsigned long long bits = qtl_abs_bits(qtl_r(acc[i][j], y2, g2));
                if (top_u[i] == kNoU || bits > top[i]) { top[i] = bits; top_u[i] = u; }
            }
        }
    }

    // the 16 lanes tx = 0 .. 15 of one ty share a permutation: they are neighbours inside a wave
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
#pragma unroll
        for (uint32_t off = 8; off; off >>= 1) {
            const unsigned long long ob = __shfl_xor(top[i], off, 64); const uint32_t ou = __shfl_xor(top_u[i], off, 64);
            if (ou != kNoU && (top_u[i] == kNoU || ob > top[i] || (ob == top[i] && ou < top_u[i]))) { top[i] = ob; top_u[i] = ou; }
        }
        const uint32_t b = b0 + (i < 2 ? 0 : 32) + 2 * ty + (i & 1);
        if (tx || b >= n_perm1) continue;
        double v; const unsigned long long bits = top[i];
        memcpy(&v, &bits, 8);
        out[b] = v;
        if (!b) best_u[k] = top_u[i];
    }
}

__global__ __launch_bounds__(256) void k_qtl_perm_best(const double *__restrict__ Y, const double *__restrict__ G, uint32_t K, uint32_t S,
                                                       const uint32_t *__restrict__ best_u, const uint32_t *__restrict__ u_var,
                                                       const double *__restrict__ yy, const double *__restrict__ gg,
                                                       uint32_t *__restrict__ best_variant, double *__restrict__ best_r,
                                                       double *__restrict__ best_slope) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const uint32_t u = best_u[k];
    if (u == kNoU) { best_variant[k] = 0xffffffffu; best_r[k] = 0.0; best_slope[k] = 0.0; return; }
    const uint32_t v = u_var[u];
    const double *y = Y + k * S, *g = G + (size_t)v * S;
    double acc = 0.0;
    for (uint32_t s = 0; s < S; ++s) acc = qtl_fma(y[s], g[s], acc);
    best_variant[k] = v; best_r[k] = qtl_r(acc, yy[k], gg[v]); best_slope[k] = qtl_slope(acc, gg[v]);
}

void launch_qtl_perm(const double *Y, uint32_t K, uint32_t S, const uint16_t *permT, size_t ldp, uint32_t n_perm1, const double *Gt, size_t ldg,
                     const uint32_t *lo, const uint32_t *count, const double *yy, const double *u_gg, double *perm_r, uint32_t *best_u,
                     hipStream_t st) {
    const uint32_t n_ptiles = (uint32_t)(ldp / kQtlTile);
    hipLaunchKernelGGL(k_qtl_perm, dim3(K * n_ptiles), dim3(256), (size_t)S * 8, st, Y, S, permT, ldp, n_ptiles, n_perm1, Gt, ldg, lo, count, yy, u_gg,
                       perm_r, best_u);
}
void launch_qtl_perm_best(const double *Y, const double *G, uint32_t K, uint32_t S, const uint32_t *best_u, const uint32_t *u_var, const double *yy,
                          const double *gg, uint32_t *best_variant, double *best_r, double *best_slope, hipStream_t st) {
    hipLaunchKernelGGL(k_qtl_perm_best, dim3((K + 255) / 256), dim3(256), 0, st, Y, G, K, S, best_u, u_var, yy, gg, best_variant, best_r, best_slope);
}

}  // namespace rgx
