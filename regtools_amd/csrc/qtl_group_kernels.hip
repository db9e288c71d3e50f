// qtl_group_kernels.hip -- device half of the grouped cis-sQTL permutation pass (rgx_cohort_qtl_permute_grouped, cohort_qtl_group.cpp; contract in
// include/regtools_amd.h; arithmetic in qtl_core.h, which the host twin runs too).  The residuals, the compaction, the G transpose and the plan are
// qtl_kernels.hip's; the tile and the slab loop are k_qtl_perm's (qtl_perm_kernels.hip), written again here so that kernel stays as it was measured.
//   k_qtl_perm_group  one workgroup per (group g, 64 consecutive permutations).  It walks the group's members in ascending table row; for every
//                 member with cis variants it brings the member's residual Y[k] into LDS (S doubles) and walks ALL tiles of 64 usable variants of
//                 that member's cis range with k_qtl_perm's slab loop: A[kk][j] = Ylds[permT[s0 + kk][b0 + j]], the B panel from Gt, 4 x 4 chains
//                 per thread, every chain the contract's acc = fma(Y[k][perm[b][s]], G[v][s], acc) in ascending s from +0.0.  Per permutation the
//                 largest |r| bits stay in registers ACROSS members, beside the place (member ordinal, u) they were first met at; the 16 lanes
//                 that share a permutation reduce by shuffles and one of them stores perm_r[g][b]: no atomics, no pair ever stored.  A group
//                 without pairs stores +0.0 and leaves.
//   k_qtl_group_best  a thread per group: the one chain of the winning pair of permutation 0 again, from the row-major residuals, as
//                 k_qtl_perm_best runs it, so the bits are the nominal scan's.
// Every word has one writer.  256 threads per workgroup, wave64, FP64 vector FMAs.
#include "kernels.h"
#include "qtl_core.h"

namespace rgx {

namespace {
constexpr uint32_t kSlab = 16;               // samples per trip through LDS
constexpr uint32_t kPerThread = kSlab * kQtlTile / 256;   // a thread's entries of one panel of one slab
constexpr uint32_t kNoU = 0xffffffffu;
constexpr unsigned long long kNoPlace = ~0ull;            // (member ordinal << 32 | u) of no pair: above every place
}  // namespace

// Y, permT, Gt, lo, count, yy, u_gg: as k_qtl_perm takes them.  grp_begin (G + 1) and grp_row: the groups' member rows, ascending inside a group.
// n_ptiles = ldp / 64; the grid is G * n_ptiles.  Dynamic LDS: S doubles.
__global__ __launch_bounds__(256) void k_qtl_perm_group(const double *__restrict__ Y, uint32_t S, const uint16_t *__restrict__ permT, size_t ldp,
                                                        uint32_t n_ptiles, uint32_t n_perm1, const double *__restrict__ Gt, size_t ldg,
                                                        const uint32_t *__restrict__ lo, const uint32_t *__restrict__ count,
                                                        const double *__restrict__ yy, const double *__restrict__ u_gg,
                                                        const uint32_t *__restrict__ grp_begin, const uint32_t *__restrict__ grp_row,
                                                        double *__restrict__ perm_r, uint32_t *__restrict__ best_row,
                                                        uint32_t *__restrict__ best_u) {
    extern __shared__ __attribute__((aligned(16))) double y_lds[];
    __shared__ __attribute__((aligned(16))) double A[kSlab][kQtlTile];
    __shared__ __attribute__((aligned(16))) double B[kSlab][kQtlTile];
    const uint32_t tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
    const uint32_t g = blockIdx.x / n_ptiles, b0 = (blockIdx.x % n_ptiles) * kQtlTile;
    const uint32_t m_begin = grp_begin[g], m_end = grp_begin[g + 1];
    double *out = perm_r + (size_t)g * n_perm1;
    uint32_t any = 0;
    for (uint32_t m = m_begin; m < m_end; ++m) any |= count[grp_row[m]];
    if (!any) {                                              // (the same for the whole workgroup, and in front of every barrier)
        if (tid < kQtlTile && b0 + tid < n_perm1) out[b0 + tid] = 0.0;
        if (!b0 && !tid) { best_row[g] = kNoU; best_u[g] = kNoU; }
        return;
    }
    const uint16_t *pa = permT + b0 + tid % kQtlTile;

    unsigned long long top[4], top_at[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) { top[i] = 0; top_at[i] = kNoPlace; }

    for (uint32_t m = m_begin; m < m_end; ++m) {             // (m, k, first and n are the same for the whole workgroup)
        const uint32_t k = grp_row[m], first = lo[k], n = count[k];
        if (!n) continue;
        // No barrier in front of this overwrite: y_lds is read only while a slab is staged, in front of that slab's first barrier, and every
        // thread has passed the barrier that ENDS the previous member's last slab, behind the last reads of A, B and y_lds alike.
        for (uint32_t s = tid; s < S; s += 256) y_lds[s] = Y[(size_t)k * S + s];
        __syncthreads();
        const double y2 = yy[k];
        const unsigned long long ordinal = (unsigned long long)(m - m_begin) << 32;

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
                if (s0 + kSlab < S) gather(s0 + kSlab);      // (the same for the whole workgroup)
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
                } else {                                     // (its own loop: a padded step would turn an acc of -0.0 into +0.0)
                    for (uint32_t kk = 0; kk < rows; ++kk) step(kk);
                }
                __syncthreads();
            }

            // the place ascends with j inside a thread, with v0 and with the member: a strictly larger |r| alone replaces, so the earliest of
            // equals stays
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t u = v0 + (j < 2 ? 0 : 32) + 2 * tx + (j & 1);
                if (u - first >= n) continue;
                const double g2 = u_gg[u];
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i) {
                    const unsigned long long bits = qtl_abs_bits(qtl_r(acc[i][j], y2, g2));
                    if (top_at[i] == kNoPlace || bits > top[i]) { top[i] = bits; top_at[i] = ordinal | u; }
                }
            }
        }
    }

    // the 16 lanes tx = 0 .. 15 of one ty share a permutation: they are neighbours inside a wave
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
#pragma unroll
        for (uint32_t off = 8; off; off >>= 1) {
            const unsigned long long ob = __shfl_xor(top[i], off, 64), oa = __shfl_xor(top_at[i], off, 64);
            if (oa != kNoPlace && (top_at[i] == kNoPlace || ob > top[i] || (ob == top[i] && oa < top_at[i]))) { top[i] = ob; top_at[i] = oa; }
        }
        const uint32_t b = b0 + (i < 2 ? 0 : 32) + 2 * ty + (i & 1);
        if (tx || b >= n_perm1) continue;
        double v; const unsigned long long bits = top[i];
        memcpy(&v, &bits, 8);
        out[b] = v;
        if (!b) { best_row[g] = grp_row[m_begin + (uint32_t)(top_at[i] >> 32)]; best_u[g] = (uint32_t)top_at[i]; }
    }
}

__global__ __launch_bounds__(256) void k_qtl_group_best(const double *__restrict__ Y, const double *__restrict__ G, uint32_t n_groups, uint32_t S,
                                                        const uint32_t *__restrict__ best_row, const uint32_t *__restrict__ best_u,
                                                        const uint32_t *__restrict__ u_var, const double *__restrict__ yy,
                                                        const double *__restrict__ gg, uint32_t *__restrict__ best_variant,
                                                        double *__restrict__ best_r, double *__restrict__ best_slope) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    const uint32_t u = best_u[g];
    if (u == kNoU) { best_variant[g] = 0xffffffffu; best_r[g] = 0.0; best_slope[g] = 0.0; return; }
    const uint32_t k = best_row[g], v = u_var[u];
    const double *y = Y + (size_t)k * S, *x = G + (size_t)v * S;
    double acc = 0.0;
    for (uint32_t s = 0; s < S; ++s) acc = qtl_fma(y[s], x[s], acc);
    best_variant[g] = v; best_r[g] = qtl_r(acc, yy[k], gg[v]); best_slope[g] = qtl_slope(acc, gg[v]);
}

void launch_qtl_perm_group(const double *Y, uint32_t n_groups, uint32_t S, const uint16_t *permT, size_t ldp, uint32_t n_perm1, const double *Gt,
                           size_t ldg, const uint32_t *lo, const uint32_t *count, const double *yy, const double *u_gg, const uint32_t *grp_begin,
                           const uint32_t *grp_row, double *perm_r, uint32_t *best_row, uint32_t *best_u, hipStream_t st) {
    const uint32_t n_ptiles = (uint32_t)(ldp / kQtlTile);
    hipLaunchKernelGGL(k_qtl_perm_group, dim3(n_groups * n_ptiles), dim3(256), (size_t)S * 8, st, Y, S, permT, ldp, n_ptiles, n_perm1, Gt, ldg, lo,
                       count, yy, u_gg, grp_begin, grp_row, perm_r, best_row, best_u);
}
void launch_qtl_group_best(const double *Y, const double *G, uint32_t n_groups, uint32_t S, const uint32_t *best_row, const uint32_t *best_u,
                           const uint32_t *u_var, const double *yy, const double *gg, uint32_t *best_variant, double *best_r, double *best_slope,
                           hipStream_t st) {
    hipLaunchKernelGGL(k_qtl_group_best, dim3((n_groups + 255) / 256), dim3(256), 0, st, Y, G, n_groups, S, best_row, best_u, u_var, yy, gg,
                       best_variant, best_r, best_slope);
}

}  // namespace rgx
