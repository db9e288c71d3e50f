// qtl_perm_kernels.hip -- device half of the cis-sQTL permutation pass, ungrouped and grouped (rgx_cohort_qtl_permute, cohort_qtl_perm.cpp;
// rgx_cohort_qtl_permute_grouped, cohort_qtl_group.cpp; contract in include/regtools_amd.h; arithmetic in qtl_core.h, which the host twins run
// too).  The residuals, the compaction, the G transpose and the plan are qtl_kernels.hip's; the slab loop is qtl_tile.h's, which k_qtl_pairs runs
// too; the reference has no counterpart.  A SERIES is a group of table rows, or -- without member lists -- table row g alone.
//   k_qtl_perm       one workgroup per (series g, 64 consecutive permutations).  It walks the series' members in ascending table row; for every
//                 member with cis variants it brings the member's residual Y[k] into LDS (S doubles) and walks ALL tiles of 64 usable variants of
//                 that member's cis range: k_qtl_pairs's tile and inner loop with permutations where it has rows.  The A panel of a slab is gathered
//                 from LDS, A[kk][j] = Ylds[permT[s0 + kk][b0 + j]], through the sample-major permutation matrix, whose leading dimension is a
//                 multiple of 64 padded with index 0, so that consecutive lanes load consecutive permutations' indices; the B panel comes from Gt
//                 as in k_qtl_pairs.  Every chain is the contract's acc = fma(Y[k][perm[b][s]], G[v][s], acc) in ascending s from +0.0, one thread
//                 from s = 0 to S - 1.  Per permutation the largest |r| bits stay in registers ACROSS tiles and members, beside the place (member
//                 ordinal, u) they were first met at -- u alone for a single member; the 16 lanes that share a permutation reduce by shuffles and
//                 one of them stores perm_r[g][b]: no atomics, no pair ever stored.  A series without pairs stores the +0.0 it began with.
//   k_qtl_perm_best  a thread per series: the one chain of the winning pair of permutation 0 again, from the row-major residuals: best_variant,
//                 best_r, best_slope -- the chain, qtl_r and qtl_slope of k_qtl_pairs, so the bits are the nominal scan's.
// Every word has one writer.  256 threads per workgroup, wave64, FP64 vector FMAs.
#include "qtl_tile.h"

namespace rgx {

namespace {
constexpr uint32_t kNoU = 0xffffffffu;
constexpr unsigned long long kNoPlace = ~0ull;            // (member ordinal << 32 | u) of no pair: above every place
}  // namespace

// Y: K x S row-major; permT: S rows of ldp uint16, ldp a multiple of 64 at or above B + 1, index 0 behind B; Gt: S rows of ldg doubles, ldg at or
// above U + 63, zero behind U.  grp_begin (n_series + 1) and grp_row: the series' member rows, ascending inside a series; a null grp_begin: series
// g is table row g alone, grp_row is not read and best_row, when null, not written.  n_ptiles = ldp / 64; the grid is n_series * n_ptiles.
// Dynamic LDS: S doubles.
__global__ __launch_bounds__(256) void k_qtl_perm(const double *__restrict__ Y, uint32_t S, const uint16_t *__restrict__ permT, size_t ldp,
                                                  uint32_t n_ptiles, uint32_t n_perm1, const double *__restrict__ Gt, size_t ldg,
                                                  const uint32_t *__restrict__ lo, const uint32_t *__restrict__ count,
                                                  const double *__restrict__ yy, const double *__restrict__ u_gg,
                                                  const uint32_t *__restrict__ grp_begin, const uint32_t *__restrict__ grp_row,
                                                  double *__restrict__ perm_r, uint32_t *__restrict__ best_row, uint32_t *__restrict__ best_u) {
    extern __shared__ __attribute__((aligned(16))) double y_lds[];
    const uint32_t tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
    const uint32_t g = blockIdx.x / n_ptiles, b0 = (blockIdx.x % n_ptiles) * kQtlTile;
    const bool listed = grp_begin != nullptr;                // (the same for the whole grid)
    const uint32_t m_begin = listed ? grp_begin[g] : g, m_end = listed ? grp_begin[g + 1] : g + 1;
    auto row_of = [&](uint32_t m) { return listed ? grp_row[m] : m; };
    double *out = perm_r + (size_t)g * n_perm1;
    const QtlTilePerms a_src{permT + b0 + tid % kQtlTile, ldp, y_lds};

    unsigned long long top[4], top_at[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) { top[i] = 0; top_at[i] = kNoPlace; }

    for (uint32_t m = m_begin; m < m_end; ++m) {             // (m, k, first and n are the same for the whole workgroup)
        const uint32_t k = row_of(m), first = lo[k], n = count[k];
        if (!n) continue;
        // No barrier in front of this overwrite: y_lds is read only while a slab is staged, in front of that slab's first barrier, and every
        // thread has passed the barrier that ENDS the previous member's last slab, behind the last reads of the panels and y_lds alike.
        for (uint32_t s = tid; s < S; s += 256) y_lds[s] = Y[(size_t)k * S + s];
        __syncthreads();
        const double y2 = yy[k];
        const unsigned long long ordinal = (unsigned long long)(m - m_begin) << 32;

        for (uint32_t v0 = first; v0 - first < n; v0 += kQtlTile) {
            double acc[4][4];
            qtl_tile_product(a_src, Gt + v0 + tid % kQtlTile, ldg, S, acc);

            // the place ascends with j inside a thread, with v0 and with the member: a strictly larger |r| alone replaces, so the earliest of
            // equals stays
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t u = v0 + qtl_tile_at(j, tx);
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

    // the 16 lanes tx = 0 .. 15 of one ty share a permutation: they are neighbours inside a wave.  A series without pairs has met no barrier and
    // comes here with the bits of +0.0 and no place in every lane.
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
#pragma unroll
        for (uint32_t off = 8; off; off >>= 1) {
            const unsigned long long ob = __shfl_xor(top[i], off, 64), oa = __shfl_xor(top_at[i], off, 64);
            if (oa != kNoPlace && (top_at[i] == kNoPlace || ob > top[i] || (ob == top[i] && oa < top_at[i]))) { top[i] = ob; top_at[i] = oa; }
        }
        const uint32_t b = b0 + qtl_tile_at(i, ty);
        if (tx || b >= n_perm1) continue;
        double v; const unsigned long long bits = top[i];
        memcpy(&v, &bits, 8);
        out[b] = v;
        if (!b) {                                            // (no place: kNoU in both)
            if (best_row) best_row[g] = top_at[i] == kNoPlace ? kNoU : row_of(m_begin + (uint32_t)(top_at[i] >> 32));
            best_u[g] = (uint32_t)top_at[i];
        }
    }
}

// best_row null: series g is table row g
__global__ __launch_bounds__(256) void k_qtl_perm_best(const double *__restrict__ Y, const double *__restrict__ G, uint32_t n_series, uint32_t S,
                                                       const uint32_t *__restrict__ best_row, const uint32_t *__restrict__ best_u,
                                                       const uint32_t *__restrict__ u_var, const double *__restrict__ yy,
                                                       const double *__restrict__ gg, uint32_t *__restrict__ best_variant,
                                                       double *__restrict__ best_r, double *__restrict__ best_slope) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_series) return;
    const uint32_t u = best_u[g];
    if (u == kNoU) { best_variant[g] = 0xffffffffu; best_r[g] = 0.0; best_slope[g] = 0.0; return; }
    const uint32_t k = best_row ? best_row[g] : (uint32_t)g, v = u_var[u];
    const double *y = Y + (size_t)k * S, *x = G + (size_t)v * S;
    double acc = 0.0;
    for (uint32_t s = 0; s < S; ++s) acc = qtl_fma(y[s], x[s], acc);
    best_variant[g] = v; best_r[g] = qtl_r(acc, yy[k], gg[v]); best_slope[g] = qtl_slope(acc, gg[v]);
}

void launch_qtl_perm(const double *Y, uint32_t n_series, uint32_t S, const uint16_t *permT, size_t ldp, uint32_t n_perm1, const double *Gt,
                     size_t ldg, const uint32_t *lo, const uint32_t *count, const double *yy, const double *u_gg, const uint32_t *grp_begin,
                     const uint32_t *grp_row, double *perm_r, uint32_t *best_row, uint32_t *best_u, hipStream_t st) {
    const uint32_t n_ptiles = (uint32_t)(ldp / kQtlTile);
    hipLaunchKernelGGL(k_qtl_perm, dim3(n_series * n_ptiles), dim3(256), (size_t)S * 8, st, Y, S, permT, ldp, n_ptiles, n_perm1, Gt, ldg, lo, count,
                       yy, u_gg, grp_begin, grp_row, perm_r, best_row, best_u);
}
void launch_qtl_perm_best(const double *Y, const double *G, uint32_t n_series, uint32_t S, const uint32_t *best_row, const uint32_t *best_u,
                          const uint32_t *u_var, const double *yy, const double *gg, uint32_t *best_variant, double *best_r, double *best_slope,
                          hipStream_t st) {
    hipLaunchKernelGGL(k_qtl_perm_best, dim3((n_series + 255) / 256), dim3(256), 0, st, Y, G, n_series, S, best_row, best_u, u_var, yy, gg,
                       best_variant, best_r, best_slope);
}

}  // namespace rgx
