// qtl_kernels.hip -- device half of the cohort's nominal cis-sQTL scan (rgx_cohort_qtl_nominal, cohort_qtl.cpp; contract in
// include/regtools_amd.h; arithmetic in qtl_core.h, which the host twin runs too).  The reference has no counterpart.
//   k_qtl_residual_pheno / _geno  a wave per table row / per variant: the vector sits in the wave's slice of LDS, where lane l alone touches the
//                 entries s % 64 == l; dot64 is the lane's strided chain and a __shfl_down halving (qtl_tile.h); the C projections run in order.  Written
//                 row-major, 512 contiguous bytes per wave and store.
//   k_qtl_compact the usable variants side by side (their place: a scan of the usable flags): input index, (tid, pos) key, gg
//   k_qtl_transpose  32 x 32 tiles through LDS: the row-major residuals to sample-major Yt[s][k] and Gt[s][u] (u: usable variants in order),
//                 zero behind the last row up to the leading dimension, so that the product kernel's panels are contiguous and need no bounds
//   k_qtl_plan    per row the range [lo, lo + count) of its cis variants among the usable ones, by binary search on the keys
//   k_qtl_tiles   per block of 64 rows the union of its rows' ranges, cut into tiles of 64 variants
//   k_qtl_totals  P and the tile count as 64-bit sums (the 32-bit scans wrap), for the call's one host wait
//   k_qtl_pairs   one workgroup per (row block, variant tile): 4 x 4 chains per thread in registers, each the contract's acc = fma(Y[k][s],
//                 G[v][s], acc) in ascending s from +0.0 -- one thread owns a chain from s = 0 to S - 1.  The samples come in slabs of 16 through
//                 two LDS panels, the next slab's loads in flight under the current slab's FMAs (qtl_tile.h, shared with k_qtl_perm): k_pca_gram's
//                 structure and its conflict-free 16-byte LDS index pattern (pca_kernels.hip).  r and slope are stored where lo[k] <= u < lo[k] + count[k].
//   k_qtl_best    a wave per row over its pairs: largest |r|, earliest on ties, by a shuffle reduction on (|r| bits, pair)
// No atomics, every word has one writer (the two flag words aside: their writers all store 1).  256 threads per workgroup, wave64, FP64 vector
// FMAs (the f64 MFMA's order of adding its four products is not documented: not used).
#include "qtl_tile.h"

namespace rgx {

namespace {

// x (the wave's slice of LDS) -> its residual against the C unit vectors of Q, in place; returns ss
__device__ __forceinline__ double qtl_residual(double *x, uint32_t S, const double *__restrict__ Q, uint32_t C, uint32_t l) {
    for (uint32_t j = 0; j < C; ++j) {
        const double *q = Q + (size_t)j * S;
        const double d = qtl_dot64(x, q, S, l);
        for (uint32_t s = l; s < S; s += 64) x[s] = qtl_project(d, q[s], x[s]);
    }
    return qtl_dot64(x, x, S, l);
}

}  // namespace

// dynamic LDS: 4 * S doubles
__global__ __launch_bounds__(256) void k_qtl_residual_pheno(const uint32_t *__restrict__ rank2, const double *__restrict__ T, uint32_t K, uint32_t S,
                                                            const double *__restrict__ Q, uint32_t C, double *__restrict__ Y, double *__restrict__ yy,
                                                            uint32_t *__restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) double qtl_lds[];
    const uint32_t l = threadIdx.x % 64, w = threadIdx.x / 64;
    const uint64_t k = (uint64_t)blockIdx.x * 4 + w;
    if (k >= K) return;                                      // (a wave leaves whole; no barrier follows)
    double *x = qtl_lds + (size_t)w * S;
    for (uint32_t s = l; s < S; s += 64) {
        const uint32_t r = rank2[k * S + s];
        double v = 0.0;
        if (pca_rank_ok(r, K)) v = T[r - 2]; else flag[kQtlFlagRank] = 1;
        x[s] = v;
    }
    const double ss = qtl_residual(x, S, Q, C, l);
    for (uint32_t s = l; s < S; s += 64) Y[k * S + s] = x[s];
    if (!l) yy[k] = ss;
}

// verdict: the contract's; usable: verdict == 0 as a word for the scan
__global__ __launch_bounds__(256) void k_qtl_residual_geno(const int8_t *__restrict__ dosage, uint32_t V, uint32_t S, const double *__restrict__ Q,
                                                           uint32_t C, double *__restrict__ G, double *__restrict__ gg, uint8_t *__restrict__ verdict,
                                                           uint32_t *__restrict__ usable, uint32_t *__restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) double qtl_lds[];
    const uint32_t l = threadIdx.x % 64, w = threadIdx.x / 64;
    const uint64_t v = (uint64_t)blockIdx.x * 4 + w;
    if (v >= V) return;
    double *x = qtl_lds + (size_t)w * S;
    const int8_t *row = dosage + v * S;
    uint32_t n = 0, sum = 0; int mn = 3, mx = -1;
    for (uint32_t s = l; s < S; s += 64) {
        const int8_t d = row[s];
        if (!qtl_dosage_ok(d)) { flag[kQtlFlagDosage] = 1; continue; }
        if (d < 0) continue;
        ++n; sum += (uint32_t)d; mn = d < mn ? d : mn; mx = d > mx ? d : mx;
    }
#pragma unroll
    for (uint32_t off = 32; off; off >>= 1) {
        n += __shfl_xor(n, off, 64); sum += __shfl_xor(sum, off, 64);
        const int a = __shfl_xor(mn, off, 64), b = __shfl_xor(mx, off, 64);
        mn = a < mn ? a : mn; mx = b > mx ? b : mx;
    }
    if (!n || mn == mx) {                                    // (the same for every lane of the wave)
        if (!l) { gg[v] = 0.0; verdict[v] = 1; usable[v] = 0; }
        return;
    }
    const double mean = qtl_mean(sum, n);
    for (uint32_t s = l; s < S; s += 64) { const int8_t d = row[s]; x[s] = d >= 0 && d <= 2 ? (double)d : mean; }
    const double ss = qtl_residual(x, S, Q, C, l);
    for (uint32_t s = l; s < S; s += 64) G[v * S + s] = x[s];
    if (!l) { const bool ok = qtl_enough(ss, S); gg[v] = ss; verdict[v] = ok ? 0 : 2; usable[v] = ok; }
}

__global__ __launch_bounds__(256) void k_qtl_compact(const uint32_t *__restrict__ usable, const uint32_t *__restrict__ place, uint32_t V,
                                                     const uint32_t *__restrict__ var_tid, const uint32_t *__restrict__ var_pos,
                                                     const double *__restrict__ gg, uint32_t *__restrict__ u_var, uint64_t *__restrict__ u_key,
                                                     double *__restrict__ u_gg) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V || !usable[v]) return;
    const uint32_t u = place[v];
    u_var[u] = v; u_key[u] = qtl_key(var_tid[v], var_pos[v]); u_gg[u] = gg[v];
}

// dst[s * ld + i] = src[(idx ? idx[i] : i) * S + s] for i < *n (n_fixed when n is null), +0.0 for *n <= i < ld
__global__ __launch_bounds__(256) void k_qtl_transpose(const double *__restrict__ src, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ n,
                                                       uint32_t n_fixed, uint32_t S, size_t ld, double *__restrict__ dst) {
    __shared__ double tile[32][33];
    const uint32_t rows = n ? *n : n_fixed, tx = threadIdx.x % 32, ty = threadIdx.x / 32;
    const uint64_t i0 = (uint64_t)blockIdx.x * 32;
    const uint32_t s0 = blockIdx.y * 32;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint64_t i = i0 + ty + 8 * j; const uint32_t s = s0 + tx;
        double v = 0.0;
        if (i < rows && s < S) v = src[(size_t)(idx ? idx[i] : (uint32_t)i) * S + s];
        tile[ty + 8 * j][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t s = s0 + ty + 8 * j; const uint64_t i = i0 + tx;
        if (s < S && i < ld) dst[(size_t)s * ld + i] = tile[tx][ty + 8 * j];
    }
}

// count has K + 1 words: the last is 0, and its place in the scan is P
__global__ __launch_bounds__(256) void k_qtl_plan(const uint32_t *__restrict__ regions, uint32_t K, uint32_t S, const double *__restrict__ yy,
                                                  const uint64_t *__restrict__ u_key, const uint32_t *__restrict__ n_usable, uint32_t window,
                                                  uint32_t *__restrict__ lo, uint32_t *__restrict__ count) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > K) return;
    if (k == K) { count[k] = 0; return; }
    uint32_t a = 0, b = 0;
    if (qtl_enough(yy[k], S)) {
        const uint32_t U = *n_usable, tid = regions[3 * k], start = regions[3 * k + 1], end = regions[3 * k + 2];
        a = qtl_bound(u_key, U, qtl_key_first(tid, start, window), false);
        b = qtl_bound(u_key, U, qtl_key_last(tid, end, window), true);
        if (b < a) b = a;                                    // (a region with end + window < start - window: no pairs)
    }
    lo[k] = a; count[k] = b - a;
}

// tile_count has n_blocks + 1 words: the last is 0
__global__ __launch_bounds__(256) void k_qtl_tiles(const uint32_t *__restrict__ lo, const uint32_t *__restrict__ count, uint32_t K, uint32_t n_blocks,
                                                   uint32_t *__restrict__ blk_lo, uint32_t *__restrict__ tile_count) {
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b > n_blocks) return;
    if (b == n_blocks) { tile_count[b] = 0; return; }
    uint32_t first = 0xffffffffu, last = 0;
    for (uint64_t k = (uint64_t)b * kQtlTile; k < (uint64_t)(b + 1) * kQtlTile && k < K; ++k) if (count[k]) {
        first = lo[k] < first ? lo[k] : first; last = lo[k] + count[k] > last ? lo[k] + count[k] : last;
    }
    blk_lo[b] = first == 0xffffffffu ? 0 : first;
    tile_count[b] = first == 0xffffffffu ? 0 : (last - first + kQtlTile - 1) / kQtlTile;
}

// one workgroup: totals[0] = the sum of count[0 .. K), totals[1] = the sum of tile_count[0 .. n_blocks)
__global__ __launch_bounds__(256) void k_qtl_totals(const uint32_t *__restrict__ count, uint32_t K, const uint32_t *__restrict__ tile_count,
                                                    uint32_t n_blocks, unsigned long long *__restrict__ totals) {
    __shared__ unsigned long long part[2][256];
    unsigned long long a = 0, b = 0;
    for (uint64_t i = threadIdx.x; i < K; i += 256) a += count[i];
    for (uint64_t i = threadIdx.x; i < n_blocks; i += 256) b += tile_count[i];
    qtl_sum2_256(part, a, b);
    if (!threadIdx.x) { totals[0] = part[0][0]; totals[1] = part[1][0]; }
}

// Yt: S rows of ldy doubles, ldy a multiple of 64 at or above K, zero behind K; Gt: S rows of ldg doubles, ldg at or above U + 63, zero behind U
__global__ __launch_bounds__(256) void k_qtl_pairs(const double *__restrict__ Yt, size_t ldy, const double *__restrict__ Gt, size_t ldg, uint32_t S,
                                                   uint32_t K, uint32_t n_blocks, const uint32_t *__restrict__ tile_begin,
                                                   const uint32_t *__restrict__ blk_lo, const uint32_t *__restrict__ lo,
                                                   const uint32_t *__restrict__ count, const uint32_t *__restrict__ pair_begin,
                                                   const double *__restrict__ yy, const double *__restrict__ u_gg, const uint32_t *__restrict__ u_var,
                                                   double *__restrict__ r, double *__restrict__ slope, uint32_t *__restrict__ pair_variant) {
    const uint32_t tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
    // the last row block whose first tile is at or in front of this one (it has tiles: the next block's first tile lies behind this one)
    uint32_t b_lo = 0, b_hi = n_blocks;
    while (b_lo + 1 < b_hi) { const uint32_t mid = b_lo + (b_hi - b_lo) / 2; if (tile_begin[mid] <= blockIdx.x) b_lo = mid; else b_hi = mid; }
    const uint32_t blk = b_lo, k0 = blk * kQtlTile, v0 = blk_lo[blk] + (blockIdx.x - tile_begin[blk]) * kQtlTile;

    double acc[4][4];
    qtl_tile_product(QtlTileRows{Yt + k0 + tid % kQtlTile, ldy}, Gt + v0 + tid % kQtlTile, ldg, S, acc);

#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t k = k0 + qtl_tile_at(i, ty);
        if (k >= K) continue;
        const uint32_t first = lo[k], n = count[k];
        if (!n) continue;
        const uint32_t base = pair_begin[k]; const double y2 = yy[k];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t u = v0 + qtl_tile_at(j, tx);
            if (u < first || u - first >= n) continue;
            const uint32_t p = base + (u - first); const double g2 = u_gg[u];
            r[p] = qtl_r(acc[i][j], y2, g2); slope[p] = qtl_slope(acc[i][j], g2); pair_variant[p] = u_var[u];
        }
    }
}

__global__ __launch_bounds__(256) void k_qtl_best(const double *__restrict__ r, const uint32_t *__restrict__ pair_begin, uint32_t K,
                                                  uint32_t *__restrict__ best) {
    const uint32_t l = threadIdx.x % 64;
    const uint64_t k = (uint64_t)blockIdx.x * 4 + threadIdx.x / 64;
    if (k >= K) return;
    const uint32_t p1 = pair_begin[k + 1];
    unsigned long long bits = 0; uint32_t at = 0xffffffffu;
    for (uint64_t p = (uint64_t)pair_begin[k] + l; p < p1; p += 64) {      // (ascending inside a lane: the earliest of equals stays)
        const unsigned long long x = qtl_abs_bits(r[p]);
        if (at == 0xffffffffu || x > bits) { bits = x; at = (uint32_t)p; }
    }
#pragma unroll
    for (uint32_t off = 32; off; off >>= 1) {
        const unsigned long long ob = __shfl_xor(bits, off, 64); const uint32_t oa = __shfl_xor(at, off, 64);
        if (oa != 0xffffffffu && (at == 0xffffffffu || ob > bits || (ob == bits && oa < at))) { bits = ob; at = oa; }
    }
    if (!l) best[k] = at;
}

void launch_qtl_residual_pheno(const uint32_t *rank2, const double *T, uint32_t K, uint32_t S, const double *Q, uint32_t C, double *Y, double *yy,
                               uint32_t *flag, hipStream_t st) {
    hipLaunchKernelGGL(k_qtl_residual_pheno, dim3((K + 3) / 4), dim3(256), (size_t)4 * S * 8, st, rank2, T, K, S, Q, C, Y, yy, flag);
}
void launch_qtl_residual_geno(const int8_t *dosage, uint32_t V, uint32_t S, const double *Q, uint32_t C, double *G, double *gg, uint8_t *verdict,
                              uint32_t *usable, uint32_t *flag, hipStream_t st) {
    if (!V) return;
    hipLaunchKernelGGL(k_qtl_residual_geno, dim3((V + 3) / 4), dim3(256), (size_t)4 * S * 8, st, dosage, V, S, Q, C, G, gg, verdict, usable, flag);
}
void launch_qtl_compact(const uint32_t *usable, const uint32_t *place, uint32_t V, const uint32_t *var_tid, const uint32_t *var_pos, const double *gg,
                        uint32_t *u_var, uint64_t *u_key, double *u_gg, hipStream_t st) {
    if (!V) return;
    hipLaunchKernelGGL(k_qtl_compact, dim3((V + 255) / 256), dim3(256), 0, st, usable, place, V, var_tid, var_pos, gg, u_var, u_key, u_gg);
}
void launch_qtl_transpose(const double *src, const uint32_t *idx, const uint32_t *n, uint32_t n_fixed, uint32_t S, size_t ld, double *dst,
                          hipStream_t st) {
    hipLaunchKernelGGL(k_qtl_transpose, dim3((uint32_t)((ld + 31) / 32), (S + 31) / 32), dim3(256), 0, st, src, idx, n, n_fixed, S, ld, dst);
}
void launch_qtl_plan(const uint32_t *regions, uint32_t K, uint32_t S, const double *yy, const uint64_t *u_key, const uint32_t *n_usable,
                     uint32_t window, uint32_t *lo, uint32_t *count, uint32_t *blk_lo, uint32_t *tile_count, unsigned long long *totals,
                     hipStream_t st) {
    const uint32_t n_blocks = (K + kQtlTile - 1) / kQtlTile;
    hipLaunchKernelGGL(k_qtl_plan, dim3(K / 256 + 1), dim3(256), 0, st, regions, K, S, yy, u_key, n_usable, window, lo, count);
    hipLaunchKernelGGL(k_qtl_tiles, dim3(n_blocks / 256 + 1), dim3(256), 0, st, lo, count, K, n_blocks, blk_lo, tile_count);
    hipLaunchKernelGGL(k_qtl_totals, dim3(1), dim3(256), 0, st, count, K, tile_count, n_blocks, totals);
}
void launch_qtl_pairs(const double *Yt, size_t ldy, const double *Gt, size_t ldg, uint32_t S, uint32_t K, uint32_t n_tiles, const uint32_t *tile_begin,
                      const uint32_t *blk_lo, const uint32_t *lo, const uint32_t *count, const uint32_t *pair_begin, const double *yy,
                      const double *u_gg, const uint32_t *u_var, double *r, double *slope, uint32_t *pair_variant, hipStream_t st) {
    if (!n_tiles) return;
    hipLaunchKernelGGL(k_qtl_pairs, dim3(n_tiles), dim3(256), 0, st, Yt, ldy, Gt, ldg, S, K, (K + kQtlTile - 1) / kQtlTile, tile_begin, blk_lo, lo,
                       count, pair_begin, yy, u_gg, u_var, r, slope, pair_variant);
}
void launch_qtl_best(const double *r, const uint32_t *pair_begin, uint32_t K, uint32_t *best, hipStream_t st) {
    hipLaunchKernelGGL(k_qtl_best, dim3((K + 3) / 4), dim3(256), 0, st, r, pair_begin, K, best);
}

}  // namespace rgx
