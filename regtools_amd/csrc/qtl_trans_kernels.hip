// qtl_trans_kernels.hip -- device half of the cohort's trans-sQTL scan (rgx_cohort_qtl_trans, cohort_qtl_trans.cpp; contract in
// include/regtools_amd.h; arithmetic in qtl_core.h, which the host twin runs too).  The residuals, the compaction and the sample-major panels are
// the nominal scan's (qtl_kernels.hip); the products are its slab loop (qtl_tile.h).  The reference has no counterpart.
//   k_qtl_trans_count   one workgroup per (row block, variant tile) of ALL n_blocks x n_vt tiles; one behind the last usable variant returns at
//                 once.  Epilogue: each thread tests its 4 x 4 values (row in the table and not flat, variant usable, pair not excluded, then
//                 bits(|r|) >= bits(r_min)); the workgroup's hits and its pairs that met go through shuffles and four LDS words into
//                 tile_hits[tile] and tile_tested[tile].  Which workgroup runs which tile is trans_tile_of's choice and changes no stored word.
//   k_qtl_trans_totals  H and the pairs that met as 64-bit sums (a 32-bit scan wraps where max_hits must be noticed), with the hit tile count, the
//                 two flag words and the usable variants beside them, for the call's one host wait
//   k_qtl_trans_hit_tiles  the tiles with hits side by side (their place: a scan of tile_flag)
//   k_qtl_trans_emit    one workgroup per tile WITH hits: the same chains again, so the same bits; the hits are marked in a 64 x 64 bit matrix in
//                 LDS (a 64-bit word per row, integer OR); a hit's rank is the popcount of the rows before it plus that of the lower bits of its
//                 own row, and (row, usable variant, r, slope) goes to tile_off[tile] + rank
//   k_qtl_trans_gather / _begin  behind the stable sort on the row (launch_radix_pass): the hits in order with their input variants; hit_begin by a
//                 binary search per row
// No floating-point atomics, every global word has one writer.  256 threads per workgroup, wave64, FP64 vector FMAs.
#include "qtl_tile.h"

namespace rgx {

namespace {

// The tile of workgroup b of n.  Consecutive workgroups go round the 8 XCDs, each with an L2 of its own, so the workgroups that share an XCD
// (b % 8 equal) get a contiguous run of places (the bijective form: n need be no multiple of 8), and a place walks super-tiles of `band` row
// blocks: all band blocks of one variant tile, then the next variant tile.  The workgroups an XCD holds at one time then read few panels.
__device__ __forceinline__ uint32_t trans_tile_of(uint32_t b, uint32_t n, uint32_t n_blocks, uint32_t n_vt, uint32_t band) {
    if (!band) return b;
    const uint32_t q = n / 8, rem = n % 8, x = b % 8;
    const uint32_t place = (x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q) + b / 8;
    const uint32_t per_band = band * n_vt, g = place / per_band, in = place % per_band;
    const uint32_t rows_here = n_blocks - g * band < band ? n_blocks - g * band : band;
    return (g * band + in % rows_here) * n_vt + in / rows_here;
}

// This thread's 4 x 4 values of tile (k0, v0): on_hit(i, j, k, u) for every hit; returns its pairs that met.
template <class F>
__device__ __forceinline__ uint32_t trans_visit(const QtlTransTiles &t, uint32_t k0, uint32_t v0, const double (&acc)[4][4], F on_hit) {
    const uint32_t tx = threadIdx.x % 16, ty = threadIdx.x / 16, U = *t.n_usable;
    uint64_t key[4]; double g2[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t u = v0 + qtl_tile_at(j, tx);
        key[j] = u < U ? t.u_key[u] : 0; g2[j] = u < U ? t.u_gg[u] : 0.0;
    }
    uint32_t met = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t k = k0 + qtl_tile_at(i, ty);
        if (k >= t.K) continue;
        const double y2 = t.yy[k];
        if (!qtl_enough(y2, t.S)) continue;
        const uint32_t tid = t.regions[3 * (size_t)k], start = t.regions[3 * (size_t)k + 1], end = t.regions[3 * (size_t)k + 2];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t u = v0 + qtl_tile_at(j, tx);
            if (u >= U || (t.exclude_cis && qtl_key_is_cis(key[j], tid, start, end, t.exclude_window))) continue;
            ++met;
            if (qtl_abs_bits(qtl_r(acc[i][j], y2, g2[j])) >= t.r_min_bits) on_hit(i, j, k, u);
        }
    }
    return met;
}

}  // namespace

__global__ __launch_bounds__(256) void k_qtl_trans_count(QtlTransTiles t, uint32_t band, uint32_t *__restrict__ tile_hits,
                                                         uint32_t *__restrict__ tile_tested, uint32_t *__restrict__ tile_flag) {
    __shared__ uint32_t part[4];
    const uint32_t tid = threadIdx.x;
    const uint32_t tile = trans_tile_of(blockIdx.x, gridDim.x, t.n_blocks, t.n_vt, band);
    const uint32_t k0 = tile / t.n_vt * kQtlTile, v0 = tile % t.n_vt * kQtlTile;
    if (v0 >= *t.n_usable) {                                 // (the same for the whole workgroup)
        if (!tid) { tile_hits[tile] = 0; tile_tested[tile] = 0; tile_flag[tile] = 0; }
        return;
    }
    double acc[4][4];
    qtl_tile_product(QtlTileRows{t.Yt + k0 + tid % kQtlTile, t.ldy}, t.Gt + v0 + tid % kQtlTile, t.ldg, t.S, acc);

    uint32_t hits = 0;
    const uint32_t met = trans_visit(t, k0, v0, acc, [&](uint32_t, uint32_t, uint32_t, uint32_t) { ++hits; });
    uint32_t both = met << 16 | hits;                        // (a tile has at most 4,096 of either: the sums stay inside their halves)
#pragma unroll
    for (uint32_t off = 32; off; off >>= 1) both += __shfl_xor(both, off, 64);
    if (tid % 64 == 0) part[tid / 64] = both;
    __syncthreads();
    if (!tid) {
        both = part[0] + part[1] + part[2] + part[3];
        tile_hits[tile] = both & 0xffffu; tile_tested[tile] = both >> 16; tile_flag[tile] = (both & 0xffffu) != 0;
    }
}

// one workgroup
__global__ __launch_bounds__(256) void k_qtl_trans_totals(const uint32_t *__restrict__ tile_hits, const uint32_t *__restrict__ tile_tested,
                                                          uint32_t n_tiles, const uint32_t *__restrict__ n_hit_tiles,
                                                          const uint32_t *__restrict__ flag, const uint32_t *__restrict__ n_usable,
                                                          unsigned long long *__restrict__ out) {
    __shared__ unsigned long long part[2][256];
    unsigned long long a = 0, b = 0;
    for (uint64_t i = threadIdx.x; i < n_tiles; i += 256) { a += tile_hits[i]; b += tile_tested[i]; }
    qtl_sum2_256(part, a, b);
    if (!threadIdx.x) {
        out[0] = part[0][0]; out[1] = part[1][0]; out[2] = *n_hit_tiles;
        out[3] = (unsigned long long)flag[0] | (unsigned long long)flag[1] << 32; out[4] = *n_usable;
    }
}

__global__ __launch_bounds__(256) void k_qtl_trans_hit_tiles(const uint32_t *__restrict__ tile_flag, const uint32_t *__restrict__ place,
                                                             uint32_t n_tiles, uint32_t *__restrict__ hit_tile) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n_tiles && tile_flag[t]) hit_tile[place[t]] = (uint32_t)t;
}

__global__ __launch_bounds__(256) void k_qtl_trans_emit(QtlTransTiles t, const uint32_t *__restrict__ hit_tile, const uint32_t *__restrict__ tile_off,
                                                        uint32_t *__restrict__ hit_row, uint32_t *__restrict__ hit_u, double *__restrict__ hit_r,
                                                        double *__restrict__ hit_slope) {
    __shared__ unsigned long long bits[kQtlTile];            // row i of the tile: bit j = its value of column j is a hit
    __shared__ uint32_t before[kQtlTile];                    // the hits of the rows in front of row i
    const uint32_t tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
    const uint32_t tile = hit_tile[blockIdx.x];
    const uint32_t k0 = tile / t.n_vt * kQtlTile, v0 = tile % t.n_vt * kQtlTile;
    if (tid < kQtlTile) bits[tid] = 0;                       // (the product's barriers stand between this and the ORs)
    double acc[4][4];
    qtl_tile_product(QtlTileRows{t.Yt + k0 + tid % kQtlTile, t.ldy}, t.Gt + v0 + tid % kQtlTile, t.ldg, t.S, acc);

    uint32_t mine = 0;                                       // bit 4 i + j: acc[i][j] is a hit
    trans_visit(t, k0, v0, acc, [&](uint32_t i, uint32_t j, uint32_t k, uint32_t u) {
        mine |= 1u << (4 * i + j);
        atomicOr(&bits[k - k0], 1ull << (u - v0));
    });
    __syncthreads();
    if (tid < kQtlTile) {
        uint32_t n = 0;
        for (uint32_t i = 0; i < tid; ++i) n += (uint32_t)__popcll(bits[i]);
        before[tid] = n;
    }
    __syncthreads();
    const uint32_t base = tile_off[tile];
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            if (!(mine >> (4 * i + j) & 1u)) continue;
            const uint32_t row = qtl_tile_at(i, ty), col = qtl_tile_at(j, tx), k = k0 + row, u = v0 + col;
            const uint32_t p = base + before[row] + (uint32_t)__popcll(bits[row] & ((1ull << col) - 1));
            const double g2 = t.u_gg[u];
            hit_row[p] = k; hit_u[p] = u; hit_r[p] = qtl_r(acc[i][j], t.yy[k], g2); hit_slope[p] = qtl_slope(acc[i][j], g2);
        }
}

__global__ __launch_bounds__(256) void k_qtl_trans_gather(const uint32_t *__restrict__ perm, uint32_t H, const uint32_t *__restrict__ hit_row,
                                                          const uint32_t *__restrict__ hit_u, const double *__restrict__ hit_r,
                                                          const double *__restrict__ hit_slope, const uint32_t *__restrict__ u_var,
                                                          uint32_t *__restrict__ row_sorted, uint32_t *__restrict__ hit_variant,
                                                          double *__restrict__ r, double *__restrict__ slope) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= H) return;
    const uint32_t j = perm ? perm[i] : (uint32_t)i;
    row_sorted[i] = hit_row[j]; hit_variant[i] = u_var[hit_u[j]]; r[i] = hit_r[j]; slope[i] = hit_slope[j];
}

__global__ __launch_bounds__(256) void k_qtl_trans_begin(const uint32_t *__restrict__ row_sorted, uint32_t H, uint32_t K,
                                                         uint32_t *__restrict__ hit_begin) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > K) return;
    uint32_t lo = 0, hi = H;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (row_sorted[mid] < k) lo = mid + 1; else hi = mid; }
    hit_begin[k] = lo;
}

void launch_qtl_trans_count(const QtlTransTiles &t, uint32_t band, uint32_t *tile_hits, uint32_t *tile_tested, uint32_t *tile_flag, hipStream_t st) {
    const uint32_t n_tiles = t.n_blocks * t.n_vt;
    if (!n_tiles) return;
    hipLaunchKernelGGL(k_qtl_trans_count, dim3(n_tiles), dim3(256), 0, st, t, band, tile_hits, tile_tested, tile_flag);
}
void launch_qtl_trans_totals(const uint32_t *tile_hits, const uint32_t *tile_tested, uint32_t n_tiles, const uint32_t *n_hit_tiles,
                             const uint32_t *flag, const uint32_t *n_usable, unsigned long long *out, hipStream_t st) {
    hipLaunchKernelGGL(k_qtl_trans_totals, dim3(1), dim3(256), 0, st, tile_hits, tile_tested, n_tiles, n_hit_tiles, flag, n_usable, out);
}
void launch_qtl_trans_hit_tiles(const uint32_t *tile_flag, const uint32_t *place, uint32_t n_tiles, uint32_t *hit_tile, hipStream_t st) {
    if (!n_tiles) return;
    hipLaunchKernelGGL(k_qtl_trans_hit_tiles, dim3((n_tiles + 255) / 256), dim3(256), 0, st, tile_flag, place, n_tiles, hit_tile);
}
void launch_qtl_trans_emit(const QtlTransTiles &t, const uint32_t *hit_tile, uint32_t n_hit_tiles, const uint32_t *tile_off, uint32_t *hit_row,
                           uint32_t *hit_u, double *hit_r, double *hit_slope, hipStream_t st) {
    if (!n_hit_tiles) return;
    hipLaunchKernelGGL(k_qtl_trans_emit, dim3(n_hit_tiles), dim3(256), 0, st, t, hit_tile, tile_off, hit_row, hit_u, hit_r, hit_slope);
}
void launch_qtl_trans_order(const uint32_t *perm, uint32_t H, const uint32_t *hit_row, const uint32_t *hit_u, const double *hit_r,
                            const double *hit_slope, const uint32_t *u_var, uint32_t K, uint32_t *row_sorted, uint32_t *hit_variant, double *r,
                            double *slope, uint32_t *hit_begin, hipStream_t st) {
    if (H) hipLaunchKernelGGL(k_qtl_trans_gather, dim3((uint32_t)(((uint64_t)H + 255) / 256)), dim3(256), 0, st, perm, H, hit_row, hit_u, hit_r,
                              hit_slope, u_var, row_sorted, hit_variant, r, slope);
    hipLaunchKernelGGL(k_qtl_trans_begin, dim3(K / 256 + 1), dim3(256), 0, st, row_sorted, H, K, hit_begin);
}

}  // namespace rgx
