// prims_kernels.hip -- the two device primitives every stage builds on: the exclusive scan of uint32 and one stable 8-bit LSD radix pass on
// a permutation.  Called through launch_scan_u32 and launch_radix_pass / launch_radix_pass_keyed by the extract pipeline (api_internal.h,
// api_records.cpp, api_reduce.cpp, api_entry.cpp, api_stage.cpp), the identify stages (cse_scan.cpp, cse_join.cpp) and the cohort code
// (cohort.cpp, cohort_cluster.cpp, cohort_pheno.cpp, cohort_qtl*.cpp, qtl_prep.cpp), the sorts through api_internal.h's radix helper.
//   k_scan_reduce    per tile of kScanTile words: the tile's sum
//   k_scan_tiles     one workgroup: exclusive scan of the tile sums, and the total
//   k_scan_apply     per tile: exclusive scan of its words on top of the tile's base
//   k_radix_hist     <KEYED> per tile of 64 x rows keys: the 256 digit counts (digit-major)
//   k_radix_offsets  one workgroup per digit: exclusive scan of its per-tile counts, and the digit's total
//   k_radix_scatter  <KEYED> per tile: the keys' places, stable inside a digit (ballot ranks)
// Constants owned here: kScanTile, kRadixRowsLarge, kRadixRowsSmall, kRadixSmallMax.
#include "wave_prims.h"

#include <algorithm>

namespace rgx {

constexpr uint32_t kScanTile = 4096;   // 256 threads x 16 items

__global__ __launch_bounds__(256) void k_scan_reduce(const uint32_t *__restrict__ in, uint32_t n, uint32_t *tile_sum) {
    __shared__ uint32_t s_wave[4];
    const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * 16;
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) sum += (base + k < n) ? in[base + k] : 0u;
    uint32_t tot; block_excl_scan_256(sum, s_wave, tot);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void k_scan_tiles(uint32_t *tile_sum, uint32_t n_tiles, uint32_t *total) {
    __shared__ uint32_t s_wave[4];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_tiles; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_tiles ? tile_sum[i] : 0u;
        uint32_t tot; const uint32_t ex = block_excl_scan_256(v, s_wave, tot);
        if (i < n_tiles) tile_sum[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0 && total) *total = carry;
}

__global__ __launch_bounds__(256) void k_scan_apply(const uint32_t *__restrict__ in, uint32_t *out, uint32_t n, const uint32_t *__restrict__ tile_sum) {
    __shared__ uint32_t s_wave[4];
    const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * 16;
    uint32_t v[16], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) { v[k] = (base + k < n) ? in[base + k] : 0u; sum += v[k]; }
    uint32_t tot; uint32_t run = block_excl_scan_256(sum, s_wave, tot) + tile_sum[blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) { if (base + k < n) out[base + k] = run; run += v[k]; }
}

size_t scan_tmp_words(uint32_t n) { return (size_t)(n + kScanTile - 1) / kScanTile + 1; }

void launch_scan_u32(const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *total, uint32_t *tmp, hipStream_t stream) {
    if (!n) { if (total) (void)hipMemsetAsync(total, 0, 4, stream); return; }
    const uint32_t tiles = (n + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(k_scan_reduce, dim3(tiles), dim3(256), 0, stream, in, n, tmp);
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(256), 0, stream, tmp, tiles, total);
    hipLaunchKernelGGL(k_scan_apply, dim3(tiles), dim3(256), 0, stream, in, out, n, tmp);
}

// ---- radix pass ------------------------------------------------------------------------------------------
// one wave per workgroup, 64 x rows keys per tile.  Round 4: 8 rows for sorts of up to two million keys -- the partial rows of the group-by, the unique rows
// of the output order: a few hundred thousand keys in 2,048-key tiles are 150 workgroups on 256 CUs, each a chain of 32 dependent rows (a pass 41 us); in
// 512-key tiles four times as many workgroups walk a quarter of the rows each
constexpr uint32_t kRadixRowsLarge = 32, kRadixRowsSmall = 8, kRadixSmallMax = 2u << 20;
static inline uint32_t radix_rows(uint32_t n) {
    return n <= kRadixSmallMax ? kRadixRowsSmall : kRadixRowsLarge;
}

__device__ __forceinline__ uint32_t radix_digit(const uint32_t *__restrict__ word, const uint32_t *__restrict__ perm_in, uint32_t i,
                                                uint32_t shift, uint32_t mask, uint32_t &src) {
    src = perm_in ? perm_in[i] : i;
    return (word[src] >> shift) & mask;
}

// lanes holding the same digit as me (8 ballots)
__device__ __forceinline__ uint64_t match_digit(uint32_t d, bool valid) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
        const uint64_t bal = __ballot((d >> b) & 1u);
        m &= ((d >> b) & 1u) ? bal : ~bal;
    }
    return m;
}

// KEYED = the key of position i is word[i] itself (it travels with the permutation: launch_radix_pass_keyed) instead of word[perm_in[i]]
template <bool KEYED>
__global__ __launch_bounds__(64) void k_radix_hist(const uint32_t *__restrict__ word, uint32_t shift, uint32_t mask,
                                                   const uint32_t *__restrict__ perm_in, uint32_t n, uint32_t n_tiles, uint32_t *hist, uint32_t rows) {
    __shared__ uint32_t s_cnt[256];
    for (uint32_t k = threadIdx.x; k < 256; k += 64) s_cnt[k] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * 64 * rows;
    for (uint32_t r = 0; r < rows; ++r) {
        const uint32_t i = base + r * 64 + threadIdx.x;
        if (i < n) { uint32_t src; atomicAdd(&s_cnt[KEYED ? ((word[i] >> shift) & mask) : radix_digit(word, perm_in, i, shift, mask, src)], 1u); }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < 256; k += 64) hist[(size_t)k * n_tiles + blockIdx.x] = s_cnt[k];   // digit-major
}

template <bool KEYED>
__global__ __launch_bounds__(64) void k_radix_scatter(const uint32_t *__restrict__ word, uint32_t shift, uint32_t mask,
                                                      const uint32_t *__restrict__ perm_in, uint32_t *perm_out, uint32_t n,
                                                      uint32_t n_tiles, const uint32_t *__restrict__ hist_scan, uint32_t *key_out,
                                                      const uint32_t *__restrict__ digit_total, uint32_t rows) {
    __shared__ uint32_t s_base[256];
    {
        // where digit d starts in the output = the totals of the digits below it: 256 numbers, scanned by every workgroup for itself
        // (4 per lane + a wave scan) instead of one more launch; + this tile's rank inside the digit (k_radix_offsets)
        const uint32_t k0 = threadIdx.x * 4;
        const uint32_t t0 = digit_total[k0], t1 = digit_total[k0 + 1], t2 = digit_total[k0 + 2], t3 = digit_total[k0 + 3];
        const uint32_t incl = wave_incl_scan(t0 + t1 + t2 + t3);
        uint32_t run = incl - (t0 + t1 + t2 + t3);
        s_base[k0] = run + hist_scan[(size_t)k0 * n_tiles + blockIdx.x]; run += t0;
        s_base[k0 + 1] = run + hist_scan[(size_t)(k0 + 1) * n_tiles + blockIdx.x]; run += t1;
        s_base[k0 + 2] = run + hist_scan[(size_t)(k0 + 2) * n_tiles + blockIdx.x]; run += t2;
        s_base[k0 + 3] = run + hist_scan[(size_t)(k0 + 3) * n_tiles + blockIdx.x];
    }
    __syncthreads();
    const uint32_t base = blockIdx.x * 64 * rows;
    for (uint32_t r = 0; r < rows; ++r) {
        const uint32_t i = base + r * 64 + threadIdx.x;
        const bool valid = i < n;
        uint32_t src = 0, key = 0;
        uint32_t d = 0;
        if (KEYED) { if (valid) { key = word[i]; src = perm_in ? perm_in[i] : i; d = (key >> shift) & mask; } }
        else d = valid ? radix_digit(word, perm_in, i, shift, mask, src) : 0u;
        const uint64_t m = match_digit(d, valid);
        if (valid) {
            const uint32_t rank = (uint32_t)__popcll(m & lanemask_lt());
            const uint32_t leader = (uint32_t)__ffsll((unsigned long long)m) - 1;
            uint32_t b = 0;
            if (lane_id() == leader) { b = s_base[d]; s_base[d] = b + (uint32_t)__popcll(m); }
            b = __shfl(b, leader, 64);
            perm_out[b + rank] = src;
            if (KEYED) key_out[b + rank] = key;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// one workgroup per digit: exclusive scan of that digit's per-tile counts (in place) + the digit's total
__global__ __launch_bounds__(256) void k_radix_offsets(uint32_t *hist, uint32_t n_tiles, uint32_t *digit_total) {
    __shared__ uint32_t s_wave[4];
    uint32_t *row = hist + (size_t)blockIdx.x * n_tiles;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_tiles; base += 256 * 8) {
        const uint32_t i0 = base + threadIdx.x * 8;
        uint32_t v[8], sum = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) { v[k] = i0 + k < n_tiles ? row[i0 + k] : 0u; sum += v[k]; }
        uint32_t tot; uint32_t ex = carry + block_excl_scan_256(sum, s_wave, tot);
#pragma unroll
        for (int k = 0; k < 8; ++k) { if (i0 + k < n_tiles) row[i0 + k] = ex; ex += v[k]; }
        carry += tot;
    }
    if (threadIdx.x == 0) digit_total[blockIdx.x] = carry;
}

// an upper bound that is MONOTONE in n: a buffer sized for n keys is reused for sorts of fewer keys (the unique rows of a merge), and up to
// kRadixSmallMax keys take the small tiles, which need four times the histogram words per key of the large ones
size_t radix_tmp_words(uint32_t n) {
    const size_t tile = 64 * (size_t)radix_rows(n), tiles = ((size_t)n + tile - 1) / tile;
    const size_t n_small = std::min<size_t>(n, kRadixSmallMax), tile_small = 64 * (size_t)radix_rows((uint32_t)n_small);
    const size_t tiles_small = (n_small + tile_small - 1) / tile_small;
    return 256 * std::max(tiles, tiles_small) + 256 + 4;
}

// a pass = three launches: per-tile digit counts, per-digit scan over the tiles, scatter
void launch_radix_pass(const uint32_t *word, uint32_t shift, uint32_t bits, const uint32_t *perm_in, uint32_t *perm_out, uint32_t n,
                       uint32_t *tmp, hipStream_t stream) {
    if (!n) return;
    const uint32_t rows = radix_rows(n), tiles = (n + 64 * rows - 1) / (64 * rows);
    const uint32_t mask = (1u << bits) - 1u;
    uint32_t *hist = tmp, *totals = tmp + (size_t)256 * tiles;
    hipLaunchKernelGGL(k_radix_hist<false>, dim3(tiles), dim3(64), 0, stream, word, shift, mask, perm_in, n, tiles, hist, rows);
    hipLaunchKernelGGL(k_radix_offsets, dim3(256), dim3(256), 0, stream, hist, tiles, totals);
    hipLaunchKernelGGL(k_radix_scatter<false>, dim3(tiles), dim3(64), 0, stream, word, shift, mask, perm_in, perm_out, n, tiles, hist, (uint32_t *)nullptr, totals, rows);
}
void launch_radix_pass_keyed(const uint32_t *key_in, uint32_t *key_out, uint32_t shift, uint32_t bits, const uint32_t *perm_in, uint32_t *perm_out,
                             uint32_t n, uint32_t *tmp, hipStream_t stream) {
    if (!n) return;
    const uint32_t rows = radix_rows(n), tiles = (n + 64 * rows - 1) / (64 * rows);
    const uint32_t mask = (1u << bits) - 1u;
    uint32_t *hist = tmp, *totals = tmp + (size_t)256 * tiles;
    hipLaunchKernelGGL(k_radix_hist<true>, dim3(tiles), dim3(64), 0, stream, key_in, shift, mask, perm_in, n, tiles, hist, rows);
    hipLaunchKernelGGL(k_radix_offsets, dim3(256), dim3(256), 0, stream, hist, tiles, totals);
    hipLaunchKernelGGL(k_radix_scatter<true>, dim3(tiles), dim3(64), 0, stream, key_in, shift, mask, perm_in, perm_out, n, tiles, hist, key_out, totals, rows);
}

}  // namespace rgx
