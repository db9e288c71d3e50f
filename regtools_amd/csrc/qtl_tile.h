// qtl_tile.h -- the one slab loop of the sQTL product kernels, with a thread's place in a tile and the totals' block sum (device only): k_qtl_pairs (qtl_kernels.hip), k_qtl_perm (qtl_perm_kernels.hip), k_qtl_perm_cond (qtl_cond_kernels.hip)
// and k_qtl_trans_count / k_qtl_trans_emit (qtl_trans_kernels.hip) run it; they differ in where an entry of the A panel comes from, which a
// small source type says.
#pragma once
#include "kernels.h"
#include "qtl_core.h"

namespace rgx {

constexpr uint32_t kSlab = 16;               // samples per trip through LDS
constexpr uint32_t kPerThread = kSlab * kQtlTile / 256;   // a thread's entries of one panel of one slab

// The A sources.  load(s): what this thread fetches from HBM for sample s (its column is tid % 64), in flight under the previous slab's FMAs;
// stage(raw): the double that goes into the panel.  A Raw{} (sample s >= S) must stage without a fault: its value is never multiplied.
struct QtlTileRows {                         // a column of the sample-major residuals: staged as it is
    using Raw = double;
    const double *col; size_t ld;
    __device__ __forceinline__ Raw load(uint32_t s) const { return col[(size_t)s * ld]; }
    __device__ __forceinline__ double stage(Raw v) const { return v; }
};
struct QtlTilePerms {                        // a column of the sample-major permutation matrix: y[index], y the row's residual in LDS
    using Raw = uint32_t;
    const uint16_t *col; size_t ld; const double *y;
    __device__ __forceinline__ Raw load(uint32_t s) const { return col[(size_t)s * ld]; }
    __device__ __forceinline__ double stage(Raw i) const { return y[i]; }
};

// where a thread's chains lie in the tile: the i-th of its four rows (t = ty = tid / 16) or columns (t = tx = tid % 16)
__device__ __forceinline__ uint32_t qtl_tile_at(uint32_t i, uint32_t t) { return (i < 2 ? 0 : 32) + 2 * t + (i & 1); }

// The contract's dot64 as a wave runs it: lane l alone holds the partial of the entries s % 64 == l, then the halving adds.  Every lane gets P[0].
__device__ __forceinline__ double qtl_halve(double p) {
#pragma unroll
    for (uint32_t off = 32; off; off >>= 1) p = qtl_add(p, __shfl_down(p, off, 64));
    return __shfl(p, 0, 64);                                 // (lane 0 holds P[0]: every lane of the wave gets it)
}
__device__ __forceinline__ double qtl_dot64(const double *a, const double *b, uint32_t S, uint32_t l) {
    double p = 0.0;
    for (uint32_t s = l; s < S; s += 64) p = qtl_fma(a[s], b[s], p);
    return qtl_halve(p);
}

// Two 64-bit sums over the 256 threads of one workgroup: a and b are this thread's shares; behind the return part[0][0] and part[1][0] hold the sums.
__device__ __forceinline__ void qtl_sum2_256(unsigned long long (&part)[2][256], unsigned long long a, unsigned long long b) {
    part[0][threadIdx.x] = a; part[1][threadIdx.x] = b;
    __syncthreads();
    for (uint32_t off = 128; off; off >>= 1) {
        if (threadIdx.x < off) { part[0][threadIdx.x] += part[0][threadIdx.x + off]; part[1][threadIdx.x] += part[1][threadIdx.x + off]; }
        __syncthreads();
    }
}

// acc[i][j] = the contract's chain over s = 0 .. S - 1 from +0.0 of A[s][a(i)] * B[s][b(j)], a(i) = qtl_tile_at(i, ty) with
// ty = tid / 16 and b(j) = qtl_tile_at(j, tx) with tx = tid % 16, for one tile of 64 x 64: 4 x 4 chains per thread in registers, one thread per chain.  The B
// panel is gb[s * ldg] (gb: this thread's column of Gt).  The samples come in slabs of 16 through two LDS panels (16,384 B static), the next
// slab's loads in flight under the current slab's FMAs.  Called by the whole workgroup of 256; it ends behind a barrier, so nothing of the
// panels -- or of what a_src.stage() reads -- is read once it has returned.
template <class ASource>
__device__ __forceinline__ void qtl_tile_product(const ASource &a_src, const double *__restrict__ gb, size_t ldg, uint32_t S, double (&acc)[4][4]) {
    __shared__ __attribute__((aligned(16))) double A[kSlab][kQtlTile];
    __shared__ __attribute__((aligned(16))) double B[kSlab][kQtlTile];
    const uint32_t tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) acc[i][j] = 0.0;

    typename ASource::Raw va[kPerThread]; double vb[kPerThread];
    auto gather = [&](uint32_t s0) {
#pragma unroll
        for (uint32_t j = 0; j < kPerThread; ++j) {
            const uint32_t s = s0 + tid / kQtlTile + 4 * j;
            va[j] = s < S ? a_src.load(s) : typename ASource::Raw{}; vb[j] = s < S ? gb[(size_t)s * ldg] : 0.0;
        }
    };
    gather(0);
    for (uint32_t s0 = 0; s0 < S; s0 += kSlab) {
#pragma unroll
        for (uint32_t j = 0; j < kPerThread; ++j) {
            A[tid / kQtlTile + 4 * j][tid % kQtlTile] = a_src.stage(va[j]); B[tid / kQtlTile + 4 * j][tid % kQtlTile] = vb[j];
        }
        __syncthreads();
        if (s0 + kSlab < S) gather(s0 + kSlab);              // (the same for the whole workgroup)
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
        } else {                                             // (its own loop: a padded step would turn an acc of -0.0 into +0.0)
            for (uint32_t kk = 0; kk < rows; ++kk) step(kk);
        }
        __syncthreads();
    }
}

}  // namespace rgx
