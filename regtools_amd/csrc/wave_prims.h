// wave_prims.h -- the wave and workgroup scans that the extract kernels share (device code only: included by the .hip files, never by host
// code).  Wave width is 64 everywhere (ballot masks are 64-bit).
//   lane_id, lanemask_lt   the lane's number in its wave, and the ballot mask of the lanes below it
//   wave_incl_scan         inclusive sum scan across the 64 lanes of a wave (six shuffles)
//   block_excl_scan_256    exclusive sum scan across a workgroup of 256 threads, and the workgroup's total; s_wave: four words of LDS
// Users: records_kernels.hip, emit_kernels.hip, prims_kernels.hip, members_kernels.hip, reduce_kernels.hip, cse_kernels.hip.
#pragma once
#include "kernels.h"

namespace rgx {

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ uint64_t lanemask_lt() { return (1ull << lane_id()) - 1ull; }

// inclusive scan across the 64 lanes of a wave
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d, 64);
        if ((int)lane_id() >= d) v += t;
    }
    return v;
}

__device__ __forceinline__ uint32_t block_excl_scan_256(uint32_t v, uint32_t *s_wave /*[4]*/, uint32_t &block_total) {
    const uint32_t incl = wave_incl_scan(v);
    const uint32_t w = threadIdx.x >> 6;
    if (lane_id() == 63) s_wave[w] = incl;
    __syncthreads();
    uint32_t off = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) off += (k < w) ? s_wave[k] : 0u;
    block_total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
    return off + incl - v;
}

}  // namespace rgx
