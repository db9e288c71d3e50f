// members_kernels.hip -- BGZF member discovery on the device (the container side; the four steps are described in
// kernels.h).  Called by api_internal.h, which lays the steps out for the front of an extract call and for the stage entry points.
//   k_magic_count, k_magic_fill   every byte offset against check_header's predicate, per 4 KiB tile (kMagicTile): count, then fill
//   k_member_link      each candidate to the candidate at its end (binary search), its ISIZE footer, the chain roots
//   k_member_jump      one pointer-doubling round of the reachability from the roots
//   k_member_compact   the reachable candidates as Member rows, and the sizes the arena offsets are scanned from
//   k_member_upos      one workgroup: the 64-bit exclusive scan of those sizes into Member::upos
//   k_member_query     host questions about the list without copying it: compressed offset -> member index and arena offset
//   k_member_fix       the true lengths a probe launch found replace the ISIZE footers
//   k_member_stop      the first member from *from on whose size ends the stream (0, or above 64 KiB)
// The DEFLATE kernels that read the list, and k_members_fetch for a list the host scanned, are kernels.hip's.
#include "wave_prims.h"

namespace rgx {

// check_header (bgzf.c:348-355): ID1 ID2 CM, FLG&4, XLEN == 6, 'B' 'C', SLEN == 2  (bytes 0,1,2,3,10..15)
__device__ __forceinline__ bool bgzf_magic_at(const uint8_t *__restrict__ p) {
    if (p[0] != 31 || p[1] != 139) return false;
    return p[2] == 8 && (p[3] & 4) && p[10] == 6 && p[11] == 0 && p[12] == 'B' && p[13] == 'C' && p[14] == 2 && p[15] == 0;
}

// one thread tests 16 consecutive offsets; a 256-thread workgroup covers one 4 KiB tile
__device__ __forceinline__ uint32_t magic_mask16(const uint8_t *__restrict__ bam, uint64_t len, uint64_t base) {
    uint32_t m = 0;
    if (base + 16 + 18 <= len) {
        // cheap prefilter on the two ID bytes using two aligned-agnostic 16-byte loads
        u32x4 a = ld128(bam + base), b = ld128(bam + base + 16);
        uint8_t w[32];
        *(u32x4 *)w = a; *(u32x4 *)(w + 16) = b;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (w[k] == 31 && w[k + 1] == 139) { if (bgzf_magic_at(bam + base + k)) m |= 1u << k; }
    } else {
        for (int k = 0; k < 16; ++k) if (base + k + 18 <= len && bgzf_magic_at(bam + base + k)) m |= 1u << k;
    }
    return m;
}

__global__ __launch_bounds__(256) void k_magic_count(const uint8_t *__restrict__ bam, uint64_t len, uint32_t *tile_cnt) {
    __shared__ uint32_t s_wave[4];
    const uint64_t base = (uint64_t)blockIdx.x * kMagicTile + threadIdx.x * 16;
    const uint32_t c = (uint32_t)__popc(magic_mask16(bam, len, base));
    uint32_t tot; block_excl_scan_256(c, s_wave, tot);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void k_magic_fill(const uint8_t *__restrict__ bam, uint64_t len, const uint32_t *__restrict__ tile_base, uint64_t *cand) {
    __shared__ uint32_t s_wave[4];
    const uint64_t base = (uint64_t)blockIdx.x * kMagicTile + threadIdx.x * 16;
    uint32_t m = magic_mask16(bam, len, base);
    uint32_t tot; uint32_t slot = tile_base[blockIdx.x] + block_excl_scan_256((uint32_t)__popc(m), s_wave, tot);
    while (m) { const uint32_t k = (uint32_t)__ffs((int)m) - 1; m &= m - 1; cand[slot++] = base + k; }
}

__global__ void k_member_link(const uint8_t *__restrict__ bam, uint64_t len, const uint64_t *__restrict__ cand, uint32_t n, uint32_t *next,
                              uint32_t *isize, uint32_t *reach, uint64_t root2) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t off = cand[i];
    const uint64_t blen = (uint64_t)ld16(bam + off + 16) + 1;       // bgzf.c:525
    uint32_t nx = n, isz = 0xffffffffu;                              // malformed member: chain ends, never inflated
    if (blen >= 26 && off + blen <= len) {
        isz = ld32(bam + off + blen - 4);
        if (isz == 0xffffffffu) isz = 0xfffffffeu;                       // ~0 is the mark of an unusable member; as a footer value both just mean "too big"
        const uint64_t want = off + blen;
        uint32_t lo = i + 1, hi = n;                                 // candidates are sorted by offset
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (cand[mid] < want) lo = mid + 1; else hi = mid; }
        if (lo < n && cand[lo] == want) nx = lo;
    } else nx = 0xffffffffu;                                         // marks "this candidate itself is unusable"
    next[i] = nx; isize[i] = isz;
    // chain roots: the start of the file, and (root2 != ~0) the compressed offset a seek lands on -- bgzf_seek does not care whether
    // the members in front of it still chain up
    reach[i] = ((i == 0 && off == 0) || off == root2) ? 1u : 0u;
}

__global__ void k_member_jump(uint32_t n, const uint32_t *__restrict__ next_in, uint32_t *next_out, uint32_t *reach) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t nx = next_in[i];
    if (nx < n) {
        if (reach[i]) reach[nx] = 1u;                                // 0 -> 1 only: benign race
        next_out[i] = next_in[nx];
    } else next_out[i] = nx;
}

__global__ void k_member_compact(const uint8_t *__restrict__ bam, uint64_t len, const uint64_t *__restrict__ cand, const uint32_t *__restrict__ isize,
                                 const uint32_t *__restrict__ reach, const uint32_t *__restrict__ rank, uint32_t n, Member *members, uint32_t *isize_compact) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !reach[i]) return;
    const uint64_t off = cand[i];
    const uint32_t blen = (uint32_t)ld16(bam + off + 16) + 1;
    const uint32_t r = rank[i];
    // inflate_block (bgzf.c:292-316) hands zlib block_length - 16 bytes from offset 18: the payload AND the footer (a stream that ends late
    // eats CRC bytes instead of failing, e.g. when BSIZE is one short).  Here: everything up to the member's end, clipped so that the
    // decoder's 16-byte look-ahead stays inside the documented bam_len + 8 readable bytes.
    Member m; m.cpos = off + 18; m.upos = 0; m.isize = isize[i];
    m.clen = blen >= 26 ? blen - 18 : 0;
    if (m.cpos + m.clen + 8 > len) m.clen = len > m.cpos + 8 ? (uint32_t)(len - 8 - m.cpos) : 0;
    members[r] = m;
    isize_compact[r] = (isize[i] <= kBgzfMaxBlock) ? isize[i] : 0u;  // oversized/unusable members hold no bytes in the arena
}

// one block (the member count lives on the device; no host round trip): 256 threads x 8 consecutive members per trip
__global__ __launch_bounds__(256) void k_member_upos(Member *members, const uint32_t *__restrict__ isz, const uint32_t *__restrict__ n_ptr, uint64_t *total) {
    __shared__ uint32_t s_wave[4];
    const uint32_t n = *n_ptr;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < n; base += 2048) {
        const uint32_t i0 = base + threadIdx.x * 8;
        uint32_t v[8], sum = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) { v[k] = i0 + k < n ? isz[i0 + k] : 0u; sum += v[k]; }     // 2048 * 65536 < 2^32
        uint32_t tot; uint32_t ex = block_excl_scan_256(sum, s_wave, tot);
#pragma unroll
        for (int k = 0; k < 8; ++k) { if (i0 + k < n) members[i0 + k].upos = carry + ex; ex += v[k]; }
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ void k_member_query(const Member *__restrict__ members, const uint32_t *__restrict__ n_ptr, const uint64_t *__restrict__ q_coff, uint32_t n_q,
                               uint32_t *q_index, uint64_t *q_upos) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_q) return;
    const uint32_t n = *n_ptr;
    const uint64_t want = q_coff[k] + 18;
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (members[mid].cpos < want) lo = mid + 1; else hi = mid; }
    const bool hit = lo < n && members[lo].cpos == want;
    q_index[k] = hit ? lo : n;
    q_upos[k] = hit ? members[lo].upos : ~0ull;
}

// the true lengths a probe launch found replace the ISIZE footers (members and the compact copy the offsets are scanned from)
__global__ void k_member_fix(Member *members, uint32_t *isize_compact, const uint32_t *__restrict__ n_ptr, const uint32_t *__restrict__ fix) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *n_ptr) return;
    const uint32_t sz = fix[i];
    members[i].isize = sz;
    isize_compact[i] = sz <= kBgzfMaxBlock ? sz : 0u;
}
__global__ void k_member_stop(const Member *__restrict__ members, const uint32_t *__restrict__ n_ptr, const uint32_t *__restrict__ from_ptr, uint32_t *stop) {
    const uint32_t n = *n_ptr;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < *from_ptr) return;
    if (i < n && (members[i].isize == 0 || members[i].isize > kBgzfMaxBlock)) atomicMin(stop, i);
}

void launch_magic_count(const uint8_t *bam, uint64_t len, uint32_t n_tiles, uint32_t *tile_cnt, hipStream_t stream) {
    if (n_tiles) hipLaunchKernelGGL(k_magic_count, dim3(n_tiles), dim3(256), 0, stream, bam, len, tile_cnt);
}
void launch_magic_fill(const uint8_t *bam, uint64_t len, uint32_t n_tiles, const uint32_t *tile_base, uint64_t *cand, hipStream_t stream) {
    if (n_tiles) hipLaunchKernelGGL(k_magic_fill, dim3(n_tiles), dim3(256), 0, stream, bam, len, tile_base, cand);
}
void launch_member_link(const uint8_t *bam, uint64_t len, const uint64_t *cand, uint32_t n, uint32_t *next, uint32_t *isize, uint32_t *reach,
                        uint64_t root2, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_member_link, dim3((n + 255) / 256), dim3(256), 0, stream, bam, len, cand, n, next, isize, reach, root2);
}
void launch_member_jump(uint32_t n, const uint32_t *next_in, uint32_t *next_out, uint32_t *reach, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_member_jump, dim3((n + 255) / 256), dim3(256), 0, stream, n, next_in, next_out, reach);
}
void launch_member_compact(const uint8_t *bam, uint64_t len, const uint64_t *cand, const uint32_t *isize, const uint32_t *reach, const uint32_t *rank, uint32_t n,
                           Member *members, uint32_t *isize_compact, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_member_compact, dim3((n + 255) / 256), dim3(256), 0, stream, bam, len, cand, isize, reach, rank, n, members, isize_compact);
}
void launch_member_upos(Member *members, const uint32_t *isize_compact, const uint32_t *n_members, uint64_t *total, hipStream_t stream) {
    hipLaunchKernelGGL(k_member_upos, dim3(1), dim3(256), 0, stream, members, isize_compact, n_members, total);
}
void launch_member_query(const Member *members, const uint32_t *n_members, const uint64_t *q_coff, uint32_t n_q, uint32_t *q_index, uint64_t *q_upos,
                         hipStream_t stream) {
    if (n_q) hipLaunchKernelGGL(k_member_query, dim3((n_q + 63) / 64), dim3(64), 0, stream, members, n_members, q_coff, n_q, q_index, q_upos);
}
void launch_member_fix(Member *members, uint32_t *isize_compact, uint32_t max_members, const uint32_t *n_members, const uint32_t *fix, hipStream_t stream) {
    if (max_members) hipLaunchKernelGGL(k_member_fix, dim3((max_members + 255) / 256), dim3(256), 0, stream, members, isize_compact, n_members, fix);
}
void launch_member_stop(const Member *members, uint32_t max_members, const uint32_t *n_members, const uint32_t *from, uint32_t *stop, hipStream_t stream) {
    if (max_members) hipLaunchKernelGGL(k_member_stop, dim3((max_members + 255) / 256), dim3(256), 0, stream, members, n_members, from, stop);
}

}  // namespace rgx
