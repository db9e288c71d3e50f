// kernels.hip -- the DEFLATE kernels of the junctions-extract hot path, hand-written for gfx950 (CDNA4): BGZF members to the inflated arena
// (SURVEY.md 8a row a1).  Called by api_front.cpp, api_entry.cpp and api_records.cpp; the decoders themselves are inflate_core.h, inflate_ring.h,
// inflate_coop.h and inflate_wave.h, which the host emulation compiles too.
//   k_inflate          <PROBE, PIECE, LITS> one lane per member, every lane copies its own matches
//   k_inflate_ring     <PROBE> the lane form with its output in a per-lane LDS ring, flushed by the wave in whole 128-byte lines
//   k_inflate_coop     <PROBE, PIECE, WIN> the lane form with long matches moved by the wave; the arrival gate of the overlapped upload
//   k_inflate_wave     one member per wave, the whole member in LDS: small inputs
//   k_member_sort      k_inflate_coop's lane assignment: per group of kSortGroup members, their indices by compressed length
//   k_members_check    a caller's own member list: does its layout suit k_inflate_coop's 32-bit offsets
//   k_wait_done, k_gate_set, k_members_fetch   the early tail's wait for a part of the launch; an upload chunk's flag word; the host scan's member list into HBM
// What a member that did not inflate reports is written once, in front of k_inflate: member_verdict, report_bad_member.  Constants owned here:
// kHotSyms and the layout of the symbol lists, kRingLdsBytes, kSortGroup, kWaveFormMaxMembers, kDefaultLaneForm, kDefaultWindow.  Per-lane
// latency bounds this file, HBM traffic the others; there is deliberately no MFMA anywhere.  The rest of the extract path: members_kernels.hip,
// records_kernels.hip, emit_kernels.hip, prims_kernels.hip, reduce_kernels.hip, over wave_prims.h; kernels.h declares all their launchers.
#include "kernels.h"

#include <mutex>
#include <type_traits>

#include "bam_core.h"
#include "inflate_core.h"
#include "inflate_coop.h"
#include "inflate_ring.h"
#include "inflate_wave.h"

namespace rgx {

// =====================================================================================================
// a1. BGZF inflate: ONE LANE PER MEMBER (64 members per wavefront, one wave per workgroup)
// =====================================================================================================
// Per-lane Huffman symbol lists, lane-interleaved so that lane L only ever touches LDS bank L % 32, bit-packed:
//   ll_sym : 288 x 9 bits, sorted by (code length, symbol): the first kHotSyms entries -- the SHORTEST, i.e. most frequent,
//            codes -- in LDS dwords 0..kLdsD-1, the long-code tail in the global scratch (one dependent L2 read per rare symbol)
//   d_sym  :  32 x 5 bits -> LDS dwords kLdsD..kLdsD+4                    + 1 pad dword
// What the split buys is occupancy: LDS per wave = kLdsDwordsPerLane * 256 B decides how many waves (each 64 members) a CU of
// 160 KiB holds, and a lane's trip is a chain of dependent ALU/LDS steps plus one memory round trip -- the other waves of
// the SIMD are what fills those gaps (measured with the output stage in place: 5 -> 7 waves per CU is 1.3x).
// The canonical codes themselves (bounds, lengths, list offsets) are 2 x 16 REGISTER words (inflate_core.h Code); the
// code-length scratch that only a block header needs is global too (40 dwords per lane, before the cold symbols).
#ifndef RGX_LAB_HOT_SYMS
#define RGX_LAB_HOT_SYMS 160
#endif
constexpr uint32_t kHotSyms = RGX_LAB_HOT_SYMS;
constexpr uint32_t kLdsLL = 0, kLdsD = (kHotSyms * 9 + 31) / 32, kLdsDwordsPerLane = kLdsD + 6;
constexpr uint32_t kInflateLdsBytes = kLdsDwordsPerLane * 64 * 4;
// (round 4: the cold end of the list is 16 bits per symbol -- ONE request per lookup, no read-modify-write when the list is built)
constexpr uint32_t kScratchLenWords = 40, kScratchColdWords = (288 - kHotSyms + 1) / 2;
constexpr uint32_t kScratchWordsPerLane = kScratchLenWords + kScratchColdWords;

struct LdsTab {
    static constexpr bool kIsHandle = true;     // (pointers into LDS and scratch: block_header_call copies the handle, not tables)
    uint32_t *base;       // LDS, already offset by lane
    uint32_t *scratch;    // global, already offset by global lane
    uint32_t stride;      // lanes in the grid (dword stride of the scratch)
    __device__ __forceinline__ uint32_t rd(uint32_t dw) const { return base[dw * 64]; }
    __device__ __forceinline__ void wr(uint32_t dw, uint32_t v) { base[dw * 64] = v; }
    __device__ __forceinline__ uint32_t grd(uint32_t dw) const { return scratch[(size_t)dw * stride]; }
    __device__ __forceinline__ void gwr(uint32_t dw, uint32_t v) { scratch[(size_t)dw * stride] = v; }
    __device__ __forceinline__ uint32_t get_bits(uint32_t dw0, uint32_t bit, uint32_t width) const {
        const uint32_t dw = dw0 + (bit >> 5), sh = bit & 31;
        const uint64_t w = (uint64_t)rd(dw) | (uint64_t)rd(dw + 1) << 32;
        return (uint32_t)(w >> sh) & ((1u << width) - 1u);
    }
    __device__ __forceinline__ void set_bits(uint32_t dw0, uint32_t bit, uint32_t width, uint32_t v) {
        const uint32_t dw = dw0 + (bit >> 5), sh = bit & 31;
        uint64_t w = (uint64_t)rd(dw) | (uint64_t)rd(dw + 1) << 32;
        const uint64_t m = (uint64_t)((1u << width) - 1u) << sh;
        w = (w & ~m) | ((uint64_t)v << sh);
        wr(dw, (uint32_t)w);
        if (sh + width > 32) wr(dw + 1, (uint32_t)(w >> 32));
    }
    // cold symbols: two per dword of the lane's scratch column
    __device__ __forceinline__ uint32_t get_cold(uint32_t c) const { return (grd(kScratchLenWords + (c >> 1)) >> (16u * (c & 1u))) & 0x1ffu; }
    __device__ __forceinline__ void set_cold(uint32_t c, uint32_t v) {
        ((uint16_t *)(scratch + (size_t)(kScratchLenWords + (c >> 1)) * stride))[c & 1u] = (uint16_t)v;
    }
    __device__ __forceinline__ uint32_t get_ll_sym(uint32_t i) const { return i < kHotSyms ? get_bits(kLdsLL, i * 9, 9) : get_cold(i - kHotSyms); }
    __device__ __forceinline__ void set_ll_sym(uint32_t i, uint32_t v) { if (i < kHotSyms) set_bits(kLdsLL, i * 9, 9, v); else set_cold(i - kHotSyms, v); }
    __device__ __forceinline__ uint32_t get_d_sym(uint32_t i) const { return get_bits(kLdsD, i * 5, 5); }
    __device__ __forceinline__ void set_d_sym(uint32_t i, uint32_t v) { set_bits(kLdsD, i * 5, 5, v); }
    __device__ __forceinline__ uint32_t get_len_word(uint32_t w) const { return grd(w); }
    __device__ __forceinline__ void set_len_word(uint32_t w, uint32_t v) { gwr(w, v); }
    __device__ __forceinline__ void clear_syms() {}
};

// What a member's claim about its size and the decoder's answer come to.  A member whose claimed size is no BGZF block size owns no bytes of the
// arena (k_member_compact): it must not write any, whatever range the host asked for, so the decoder did not run for it (ran = false).  ~0 = the
// member runs past the end of the file (k_member_link).  A member that ran must inflate to exactly the size it claims.
// (k_inflate and k_inflate_wave branch round the decoder on `isize > kBgzfMaxBlock` -- !run of the other two -- and call this on either side: same code as before)
__device__ __forceinline__ int member_verdict(const Member &mb, bool ran, int st, uint32_t out_len) {
    if (!ran) st = mb.isize == 0xffffffffu ? INF_IN_OVERRUN : INF_OUT_OVERFLOW;
    else if (st == INF_OK && out_len != mb.isize) st = INF_SIZE_MISMATCH;
    return st;
}
// What a member that did not inflate reports.  Members in front of a seek target (below ignore_below) are inflated for the header only: their
// failures do not end the record stream and are reported apart (the header read and the footer check still want to know).
__device__ __forceinline__ void report_bad_member(uint32_t m, uint32_t index_bias, uint32_t ignore_below, uint32_t *status, uint8_t *bad, int code) {
    const uint32_t mi = m + index_bias;       // (index in the caller's member range: a range may be launched in several pieces)
    if (bad) bad[mi] = 1;
    uint32_t *slot = mi >= ignore_below ? status : status + kStatusEarly;
    const uint32_t prev = atomicMin(&slot[0], mi);
    if (mi < prev) slot[1] = (uint32_t)code;  // best effort: status of (one of) the earliest bad members
}

// PROBE = false: the pipeline's launch -- member m goes to its planned place arena + upos (planned from the ISIZE footers) and must
// inflate to exactly ISIZE bytes.  PROBE = true: the repair launch for files whose footers lie (bgzf.c:292-316 never reads ISIZE: a
// block is as long as zlib says): every member into its own 64 KiB slot, true length (or ~0 = does not inflate) to sizes[m].
// PIECE: the same code under a second symbol -- the launches of rgx_extract_mem's overlapped upload cover a third of a file each and
// run side by side; a profiler's per-kernel statistics keep them apart from the whole-range launches the roofline is quoted on.
template <bool PROBE, bool PIECE = false, int LITS = 1 /* literals per trip (inflate_core.h): 4 for payloads that are mostly literals */>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_inflate(const uint8_t *__restrict__ comp, const Member *__restrict__ members,
                                                uint32_t n_members, uint8_t *__restrict__ arena, uint64_t upos_bias, uint32_t *len_scratch,
                                                uint32_t *status, uint32_t ignore_below, uint32_t index_bias, uint8_t *bad) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t m = blockIdx.x * 64 + threadIdx.x;
    if (m >= n_members) return;
    Member mb = members[m];
    LdsTab T{lds + threadIdx.x, len_scratch + m, gridDim.x * 64};
    uint32_t out_len = 0;
    if (PROBE) {
        if (mb.isize == 0xffffffffu) { status[m] = 0xffffffffu; return; }   // k_member_link: BSIZE runs past the end of the file (or is < 26): the read fails upstream
        const int st = inflate_raw(comp + mb.cpos, mb.clen, arena + (uint64_t)m * kBgzfMaxBlock, kBgzfMaxBlock, &out_len, T);
        status[m] = st == INF_OK ? out_len : 0xffffffffu;
        return;
    }
    int st;
    if (mb.isize > kBgzfMaxBlock) st = member_verdict(mb, false, INF_OK, 0);           // (= !run of the other kernels: owns no bytes of the arena, the decoder does not run)
    else {
        st = inflate_raw<LITS>(comp + mb.cpos, mb.clen, arena + (mb.upos - upos_bias), mb.isize, &out_len, T);
        st = member_verdict(mb, true, st, out_len);
    }
    if (st != INF_OK) report_bad_member(m, index_bias, ignore_below, status, bad, st);
}

// ---- round 2: the same decoder with its output in LDS (inflate_ring.h) --------------------------------------------------------------
// LDS of one wave (= one workgroup): [symbol lists, kLdsDwordsPerLane x 64 dwords][rings, kRingLaneDw x 64 dwords][flush work list, 128 x 4].
// Everything is dword-interleaved across the lanes (dword d of lane L at d * 64 + L), so a lane only ever touches bank L % 32 and
// consecutive dwords of a lane are one ds_read2st64_b32 / ds_write2st64_b32 apart.  159 dwords per lane = 40 704 B per wave: four waves per CU.
constexpr uint32_t kRingLdsDwords = (kLdsDwordsPerLane + kRingLaneDw + 8) * 64;      // (flush list: 128 items of 4 dwords)
constexpr uint32_t kRingLdsBytes = kRingLdsDwords * 4;

struct LdsRing {
    uint32_t *base;       // LDS, already offset by lane
    __device__ __forceinline__ uint32_t rd(uint32_t dw) const { return base[dw * 64]; }
    __device__ __forceinline__ void rd4(uint32_t dw, uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d) const {
        const uint32_t *q = base + dw * 64;
        a = q[0]; b = q[64]; c = q[128]; d = q[192];
    }
    __device__ __forceinline__ void wr4(uint32_t dw, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
        uint32_t *q = base + dw * 64;
        q[0] = a; q[64] = b; q[128] = c; q[192] = d;
    }
    __device__ __forceinline__ void wr8(uint32_t byte_pos, uint32_t b) { ((uint8_t *)(base + (byte_pos >> 2) * 64))[byte_pos & 3u] = (uint8_t)b; }
};

// The wave as a flushing machine.  A flush round: every lane with complete lines appends one 16-byte work item per line {line base
// address, position, ring line, member} to a list in LDS (slots from ballots: no atomics); then lane j stores piece j & 7 (16 bytes) of
// item 8 * step + (j >> 3): one store instruction = eight whole, aligned 128-byte lines, and only as many instructions as there are lines.
// Four steps are read before the first is stored, so a round waits on LDS twice, not per line.  (A member's ring lives in ONE bank, so
// the eight lanes of a line take turns on it: 32 LDS cycles per eight lines -- LDS time well spent: what HBM sees is each output byte
// once, in full lines.)
struct WaveCoop {
    uint32_t *ring_wave;  // LDS: dword d of lane L's ring at ring_wave[d * 64 + L]
    uint32_t *list;       // LDS: 128 work items of 4 dwords
    uint32_t lane;
    __device__ __forceinline__ bool any(bool b) const { return __builtin_amdgcn_ballot_w64(b) != 0; }
    __device__ __forceinline__ void flush_lines(const LdsRing &R, RingOut &O) const {
        if (O.fl & 127u) {                                        // the partial line in front of the member's first boundary: this lane alone
            const uint32_t c = (O.fl + 127u) & ~127u;
            if (O.hd >= c) { O.slow_flush(R, O.fl, c); O.fl = c; }
        }
        const uint32_t nl = (O.fl & 127u) ? 0u : (O.hd - O.fl) >> 7;            // 0..2 (head - flushed <= kRingFill)
        const uint64_t m0 = __builtin_amdgcn_ballot_w64(nl > 0), m1 = __builtin_amdgcn_ballot_w64(nl > 1);
        const uint32_t c0 = (uint32_t)__popcll(m0), total = c0 + (uint32_t)__popcll(m1);
        if (!total) return;
        const uint64_t lt = (1ull << lane) - 1ull;
        {
            const uint64_t a = (uint64_t)(uintptr_t)O.lbase;
            uint32_t line = (O.fl % kRingBytes) >> 7;
            if (nl > 0) { const u32x4 e = {(uint32_t)a, (uint32_t)(a >> 32), O.fl, line << 8 | lane}; *(u32x4 *)(list + 4 * (uint32_t)__popcll(m0 & lt)) = e; }
            if (nl > 1) {
                if (++line >= 3) line = 0;
                const u32x4 e = {(uint32_t)a, (uint32_t)(a >> 32), O.fl + 128, line << 8 | lane}; *(u32x4 *)(list + 4 * (c0 + (uint32_t)__popcll(m1 & lt))) = e;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const uint32_t piece = lane & 7u, sub = lane >> 3;
        for (uint32_t base = 0; base < total; base += 32) {
            u32x4 e[4], v[4];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const uint32_t k = base + 8 * s4 + sub;
                e[s4] = *(const u32x4 *)(list + 4 * (k < total ? k : total - 1));
            }
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const uint32_t *q = ring_wave + ((e[s4][3] >> 8) * 32 + piece * 4) * 64 + (e[s4][3] & 0xffu);
                v[s4] = u32x4{q[0], q[64], q[128], q[192]};
            }
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                if (base + 8 * s4 + sub < total) {
                    uint8_t *dst = (uint8_t *)(uintptr_t)((uint64_t)e[s4][0] | (uint64_t)e[s4][1] << 32) + e[s4][2] + 16 * piece;
                    *(u32x4 *)dst = v[s4];
                }
            }
        }
        O.fl += 128 * nl;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();                             // (the list is rewritten by the next round)
    }
};

template <bool PROBE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_inflate_ring(const uint8_t *__restrict__ comp, const Member *__restrict__ members,
                                                uint32_t n_members, uint8_t *arena, uint64_t upos_bias, uint32_t *len_scratch,
                                                uint32_t *status, uint32_t ignore_below, uint32_t index_bias, uint8_t *bad) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t m = blockIdx.x * 64 + lane;
    const bool have = m < n_members;
    Member mb = members[have ? m : n_members - 1];
    LdsTab T{lds + lane, len_scratch + (have ? m : 0), gridDim.x * 64};
    LdsRing R{lds + kLdsDwordsPerLane * 64 + lane};
    WaveCoop C{lds + kLdsDwordsPerLane * 64, lds + (kLdsDwordsPerLane + kRingLaneDw) * 64, lane};
    uint32_t out_len = 0;
    if (PROBE) {
        const bool run = have && mb.isize != 0xffffffffu;         // ~0: BSIZE runs past the end of the file (or is < 26): the read fails upstream
        const int st = inflate_ring(comp + mb.cpos, mb.clen, arena + (uint64_t)(have ? m : 0) * kBgzfMaxBlock, kBgzfMaxBlock, &out_len, T, R, C, run);
        if (have) status[m] = run && st == INF_OK ? out_len : 0xffffffffu;
        return;
    }
    const bool run = have && mb.isize <= kBgzfMaxBlock;           // (member_verdict: the others own no bytes of the arena)
    int st = inflate_ring(comp + mb.cpos, mb.clen, arena + (run ? mb.upos - upos_bias : 0), run ? mb.isize : 0, &out_len, T, R, C, run);
    if (!have) return;
    st = member_verdict(mb, run, st, out_len);
    if (st != INF_OK) report_bad_member(m, index_bias, ignore_below, status, bad, st);
}

// ---- round 3: long copies moved by the wave (inflate_coop.h) ---------------------------------------------------------------------------
// The wave as a copying machine.  A round serves up to four pending long copies, sixteen lanes each: the owners' lane numbers come from a
// ballot (scalar bit scans), every lane pulls its group's copy -- destination of the first whole chunk (relative to the wave's lowest output
// address: the members of a wave lie next to each other in the arena), distance, chunk count -- with two ds_bpermute, loads 16 bytes from
// (chunk j) - distance and, after the trip's one wait, stores them to chunk j: aligned, and 256 consecutive bytes per group.  Up to
// four rounds are in flight per trip (one per four lanes that start a long match in the same trip; the bench payload averages two);
// a trip with more finishes the earlier ones on the spot.
struct WaveCopy {                     // (kCoopRounds = 4 rounds in flight: d0..d3 / t0..t3)
    uint8_t *wave_base;
    uint32_t lane;
    u32x4 d0, d1, d2, d3;
    uint32_t t0, t1, t2, t3;          // destination (relative) of what d* holds, ~0 = nothing
    __device__ __forceinline__ bool any(bool b) const { return __builtin_amdgcn_ballot_w64(b) != 0; }
    __device__ __forceinline__ void stores() {
        if (t0 != 0xffffffffu) *(u32x4 *)(wave_base + t0) = d0;
        if (t1 != 0xffffffffu) *(u32x4 *)(wave_base + t1) = d1;
        if (t2 != 0xffffffffu) *(u32x4 *)(wave_base + t2) = d2;
        if (t3 != 0xffffffffu) *(u32x4 *)(wave_base + t3) = d3;
        t0 = t1 = t2 = t3 = 0xffffffffu;
    }
    __device__ __forceinline__ void begin(bool want, uint8_t *out, uint32_t o_body, uint32_t dist, uint32_t nb) {
        uint64_t mask = __builtin_amdgcn_ballot_w64(want);
        if (!mask) return;
        const uint32_t rel = (uint32_t)(out - wave_base) + o_body, packed = dist | nb << 16;
        const uint32_t g = lane >> 4, j = lane & 15u;
        for (;;) {
#define RGX_ROUND(D, Tg)                                                                                                         \
            if (mask) {                                                                                                          \
                const int l0 = __builtin_ctzll(mask); mask &= mask - 1;                                                          \
                const int l1 = mask ? __builtin_ctzll(mask) : -1; mask &= mask - 1;                                              \
                const int l2 = mask ? __builtin_ctzll(mask) : -1; mask &= mask - 1;                                              \
                const int l3 = mask ? __builtin_ctzll(mask) : -1; mask &= mask - 1;                                              \
                const int lg = g == 0 ? l0 : g == 1 ? l1 : g == 2 ? l2 : l3;                                                     \
                const uint32_t dd = (uint32_t)__builtin_amdgcn_ds_bpermute((lg < 0 ? 0 : lg) << 2, (int)rel);                    \
                const uint32_t pp = (uint32_t)__builtin_amdgcn_ds_bpermute((lg < 0 ? 0 : lg) << 2, (int)packed);                 \
                if (lg >= 0 && j < (pp >> 16)) { Tg = dd + 16u * j; D = ld128(wave_base + Tg - (pp & 0xffffu)); }                 \
            }
            RGX_ROUND(d0, t0) RGX_ROUND(d1, t1) RGX_ROUND(d2, t2) RGX_ROUND(d3, t3)
#undef RGX_ROUND
            if (!mask) break;
            __builtin_amdgcn_s_waitcnt(0x0F70);                   // more than four rounds in one trip: finish these now
            stores();
        }
    }
    __device__ __forceinline__ void end() { stores(); }
};

// Lane assignment: per group of kSortGroup consecutive members, their indices sorted by compressed length (bitonic sort in LDS, one
// workgroup per group).  A group spans at most kSortGroup x 64 KiB = 64 MiB of the arena: offsets relative to its first member fit 32 bits.
constexpr uint32_t kSortGroup = kInflateSortGroup;
__global__ __launch_bounds__(256) void k_member_sort(const Member *__restrict__ members, uint32_t n_members, uint32_t *perm) {
    __shared__ uint32_t key[kSortGroup];
    const uint32_t g0 = blockIdx.x * kSortGroup;
    for (uint32_t t = threadIdx.x; t < kSortGroup; t += 256) {
        const uint32_t i = g0 + t;
        key[t] = i < n_members ? (min(members[i].clen, 0x1fffffu) << 10 | t) : 0xffffffffu;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= kSortGroup; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < kSortGroup; t += 256) {
                const uint32_t x = t ^ j;
                if (x > t) {
                    const uint32_t a = key[t], b = key[x];
                    const bool up = (t & k) == 0;
                    if ((a > b) == up) { key[t] = b; key[x] = a; }
                }
            }
            __syncthreads();
        }
    for (uint32_t t = threadIdx.x; t < kSortGroup; t += 256) if (g0 + t < n_members) perm[g0 + t] = g0 + (key[t] & 1023u);
}

// What k_inflate_coop asks of a member list the PIPELINE did not make (rgx_k_inflate / rgx_k_inflate_form): its wave copies address the arena with
// 32-bit offsets from the first member of a group of kSortGroup, so upos must not decrease along the list and a group (plus one member's
// 64 KiB) must span less than 4 GiB.  A list that does not is refused: status[0] = the first offending member, status[1] = INF_OUT_OVERFLOW.
__global__ void k_members_check(const Member *__restrict__ members, uint32_t n_members, uint32_t *status, uint32_t *veto) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_members) return;
    const uint32_t first = (m / kSortGroup) * kSortGroup;
    const bool bad = (m > 0 && members[m].upos < members[m - 1].upos) || members[m].upos < members[first].upos ||
                     members[m].upos - members[first].upos > 0xfffe0000ull;
    if (bad) { *veto = 1; const uint32_t prev = atomicMin(&status[0], m); if (m < prev) status[1] = (uint32_t)INF_OUT_OVERFLOW; }
}

// early tail: this wave's bytes (and its members' verdicts) are out -- count it in its part of the launch (kernels.h InflateGate)
__device__ __forceinline__ void gate_wave_done(const InflateGate &gate, uint32_t lane) {
    if (!gate.done) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (lane == 0) {
        const uint32_t b = blockIdx.x;
        uint32_t part = 0;
#pragma unroll
        for (uint32_t k = 0; k + 1 < kGateParts; ++k) part += b >= gate.part_start[k] ? 1u : 0u;
        __hip_atomic_fetch_add(gate.done + part, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}
__global__ void k_wait_done(const uint32_t *done, uint32_t expected, uint32_t *timed_out) {
    uint32_t spins = 0;
    while (__hip_atomic_load(done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < expected) {
        if (++spins > 120000u) { *timed_out = 1; break; }
        for (int k = 0; k < 5; ++k) __builtin_amdgcn_s_sleep(127);
    }
}
void launch_wait_done(const uint32_t *done, uint32_t expected, uint32_t *timed_out, hipStream_t stream) {
    hipLaunchKernelGGL(k_wait_done, dim3(1), dim3(1), 0, stream, done, expected, timed_out);
}

// one lane per member like k_inflate; no lane leaves before the wave is done (the lanes without a member serve the others' copies)
template <bool PROBE, bool PIECE = false, int WIN = 0 /* bit reader: 0 = 8 bytes a refill, 1 = 16-byte window */>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_inflate_coop(const uint8_t *__restrict__ comp, const Member *__restrict__ members,
                                                uint32_t n_members, uint8_t *arena, uint64_t upos_bias, uint32_t *len_scratch,
                                                uint32_t *status, uint32_t ignore_below, uint32_t index_bias, uint8_t *bad, uint32_t pairs,
                                                const uint32_t *__restrict__ perm, const uint32_t *veto, InflateGate gate) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    // (stage entry point only: k_members_check found the list's layout unfit for 32-bit offsets -- nothing may be written)
    if (veto && *veto) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t slot = blockIdx.x * 64 + lane;
    const bool have = slot < n_members;
    // which member this lane decodes: the members of a group of kSortGroup come sorted by compressed length (k_member_sort), so that the 64
    // lanes of a wave need about the same number of trips (a wave runs as long as its longest lane: 93.5 -> 98.6 % of the lanes busy)
    const uint32_t m = have ? (perm ? perm[slot] : slot) : n_members - 1;
    const Member mb = members[m];
    if (PIECE && gate.flags) {
        // the upload chunk with the last byte any lane of this wave reads (payload + footer + the bit reader's look-ahead); one lane polls,
        // seldom (every waiting wave's poll is a request to the fabric the running waves share), an acquire then drops what this CU's L1 may
        // hold.  A chunk that never comes (the host gave up): after ~2 s the wave's members are reported as not inflated.
        uint32_t need = gate_chunk_needed(mb.cpos, mb.clen, gate.lo, gate.chunk_bytes, gate.n_chunks);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) need = max(need, (uint32_t)__shfl_xor((int)need, d, 64));
        bool arrived = true;
        if (lane == 0) {
            uint32_t spins = 0;
            while (__hip_atomic_load(gate.flags + need, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != gate.epoch) {
                if (++spins > 100000u) { arrived = false; break; }
                for (int k = 0; k < 5; ++k) __builtin_amdgcn_s_sleep(127);
            }
        }
        arrived = __builtin_amdgcn_ballot_w64(!arrived) == 0;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        // (the members of the last chunks are what the call waits for -- their own chain behind the last arrival: their waves issue ahead of the
        //  waves of earlier chunks that share their SIMD)
        if (!arrived) {
            if (have) report_bad_member(m, index_bias, ignore_below, status, bad, INF_IN_OVERRUN);
            gate_wave_done(gate, lane);
            return;
        }
    }
    LdsTab T{lds + lane, len_scratch + (have ? slot : 0), gridDim.x * 64};
    // the lowest output address the wave's lanes can have: the first member of the wave's group (upos grows with the member index; PROBE: slot m)
    const uint32_t first = perm ? (blockIdx.x * 64 / kSortGroup) * kSortGroup : blockIdx.x * 64;
    const uint64_t base_off = PROBE ? (uint64_t)first * kBgzfMaxBlock : members[first].upos - upos_bias;
    WaveCopy C;
    C.wave_base = arena + base_off; C.lane = lane;
    C.d0 = C.d1 = C.d2 = C.d3 = u32x4{0, 0, 0, 0};
    C.t0 = C.t1 = C.t2 = C.t3 = 0xffffffffu;
    uint32_t out_len = 0;
    if (PROBE) {
        const bool run = have && mb.isize != 0xffffffffu;         // ~0: BSIZE runs past the end of the file (or is < 26): the read fails upstream
        const int st = inflate_coop<BitReader>(comp + mb.cpos, mb.clen, arena + (uint64_t)(have ? m : first) * kBgzfMaxBlock, kBgzfMaxBlock, &out_len, T, C, run, pairs);
        if (have) status[m] = run && st == INF_OK ? out_len : 0xffffffffu;
        return;
    }
    const bool run = have && mb.isize <= kBgzfMaxBlock;           // (member_verdict: the others own no bytes of the arena)
    typedef typename std::conditional<WIN == 1, BitReaderWin, BitReader>::type BR;
    int st = inflate_coop<BR>(comp + mb.cpos, mb.clen, run ? arena + (mb.upos - upos_bias) : C.wave_base, run ? mb.isize : 0, &out_len, T, C, run, pairs);
    if (have) {
        st = member_verdict(mb, run, st, out_len);
        if (st != INF_OK) report_bad_member(m, index_bias, ignore_below, status, bad, st);
    }
    if (PIECE) gate_wave_done(gate, lane);
}

// (the code-length / cold-symbol scratch of every lane, + the lane assignment of k_inflate_coop behind it)
static size_t inflate_scratch_words(uint32_t n_members) { return (size_t)((n_members + 63) / 64) * 64 * kScratchWordsPerLane; }
size_t inflate_scratch_bytes(uint32_t n_members) { return (inflate_scratch_words(n_members) + ((size_t)n_members + 63) / 64 * 64 + kSortGroup) * 4; }

// ---- the small-input form: one member per wave, the whole member in LDS (inflate_wave.h) ------------------------------------------------
struct DevWave {
    uint32_t lane;
    template <class F> __device__ __forceinline__ void lanes(F f) const { f(lane); }
    __device__ __forceinline__ void sync() const {                       // one wave per workgroup: orders the lanes' LDS traffic (and the compiler)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
};
static_assert(sizeof(WaveShared) <= 80 * 1024, "two wave-per-member workgroups per CU");

__global__ __launch_bounds__(64) void k_inflate_wave(const uint8_t *__restrict__ comp, const Member *__restrict__ members, uint32_t n_members, uint8_t *arena,
                                                     uint64_t upos_bias, uint32_t *status, uint32_t ignore_below, uint32_t index_bias, uint8_t *bad) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    WaveShared &S = *reinterpret_cast<WaveShared *>(lds);
    const uint32_t m = blockIdx.x;
    if (m >= n_members) return;
    const Member mb = members[m];
    DevWave W{threadIdx.x};
    int st;
    uint32_t out_len = 0;
    if (mb.isize > kBgzfMaxBlock) st = member_verdict(mb, false, INF_OK, 0);           // (= !run of the other kernels: owns no bytes of the arena, the decoder does not run)
    else {
        st = inflate_wave(W, S, comp + mb.cpos, mb.clen, arena + (mb.upos - upos_bias), mb.isize, &out_len);
        st = member_verdict(mb, true, st, out_len);
    }
    if (st != INF_OK && threadIdx.x == 0) report_bad_member(m, index_bias, ignore_below, status, bad, st);
}

// Four forms of the decoder (rgx_k_inflate_form / REGTOOLS_AMD_INFLATE = lane | wave | ring | coop):
//   1 lane  k_inflate       (round 1: one member per lane, every lane copies its own matches, 12 waves per CU)
//   2 wave  k_inflate_wave  (round 2: one member per WAVE, member in LDS: small inputs -- 1.17 ms per 512 members against the lane forms'
//                            7.7-9.7 ms per launch whatever its size; wins up to ~4,000 members, tools/inflate_forms.py)
//   3 ring  k_inflate_ring  (round 2: lane form with a per-lane LDS window; 0.5x the HBM traffic, 4 waves per CU, 1.9x slower: DESIGN.md 5.1)
//   4 coop  k_inflate_coop  (round 3: lane form, long matches moved by the wave in aligned 256-byte pieces: inflate_coop.h)
// The pipeline (form 0) takes the wave form up to kWaveFormMaxMembers members and kDefaultLaneForm beyond.
constexpr uint32_t kWaveFormMaxMembers = 2048;
constexpr int kDefaultLaneForm = 4;
constexpr int kDefaultWindow = 1;     // k_inflate_coop's bit reader (its WIN parameter)
static int inflate_form_env() {
    static const int f = [] {
        const char *e = getenv("REGTOOLS_AMD_INFLATE");
        return !e ? 0 : !strcmp(e, "lane") ? 1 : !strcmp(e, "wave") ? 2 : !strcmp(e, "ring") ? 3 : !strcmp(e, "coop") ? 4 : 0;
    }();
    return f;
}
// (the attribute belongs to the current device's copy of the function: once per device, and the shard threads of rgx_extract_multi
// may get here together)
// A configuration step that failed (hipFuncSetAttribute on this device's copy of a kernel) must not pass silently: the launch behind it
// would fail or run with too little LDS, the arena would stay untouched and the stages behind it would read it.  The error is kept per host
// thread until the caller's next checked HIP call (api_internal.h HIP_TRY -> pending_launch_error) turns it into RGX_ERR_DEVICE.
static thread_local hipError_t tl_launch_error = hipSuccess;
hipError_t pending_launch_error() {
    hipError_t e = tl_launch_error; tl_launch_error = hipSuccess;
    const hipError_t last = hipGetLastError();                    // (a launch whose configuration was refused: sticky until read)
    return e != hipSuccess ? e : last;
}
static void inflate_attrs() {
    static std::mutex mu;
    static bool done_dev[64] = {};
    static hipError_t err_dev[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    std::lock_guard<std::mutex> lk(mu);
    bool &done = done_dev[dev];
    if (done) { if (err_dev[dev] != hipSuccess) tl_launch_error = err_dev[dev]; return; }
    hipError_t first = hipSuccess;
    auto set = [&](const void *fn, uint32_t bytes) { const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes); if (e != hipSuccess && first == hipSuccess) first = e; };
    set((const void *)k_inflate<false, false>, kInflateLdsBytes);
    set((const void *)k_inflate<false, true>, kInflateLdsBytes);
    set((const void *)k_inflate<true>, kInflateLdsBytes);
    set((const void *)k_inflate_coop<false, false, 0>, kInflateLdsBytes);
    set((const void *)k_inflate<false, false, 4>, kInflateLdsBytes);
    set((const void *)k_inflate<false, true, 4>, kInflateLdsBytes);
    set((const void *)k_inflate_coop<false, true, 0>, kInflateLdsBytes);
    set((const void *)k_inflate_coop<false, false, 1>, kInflateLdsBytes);
    set((const void *)k_inflate_coop<false, true, 1>, kInflateLdsBytes);
    set((const void *)k_inflate_coop<true>, kInflateLdsBytes);
    set((const void *)k_inflate_wave, (uint32_t)sizeof(WaveShared));
    set((const void *)k_inflate_ring<false>, kRingLdsBytes);
    set((const void *)k_inflate_ring<true>, kRingLdsBytes);
    err_dev[dev] = first; done = true;
    if (first != hipSuccess) tl_launch_error = first;
}
// The gate's flag word, written ON THE DEVICE (a one-lane kernel queued on the copy stream behind the chunk's copy): a word the copy engine
// wrote was seen by the polling waves only hundreds of microseconds later (their system-scope loads are served by an L2 that the engine's
// write does not reach; measured: 604 ms per step); a store from a wave is coherent with them.
__global__ void k_gate_set(uint32_t *flag, uint32_t epoch) { __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
void launch_gate_set(uint32_t *flag, uint32_t epoch, hipStream_t stream) { hipLaunchKernelGGL(k_gate_set, dim3(1), dim3(1), 0, stream, flag, epoch); }
// The host scan's member list, from page-locked host memory into HBM: 16 bytes a lane, every byte over the link once.  (Both blocks are a member
// longer than the list: the last lane's 16 bytes may end 8 behind it.)
__global__ __launch_bounds__(256) void k_members_fetch(const uint4 *__restrict__ src, uint4 *__restrict__ dst, uint32_t n16) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n16; i += gridDim.x * 256) dst[i] = src[i];
}
void launch_members_fetch(const Member *host_members, Member *dst, uint32_t n_members, hipStream_t stream) {
    static_assert(sizeof(Member) == 24, "two members are three 16-byte words");
    const uint32_t n16 = (uint32_t)(((uint64_t)n_members * sizeof(Member) + 15) / 16);
    if (!n16) return;
    hipLaunchKernelGGL(k_members_fetch, dim3(std::min<uint32_t>((n16 + 255) / 256, 256)), dim3(256), 0, stream, (const uint4 *)host_members, (uint4 *)dst, n16);
}
bool inflate_takes_coop(uint32_t n_members) {
    const int f = inflate_form_env();
    return f ? f == 4 : n_members > kWaveFormMaxMembers && kDefaultLaneForm == 4;
}
void launch_inflate(const uint8_t *comp, const Member *members, uint32_t n_members, uint8_t *arena, uint64_t upos_bias, uint32_t *len_scratch,
                    uint32_t *status, hipStream_t stream, uint32_t ignore_below, uint32_t index_bias, bool piece, int form, uint8_t *bad, int plan, bool check_layout, InflateGate gate) {
    if (!n_members) return;
    inflate_attrs();
    // k_inflate_coop's mode word (inflate_coop.h): bit 0 = a literal and the symbol behind it per trip, bits 0 + 1 = exact bit counts and a
    // match behind a literal pair in the same trip, bit 2 = runs (distance <= 16) written from registers, 64 bytes a trip (round 4).
    // Same box, interleaved, ms (tools/lab/runs_ab.sh, profiles/r04_inflate_modes.txt): bench payload mode 1 15.2-15.3 / 3 14.2-15.1 / 7 14.1-15.0;
    // random bases + qualities 1: 48.2-48.4 / 3: 45.4-47.4; long reads 0: 121.2 / 1: 123.9-124.7 / 4: 79.8-79.9 / 5: 80.4-80.6 / 7: 80.5-80.9.
    const uint32_t two = (plan & 1) ? 7u : 4u;
    if (!form) form = inflate_form_env();
    if (!form) form = n_members <= kWaveFormMaxMembers ? 2 : (plan & 2) ? 1 : kDefaultLaneForm;
    const uint32_t blocks = (n_members + 63) / 64;
    switch (form) {
    case 2:
        hipLaunchKernelGGL(k_inflate_wave, dim3(n_members), dim3(64), (uint32_t)sizeof(WaveShared), stream, comp, members, n_members, arena, upos_bias, status, ignore_below, index_bias, bad);
        break;
    case 3:
        hipLaunchKernelGGL(k_inflate_ring<false>, dim3(blocks), dim3(64), kRingLdsBytes, stream, comp, members, n_members, arena, upos_bias, len_scratch, status, ignore_below, index_bias, bad);
        break;
    case 4: {
        // plan bit 0 set (payloads that compress up to 32 x): literal pairs and lanes sorted by compressed length; the windowed bit reader always
        // (round 4: its loads are no longer waited for on the spot -- long reads 117.5 ms with it against 120.7 without, kernels.h)
        const bool sort = (plan & 1) != 0;
        const int win = kDefaultWindow;
        uint32_t *perm = sort ? len_scratch + inflate_scratch_words(n_members) : nullptr;
        if (perm) hipLaunchKernelGGL(k_member_sort, dim3((n_members + kSortGroup - 1) / kSortGroup), dim3(256), 0, stream, members, n_members, perm);
        // (the veto word: behind the lane assignment in the scratch; only the stage entry point asks for the check)
        uint32_t *veto = check_layout ? len_scratch + inflate_scratch_words(n_members) + ((size_t)n_members + 63) / 64 * 64 + kSortGroup - 1 : nullptr;
        if (check_layout) {
            (void)hipMemsetAsync(veto, 0, 4, stream);
            hipLaunchKernelGGL(k_members_check, dim3((n_members + 255) / 256), dim3(256), 0, stream, members, n_members, status, veto);
        }
#define RGX_COOP(PIECE_, WIN_) hipLaunchKernelGGL((k_inflate_coop<false, PIECE_, WIN_>), dim3(blocks), dim3(64), kInflateLdsBytes, stream, comp, members, n_members, arena, upos_bias, len_scratch, status, ignore_below, index_bias, bad, two, perm, veto, gate)
        if (piece) { if (win) RGX_COOP(true, 1); else RGX_COOP(true, 0); }
        else { if (win) RGX_COOP(false, 1); else RGX_COOP(false, 0); }
#undef RGX_COOP
        break;
    }
    default: {
        // plan bit 1 = a payload of mostly literals (< 8 x): up to four of them per trip
        const bool lits4 = form == 5 || (plan & 2) != 0;          // (form 5: the stage entry point's way to ask for it)
#define RGX_LANE(PIECE_, LITS_) hipLaunchKernelGGL((k_inflate<false, PIECE_, LITS_>), dim3(blocks), dim3(64), kInflateLdsBytes, stream, comp, members, n_members, arena, upos_bias, len_scratch, status, ignore_below, index_bias, bad)
        if (piece) { if (lits4) RGX_LANE(true, 4); else RGX_LANE(true, 1); }
        else { if (lits4) RGX_LANE(false, 4); else RGX_LANE(false, 1); }
#undef RGX_LANE
    }
    }
}
void launch_inflate_probe(const uint8_t *comp, const Member *members, uint32_t n_members, uint8_t *slots, uint32_t *len_scratch, uint32_t *sizes,
                          hipStream_t stream) {
    if (!n_members) return;
    inflate_attrs();
    const int form = inflate_form_env() ? inflate_form_env() : kDefaultLaneForm;
    const uint32_t blocks = (n_members + 63) / 64;
    if (form == 3) hipLaunchKernelGGL(k_inflate_ring<true>, dim3(blocks), dim3(64), kRingLdsBytes, stream, comp, members, n_members, slots, (uint64_t)0, len_scratch, sizes, 0u, 0u, (uint8_t *)nullptr);
    else if (form == 4) hipLaunchKernelGGL(k_inflate_coop<true>, dim3(blocks), dim3(64), kInflateLdsBytes, stream, comp, members, n_members, slots, (uint64_t)0, len_scratch, sizes, 0u, 0u, (uint8_t *)nullptr, 1u, (const uint32_t *)nullptr, (const uint32_t *)nullptr, InflateGate());
    else hipLaunchKernelGGL(k_inflate<true>, dim3(blocks), dim3(64), kInflateLdsBytes, stream, comp, members, n_members, slots, (uint64_t)0, len_scratch, sizes, 0u, 0u, (uint8_t *)nullptr);
}

}  // namespace rgx
