// records_kernels.hip -- from the inflated arena to the read table: record framing and the decode to SoA rows (SURVEY.md 8a rows a2, a3, a5,
// a6).  Called by api_records.cpp and api_internal.h; what a record means is bam_core.h's (rec_head, rec_sane, record_row), which the host
// twins run too.
//   k_seg_walk         one lane per arena segment: guess the first record start in the segment, walk the block_size chain out of it
//   k_seg_verify       one sweep that makes the guesses agree with their left neighbours' exits (the host loops until nothing changes)
//   k_seg_truncate     the chain ended inside a segment: nothing starts to its right
//   k_decode_seg       <STAGED> one wave per segment, the segment's bytes staged through LDS (or, STAGED = false, read in place): SoA rows,
//                      per-read event counts, per-segment totals
//   k_decode_sparse    long records: one lane per segment, every read from the arena
//   k_long_fill        the list of the reads that go to k_emit_long, one wave per segment, no atomics
//   k_collect_odd_aux  identify -s XS: the reads whose strand tag lies behind an aux field of unknown type
// Constants owned here: kSegTail, kSegMaxRecs (the staged window); the segment sizes and the chain marks are kernels.h's.  decode_knobs
// (REGTOOLS_AMD_DECODE) lives here too.  Integer and byte work bounded by HBM traffic; no MFMA.
#include "wave_prims.h"

#include <cstdlib>
#include <cstring>

namespace rgx {

// =====================================================================================================
// a2. record framing: speculative per-segment chains, verified exactly
// =====================================================================================================
// Walk the block_size chain from `o` until it leaves [.., seg_end). Returns the first record start >= seg_end
// (or kChainEnd when the chain hits an unreadable record / the end of the stream) and counts the records started.
// cp (optional): cp[j] = offset of record 8j from seg_begin -- k_decode_seg's lanes re-walk eight records each from there instead of
// one lane re-walking all of them.
__device__ __forceinline__ uint64_t walk_chain(const uint8_t *arena, uint64_t o, uint64_t seg_end, uint64_t lim, uint32_t &cnt, uint16_t *cp = nullptr,
                                               uint64_t seg_begin = 0, bool lite = false) {
    cnt = 0;
    while (o < seg_end) {
        if (o + 36 > lim) return kChainEnd;             // bam_read1: short read of the fixed part
        RecHead h;
        if (lite) {                                     // block_size alone: ONE request per record (the rest of the test: the decode pass, SegGeom::lite_walk)
            h.block_len = (int32_t)ld32(arena + o);
            if (h.block_len < 32) return kChainEnd;
        } else {
            rec_head(arena + o, h);
            if (!rec_sane(h)) return kChainEnd;         // sam.c:421-423 -> iteration ends
        }
        uint64_t nxt = o + 4 + (uint64_t)(uint32_t)h.block_len;
        if (nxt > lim) return kChainEnd;                // truncated record body
        if (cp && (cnt & 7u) == 0) cp[cnt >> 3] = (uint16_t)(o - seg_begin);
        ++cnt;
        o = nxt;
    }
    return o;
}

// the bytes segment s covers: [a, b), where its chain's readable bytes end (lim), and whether s is the first segment of its chain
__device__ __forceinline__ void seg_of(const SegGeom &g, uint32_t s, uint64_t &a, uint64_t &b, uint64_t &lim, bool &first) {
    if (!g.chunks) {
        a = g.pos0 + (uint64_t)s * g.seg_bytes; b = a + g.seg_bytes; lim = g.lim; first = s == 0;
        if (b > lim) b = lim;
        return;
    }
    uint32_t lo = 0, hi = g.n_chunks;                    // the last chunk whose seg_base is <= s (few chunks, the table stays in the caches)
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (g.chunks[mid].seg_base <= s) lo = mid; else hi = mid; }
    const SegChunk c = g.chunks[lo];
    a = c.a + (uint64_t)(s - c.seg_base) * g.seg_bytes; b = a + g.seg_bytes; lim = c.dlim; first = s == c.seg_base;
    if (b > c.b) b = c.b;
}

__global__ void k_seg_walk(const uint8_t *__restrict__ arena, SegGeom g, uint32_t n_seg, int32_t n_ref,
                           uint64_t *seg_start, uint64_t *seg_exit, uint32_t *seg_cnt, uint16_t *seg_cp, uint32_t s_begin) {
    uint32_t s = s_begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    uint16_t *cp = g.seg_bytes == kSegBytes ? seg_cp + (size_t)s * kSegCpSlots : nullptr;     // (checkpoints: 16-bit offsets, 16 KiB segments only)
    uint64_t a, b, lim; bool first;
    seg_of(g, s, a, b, lim, first);
    uint64_t o = a, ex = kChainEnd;
    uint32_t cnt = 0;
    if (!first) {
        // guess: first offset in the segment where three chained records all look like records AND the block_size chain from
        // there leaves the segment through readable records.  A false start almost never survives that (a 16 KiB walk is dozens
        // of records), so wrong exits -- the expensive kind of misprediction, see k_seg_verify -- are rare.
        // (the search loop and the walk are kept apart so that the lanes of a wave walk their segments together)
        o = kChainEnd;
        uint64_t c = a;
        for (;;) {
            // Coarse filter first, 16 candidate offsets per 20-byte load: the word at a record start is a block_size, i.e. in
            // [32, 2^27] (rec_sane / rec_plausible).  Sequence and quality bytes (long reads: kilobytes of them before the next
            // record) fail it without another memory access; only survivors get the full test below.
            uint64_t cand = kChainEnd;
            while (c < b) {
                const u32x4 v = ld128(arena + c);
                const uint32_t w[5] = {v[0], v[1], v[2], v[3], ld32(arena + c + 16)};
                uint32_t mask = 0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const uint32_t bl = (i & 3) ? __builtin_amdgcn_alignbyte(w[(i >> 2) + 1], w[i >> 2], (uint32_t)(i & 3)) : w[i >> 2];
                    mask |= (bl - 32u <= (1u << 27) - 32u ? 1u : 0u) << i;
                }
                const uint64_t room = b - c;
                if (room < 16) mask &= (1u << (uint32_t)room) - 1u;
                bool found = false;
                while (mask) {
                    const uint32_t i = (uint32_t)__builtin_ctz(mask);
                    mask &= mask - 1;
                    const uint64_t q = c + i;
                    if (!rec_plausible(arena, q, lim, n_ref)) continue;
                    const uint64_t c2 = q + 4 + (uint64_t)ld32(arena + q);
                    if (c2 < lim) {
                        if (!rec_plausible(arena, c2, lim, n_ref)) continue;
                        const uint64_t c3 = c2 + 4 + (uint64_t)ld32(arena + c2);
                        if (c3 < lim && !rec_plausible(arena, c3, lim, n_ref)) continue;
                    }
                    cand = q; found = true; break;
                }
                if (found) break;
                c += 16;
            }
            if (cand == kChainEnd) break;
            ex = walk_chain(arena, cand, b, lim, cnt, cp, a, g.lite_walk != 0);
            if (ex != kChainEnd) { o = cand; break; }
            c = cand + 1;
        }
        if (o == kChainEnd) { ex = kChainUnknown; o = b; cnt = 0; }  // nothing usable: a placeholder that claims nothing (see k_seg_verify)
    } else ex = walk_chain(arena, o, b, lim, cnt, cp, a, g.lite_walk != 0);
    seg_start[s] = o; seg_exit[s] = ex; seg_cnt[s] = cnt;
}

// is segment s (> 0) framed the way its left neighbour's exit says it must be?
__device__ __forceinline__ bool seg_consistent(uint64_t b /* the segment's end */, uint64_t expect, uint64_t st, uint64_t ex, uint32_t cnt) {
    return expect >= b ? (st == b && ex == expect && cnt == 0) : st == expect;   // expect >= b (incl. kChainEnd): no record starts here
}

// One sweep.  Segment states: a GUESS (start/exit from a walk that left the segment through readable records), or a PLACEHOLDER
// (the search found nothing; exit = kChainUnknown: typical for the segments inside a record that is longer than a segment).
//  * a placeholder adopts its left neighbour's exit as soon as that exit is a real value -- it has no opinion to defend, and runs of
//    placeholders (long reads) resolve left to right, all runs of the file in parallel;
//  * a guess that disagrees with its left neighbour's exit is re-walked from that exit only once the neighbour itself agrees with
//    ITS neighbour: a wrong exit (a guess that landed on a false chain which never re-joins the true one) is then repaired where it
//    happened instead of being copied one segment to the right per sweep with the repair trailing it to the end of the file.
// Sweeps needed = longest run of consecutive placeholders / disagreeing guesses (+1 to see "no change").  status[0] = leftmost segment
// that is not final yet, so the loop ends only when the whole chain agrees -- which, segment 0 being exact, means it is exact.
// status[1] = leftmost segment whose chain ends (kChainEnd): when that one lies in the exact prefix the stream really ends there
// (truncated / unreadable record, sam.c:421-423) and the host empties everything to its right in one launch.
__global__ void k_seg_verify(const uint8_t *__restrict__ arena, SegGeom g, uint32_t n_seg,
                             const uint64_t *__restrict__ st_in, const uint64_t *__restrict__ ex_in, const uint32_t *__restrict__ cnt_in,
                             uint64_t *st_out, uint64_t *ex_out, uint32_t *cnt_out, uint32_t *status, uint16_t *seg_cp) {
    uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    uint64_t st = st_in[s], ex = ex_in[s];
    uint32_t cnt = cnt_in[s];
    uint64_t a, b, lim; bool first;
    seg_of(g, s, a, b, lim, first);
    if (ex == kChainEnd && (first || ex_in[s - 1] != kChainEnd)) atomicMin(status + 1, s);
    if (!first) {                                                               // (a chain's first segment starts at an exact offset)
        const uint64_t expect = ex_in[s - 1];
        if (expect == kChainUnknown) atomicMin(status, s);                      // the left neighbour knows nothing yet: wait
        else if (!seg_consistent(b, expect, st, ex, cnt)) {
            atomicMin(status, s);
            const bool placeholder = ex == kChainUnknown;
            uint64_t a1, b1, lim1; bool first1;
            seg_of(g, s - 1, a1, b1, lim1, first1);
            const bool left_settled = first1 || (ex_in[s - 2] != kChainUnknown && seg_consistent(b1, ex_in[s - 2], st_in[s - 1], expect, cnt_in[s - 1]));
            if (placeholder || left_settled) {
                if (expect >= b) { st = b; ex = expect; cnt = 0; }
                else { st = expect; ex = walk_chain(arena, st, b, lim, cnt, g.seg_bytes == kSegBytes ? seg_cp + (size_t)s * kSegCpSlots : nullptr, a, g.lite_walk != 0); }
            }
        }
    }
    st_out[s] = st; ex_out[s] = ex; cnt_out[s] = cnt;
}

// the record chain ended inside segment `last`: no record starts to its right
__global__ void k_seg_truncate(SegGeom g, uint32_t n_seg, uint32_t last, uint64_t *st, uint64_t *ex, uint32_t *cnt) {
    uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg || s <= last) return;
    uint64_t a, b, lim; bool first;
    seg_of(g, s, a, b, lim, first);
    st[s] = b; ex[s] = kChainEnd; cnt[s] = 0;
}

void launch_seg_walk(const uint8_t *arena, SegGeom g, uint32_t n_seg, int32_t n_ref, uint64_t *seg_start,
                     uint64_t *seg_exit, uint32_t *seg_cnt, uint16_t *seg_cp, hipStream_t stream, uint32_t s_begin) {
    if (n_seg <= s_begin) return;
    hipLaunchKernelGGL(k_seg_walk, dim3((n_seg - s_begin + 63) / 64), dim3(64), 0, stream, arena, g, n_seg, n_ref, seg_start, seg_exit, seg_cnt, seg_cp, s_begin);
}
void launch_seg_verify(const uint8_t *arena, SegGeom g, uint32_t n_seg, const uint64_t *seg_start_in,
                       const uint64_t *seg_exit_in, const uint32_t *seg_cnt_in, uint64_t *seg_start_out, uint64_t *seg_exit_out,
                       uint32_t *seg_cnt_out, uint32_t *status, uint16_t *seg_cp, hipStream_t stream) {
    if (!n_seg) return;
    hipLaunchKernelGGL(k_seg_verify, dim3((n_seg + 63) / 64), dim3(64), 0, stream, arena, g, n_seg, seg_start_in, seg_exit_in,
                       seg_cnt_in, seg_start_out, seg_exit_out, seg_cnt_out, status, seg_cp);
}
void launch_seg_truncate(SegGeom g, uint32_t n_seg, uint32_t last, uint64_t *seg_start, uint64_t *seg_exit, uint32_t *seg_cnt, hipStream_t stream) {
    if (!n_seg) return;
    hipLaunchKernelGGL(k_seg_truncate, dim3((n_seg + 255) / 256), dim3(256), 0, stream, g, n_seg, last, seg_start, seg_exit, seg_cnt);
}

// =====================================================================================================
// a2/a3/a5/a6. decode to SoA (one lane per record) + per-read junction-event count
// =====================================================================================================
// ONE WAVE PER SEGMENT.  The segment's bytes are loaded once, coalesced (16 B per lane per
// instruction), into LDS; lane 0 re-walks the (already verified) record chain there at LDS latency and leaves the
// record offsets in LDS; then the 64 lanes decode the records in parallel from LDS and write the SoA rows coalesced.
// Scattered 4-byte global reads of the record heads (one 64 B HBM sector per field group) become a streaming read.
constexpr uint32_t kSegTail = 1024;                      // bytes past the segment end kept in LDS (record bodies)
constexpr uint32_t kSegMaxRecs = kSegBytes / 36 + 2;     // a record is at least 36 bytes

// What a decode kernel's lane gathers over its records; the kernel says how it walks its segment and where a record's bytes are read from
// (cigar_at, tag_strand: LDS window or arena), what the record means is bam_core.h's record_row.
struct DecodeTally { uint32_t n_iter = 0, n_long = 0, first_stop = 0xffffffffu, last_in = 0; };
// Row i of the read table from the record at arena offset o, and everything the rule's answers cause.
template <class CigarAt, class TagStrand>
__device__ __forceinline__ void decode_record(RecHead &h, uint32_t i, uint64_t o, const ExtractCfg &cfg, const ReadSoA &soa, DecodeTally &t,
                                              CigarAt &&cigar_at, TagStrand &&tag_strand) {
    // (the framing only looked at block_size: the call starts over with the full walk.  Until then the record is inert: its CIGAR count and its
    //  aux offset are not to be believed -- a negative l_seq puts the aux walk in front of the arena, 65,535 operations run past its end)
    if (cfg.insane_out && !rec_sane(h)) { cfg.insane_out[0] = 1; h.n_cigar = 0; }
    soa.tid[i] = h.tid; soa.pos[i] = h.pos;
    soa.flag_nc[i] = h.flag << 16 | h.n_cigar;
    soa.cig_off[i] = o + 36 + h.l_qname;
    if (soa.rec_off) soa.rec_off[i] = o;
    const RecordRow r = record_row(h, i, cfg, cigar_at, tag_strand);
    if (r.stop_candidate) t.first_stop = min(t.first_stop, i);
    if (r.in_region) { ++t.n_iter; t.last_in = i + 1; }
    t.n_long += r.is_long ? 1u : 0u;
    if (r.abort_read) atomicMin(cfg.abort_out, i);
    if (r.odd_read) atomicAdd(cfg.odd_count, 1u);
    soa.strand[i] = r.strand;
    soa.n_ev[i] = r.nev;
}
// the wave's candidates of the end rule into ExtractCfg::stop_out
__device__ __forceinline__ void stop_reduce(uint32_t *stop_out, uint32_t first_stop, uint32_t last_in) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { first_stop = min(first_stop, (uint32_t)__shfl_xor((int)first_stop, d, 64)); last_in = max(last_in, (uint32_t)__shfl_xor((int)last_in, d, 64)); }
    // (segments are launched roughly in order: after the first few, the values in memory already beat most candidates)
    if (threadIdx.x == 0) {
        if (first_stop < *(volatile uint32_t *)&stop_out[0]) atomicMin(&stop_out[0], first_stop);
        if (last_in > *(volatile uint32_t *)&stop_out[1]) atomicMax(&stop_out[1], last_in);
    }
}
// STAGED = false is the form for long records (kilobytes of sequence and quality per record, two or three records per segment):
// nothing is staged, heads / CIGAR / aux are read where they lie, and the 95 % of the stream that is sequence and quality never
// leaves HBM.  The host picks it when the mean record is longer than kSparseRecordBytes.
template <bool STAGED>
__global__ __launch_bounds__(64) void k_decode_seg(const uint8_t *__restrict__ arena, SegGeom g, uint32_t n_seg,
                                                   const uint64_t *__restrict__ seg_start, const uint32_t *__restrict__ seg_base,
                                                   const uint32_t *__restrict__ seg_cnt, ExtractCfg cfg, ReadSoA soa, uint32_t *seg_iter,
                                                   uint32_t *seg_long, const uint16_t *__restrict__ seg_cp, uint32_t s_begin) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_buf[];          // kSegBytes + kSegTail + 48 when STAGED, nothing otherwise
    __shared__ uint32_t s_off[kSegMaxRecs];
    const uint32_t s = s_begin + blockIdx.x, lane = threadIdx.x;
    const uint32_t cnt = seg_cnt[s];
    if (cnt == 0) { if (lane == 0) { seg_iter[s] = 0; seg_long[s] = 0; } return; }
    uint64_t a, seg_b, seg_lim; bool seg_first;
    seg_of(g, s, a, seg_b, seg_lim, seg_first);
    // window [w0, w1): 16-byte aligned start at/below the segment begin, end = segment end + tail, clipped to the arena
    const uint64_t w0 = a & ~15ull;
    uint64_t w1 = a + kSegBytes + kSegTail;
    if (w1 > g.data_end) w1 = g.data_end;
    if constexpr (STAGED) {
        // all loads of the window in flight at once (18 x 1 KiB per wave), then the LDS stores: one HBM latency, not eighteen
        constexpr int kChunks = (kSegBytes + kSegTail + 16 + 1023) / 1024;
        u32x4 r[kChunks];
#pragma unroll
        for (int j = 0; j < kChunks; ++j) {
            const uint64_t o = w0 + (uint64_t)j * 1024 + (uint64_t)lane * 16;
            if (o < w1) r[j] = ld128(arena + o);               // reads < 16 B past lim: the arena is padded
        }
#pragma unroll
        for (int j = 0; j < kChunks; ++j) {
            const uint64_t o = w0 + (uint64_t)j * 1024 + (uint64_t)lane * 16;
            if (o < w1) *(u32x4 *)(s_buf + (o - w0)) = r[j];
        }
    }
    __syncthreads();
    // unaligned 32-bit read from the LDS window: two aligned dword reads + a byte funnel shift (v_alignbyte_b32)
    const uint32_t *s_w = (const uint32_t *)s_buf;
    auto lds32 = [&](uint32_t off) -> uint32_t {
        if constexpr (STAGED) return __builtin_amdgcn_alignbyte(s_w[(off >> 2) + 1], s_w[off >> 2], off & 3u);
        else return ld32(arena + w0 + off);
    };
    // chain walk inside LDS: lane j re-walks records 8j .. 8j+7 from the checkpoint the framing left (a segment holds at most
    // kSegMaxRecs = 457 records = 58 checkpoints)
    if (lane * 8 < cnt) {
        uint64_t o = a + seg_cp[(size_t)s * kSegCpSlots + lane];
        const uint32_t k_end = min(cnt, lane * 8 + 8);
        for (uint32_t k = lane * 8; k < k_end; ++k) {
            const uint32_t ro = (uint32_t)(o - w0);
            s_off[k] = ro;
            o += 4 + (uint64_t)((STAGED && o + 4 <= w1) ? lds32(ro) : ld32(arena + o));
        }
    }
    __syncthreads();
    const uint32_t base = seg_base[s];
    DecodeTally t;
    for (uint32_t k = lane; k < cnt; k += 64) {
        const uint32_t ro = s_off[k];
        const uint64_t o = w0 + ro;
        // the 36-byte record head always lies inside the window (tail >= 36); CIGAR / aux of the spliced minority are read from the arena
        RecHead h;
        {
            const uint32_t sh = ro & 3u, wi = ro >> 2;
            uint32_t x[8];
            if constexpr (STAGED) {
                uint32_t d[9];
#pragma unroll
                for (int q = 0; q < 9; ++q) d[q] = s_w[wi + q];
#pragma unroll
                for (int q = 0; q < 8; ++q) x[q] = __builtin_amdgcn_alignbyte(d[q + 1], d[q], sh);
            } else {
                (void)sh; (void)wi;
#pragma unroll
                for (int q = 0; q < 8; ++q) x[q] = ld32(arena + o + 4 * q);
            }
            rec_head_words(x, h);
        }
        // body (CIGAR, aux) from the LDS window when the whole record is inside it, else straight from the arena
        const uint64_t rec_end = o + 4 + (uint64_t)(uint32_t)h.block_len;
        const bool in_win = STAGED && rec_end <= w1;
        const uint32_t cig_ro = ro + 36 + h.l_qname;
        const uint8_t *g_data = arena + o + 36;
        auto cigar_at = [&](uint32_t q) -> uint32_t { return in_win ? lds32(cig_ro + 4 * q) : ld32(g_data + h.l_qname + 4 * (size_t)q); };
        auto tag_strand = [&](uint8_t t0, uint8_t t1, bool *unknown) -> char {
            const int64_t l_data = (int64_t)h.block_len - 32;
            // two call sites on purpose: the LDS one compiles to ds_read_u8, the other to global loads (no flat/generic pointer)
            if (in_win) { const uint8_t *body = s_buf + ro + 36; return strand_from_tag(body + h.aux_off, body + l_data, t0, t1, unknown); }
            return strand_from_tag(g_data + h.aux_off, g_data + l_data, t0, t1, unknown);
        };
        decode_record(h, base + k, o, cfg, soa, t, cigar_at, tag_strand);
    }
    // per-segment totals instead of global atomics: one hot address serialises at ~90 atomics/us
    const uint32_t n_iter = wave_incl_scan(t.n_iter), n_long = wave_incl_scan(t.n_long);
    if (lane == 63) { seg_iter[s] = n_iter; seg_long[s] = n_long; }
    if (cfg.stop_out) stop_reduce(cfg.stop_out, t.first_stop, t.last_in);
}

// Long records (k_decode_seg<false>'s workload: two or three records per 16 KiB segment), one LANE per segment.  A wave per segment is a workgroup
// per two records there -- 4 M workgroups of which one lane works, each a chain of dependent gathers (checkpoint, the records' lengths, head, CIGAR, aux):
// 10.6 ms for config 5's 10 M records.  Here a lane follows its own segment's records from the verified start; sixty-four chains per wave.
// Same rows, same counts: decode_record with every read from the arena.
__global__ __launch_bounds__(64) void k_decode_sparse(const uint8_t *__restrict__ arena, uint32_t n_seg, const uint64_t *__restrict__ seg_start,
                                                      const uint32_t *__restrict__ seg_base, const uint32_t *__restrict__ seg_cnt, ExtractCfg cfg, ReadSoA soa,
                                                      uint32_t *seg_iter, uint32_t *seg_long, uint32_t s_begin) {
    const uint32_t s = s_begin + blockIdx.x * 64 + threadIdx.x;
    DecodeTally t;
    if (s < n_seg) {
        const uint32_t cnt = seg_cnt[s];
        uint64_t o = cnt ? seg_start[s] : 0;
        const uint32_t base = cnt ? seg_base[s] : 0;
        for (uint32_t k = 0; k < cnt; ++k) {
            RecHead h;
            rec_head(arena + o, h);
            const uint8_t *g_data = arena + o + 36;
            auto cigar_at = [&](uint32_t q) -> uint32_t { return ld32(g_data + h.l_qname + 4 * (size_t)q); };
            auto tag_strand = [&](uint8_t t0, uint8_t t1, bool *unknown) -> char {
                return strand_from_tag(g_data + h.aux_off, g_data + ((int64_t)h.block_len - 32), t0, t1, unknown);
            };
            decode_record(h, base + k, o, cfg, soa, t, cigar_at, tag_strand);
            o += 4 + (uint64_t)(uint32_t)h.block_len;
        }
        seg_iter[s] = t.n_iter; seg_long[s] = t.n_long;
    }
    if (cfg.stop_out) stop_reduce(cfg.stop_out, t.first_stop, t.last_in);
}

// list of the reads that go to the wave-per-read kernel, built without atomics: one wave per segment, positions from the
// exclusive scan of the per-segment counts
__global__ __launch_bounds__(64) void k_long_fill(uint32_t n_seg, const uint32_t *__restrict__ seg_base, const uint32_t *__restrict__ seg_cnt,
                                                  const uint32_t *__restrict__ seg_long_base, ExtractCfg cfg, ReadSoA soa, uint32_t *long_list) {
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    const uint32_t cnt = seg_cnt[s], base = seg_base[s];
    uint32_t out = seg_long_base[s];
    for (uint32_t k0 = 0; k0 < cnt; k0 += 64) {
        const uint32_t k = k0 + lane;
        bool is_long = false;
        if (k < cnt) is_long = soa.n_ev[base + k] != 0 && (soa.flag_nc[base + k] & 0xffff) > cfg.long_threshold;
        const uint64_t m = __ballot(is_long);
        if (is_long) long_list[out + (uint32_t)__popcll(m & lanemask_lt())] = base + k;
        out += (uint32_t)__popcll(m);
    }
}

const DecodeKnobs &decode_knobs() {
    static const DecodeKnobs k = [] {
        DecodeKnobs v;
        if (const char *e = getenv("REGTOOLS_AMD_DECODE")) {
            v.wave_form = !strncmp(e, "wave", 4);
            if (const char *c = strchr(e, ',')) v.seg_bytes = atoi(c + 1);
        }
        return v;
    }();
    return k;
}
void launch_decode_seg(const uint8_t *arena, SegGeom g, uint32_t n_seg, const uint64_t *seg_start, const uint32_t *seg_base,
                       const uint32_t *seg_cnt, ExtractCfg cfg, ReadSoA soa, uint32_t *seg_iter, uint32_t *seg_long, const uint16_t *seg_cp, bool staged, hipStream_t stream,
                       uint32_t s_begin) {
    if (n_seg <= s_begin) return;
    const uint32_t n = n_seg - s_begin;
    if (staged && g.seg_bytes == kSegBytes) hipLaunchKernelGGL(k_decode_seg<true>, dim3(n), dim3(64), kSegBytes + kSegTail + 48, stream, arena, g, n_seg, seg_start, seg_base, seg_cnt, cfg, soa, seg_iter, seg_long, seg_cp, s_begin);
    else {
        static const bool wave_form = decode_knobs().wave_form;     // (tests: the workgroup-per-segment form it replaced)
        if (wave_form && g.seg_bytes == kSegBytes) hipLaunchKernelGGL(k_decode_seg<false>, dim3(n), dim3(64), 0, stream, arena, g, n_seg, seg_start, seg_base, seg_cnt, cfg, soa, seg_iter, seg_long, seg_cp, s_begin);
        else hipLaunchKernelGGL(k_decode_sparse, dim3((n + 63) / 64), dim3(64), 0, stream, arena, n_seg, seg_start, seg_base, seg_cnt, cfg, soa, seg_iter, seg_long, s_begin);
    }
}
// identify -s XS: the reads whose strand tag lies behind an aux field of unknown type (marked by the decode kernels), with the span the iterator tests
__global__ void k_collect_odd_aux(const uint8_t *__restrict__ arena, ReadSoA soa, uint32_t n_rec, uint32_t cap, uint32_t *count, int32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec || !(soa.strand[i] & 0x80u)) return;
    const uint32_t fnc = soa.flag_nc[i];
    const int32_t pos = soa.pos[i];
    const uint32_t k = atomicAdd(count, 1u);
    if (k < cap) { out[3 * (size_t)k] = soa.tid[i]; out[3 * (size_t)k + 1] = pos; out[3 * (size_t)k + 2] = rec_endpos(arena + soa.cig_off[i], fnc & 0xffffu, fnc >> 16, pos); }
}
void launch_collect_odd_aux(const uint8_t *arena, ReadSoA soa, uint32_t n_rec, uint32_t cap, uint32_t *count, int32_t *out, hipStream_t stream) {
    if (n_rec) hipLaunchKernelGGL(k_collect_odd_aux, dim3((n_rec + 255) / 256), dim3(256), 0, stream, arena, soa, n_rec, cap, count, out);
}
void launch_long_fill(uint32_t n_seg, const uint32_t *seg_base, const uint32_t *seg_cnt, const uint32_t *seg_long_base, ExtractCfg cfg, ReadSoA soa,
                      uint32_t *long_list, hipStream_t stream) {
    if (n_seg) hipLaunchKernelGGL(k_long_fill, dim3(n_seg), dim3(64), 0, stream, n_seg, seg_base, seg_cnt, seg_long_base, cfg, soa, long_list);
}

}  // namespace rgx
