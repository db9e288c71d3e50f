// emit_kernels.hip -- the CIGAR scan and the junction events: one event per N operation that passes junction_qc,
// at the slot the exclusive scan of the reads' event counts gives it.  Called by api_records.cpp; the CIGAR rules (cigar_walk, intron_ok,
// strand_from_motif, rec_endpos) are bam_core.h's.
//   k_emit_short   one lane per read, the serial state machine (reads of up to ExtractCfg::long_threshold operations)
//   k_emit_long    one wave per read of the long list (k_long_fill): operations in tiles of 64, classified with ballots, positioned with a
//                  wave prefix sum of the reference advance
#include "wave_prims.h"

namespace rgx {

__device__ __forceinline__ void put_event(const EventSoA &ev, uint32_t slot, int32_t tid, uint32_t start, uint32_t end, uint32_t ts,
                                          uint32_t te, char strand, uint32_t rpos, uint32_t rend, uint32_t read) {
    if (ev.read) ev.read[slot] = read;
    ev.tid[slot] = (uint32_t)tid; ev.start[slot] = start;
    ev.ilen_cls[slot] = (end - start) << 2 | strand_class(strand);
    ev.ts[slot] = ts; ev.te[slot] = te; ev.strand[slot] = (uint8_t)strand;
    if (ev.rpos) { ev.rpos[slot] = rpos; ev.rend[slot] = rend; }
}

// short reads: one lane per read, the serial state machine (config 2: 1 or 3 ops)
// (row_begin, part_totals, n_parts: the early tail emits the rows of one part of the file at a time; ev_base then counts from the part's first row, and the
//  events of the parts in front of it -- their totals sit in device memory, nobody waited for them -- are added here)
__global__ void k_emit_short(const uint8_t *__restrict__ arena, uint32_t n_rec, ExtractCfg cfg, ReadSoA soa,
                             const uint32_t *__restrict__ ev_base, EventSoA ev, uint32_t row_begin, const uint32_t *__restrict__ part_totals, uint32_t n_parts, uint32_t slot_cap) {
    uint32_t i = row_begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    uint32_t nev = soa.n_ev[i];
    if (!nev) return;
    uint32_t fnc = soa.flag_nc[i], n_cigar = fnc & 0xffff;
    if (n_cigar > cfg.long_threshold) return;
    const uint8_t *cig = arena + soa.cig_off[i];
    int32_t tid = soa.tid[i];
    char strand = (char)soa.strand[i];
    uint32_t slot = ev_base[i];
    for (uint32_t k = 0; k < n_parts; ++k) slot += part_totals[k];
    const int32_t pos = soa.pos[i];
    const uint32_t rend = ev.rpos ? (uint32_t)rec_endpos(cig, n_cigar, fnc >> 16, pos) : 0u;     // bam_endpos of the supporting read
    char carried = 0;
    cigar_walk(pos, cig, n_cigar, [&](uint32_t s, uint32_t e, uint32_t ts, uint32_t te) {
        char st = strand;
        if (cfg.fa_data) {
            // set_junction_strand (junctions_extractor.cc:345-359): motif first, the tag/flag rule only when the motif says '?'.
            // The strand is decided (and carried to the read's next junction) BEFORE junction_qc.
            const FaContig fc = cfg.fa_tab[tid];
            if (!fc.present) { cfg.fa_missing[0] = 1u + (uint32_t)tid; }
            else { const char m = strand_from_motif(cfg.fa_data, fc, s, e, carried); if (m != '?') st = m; }
            carried = st;
        }
        if (intron_ok(s, e, cfg.min_intron, cfg.max_intron)) { if (slot < slot_cap) put_event(ev, slot, tid, s, e, ts, te, st, (uint32_t)pos, rend, i); ++slot; }   // (slot_cap: a block sized before the count was known)
    });
}

// long reads: one WAVE per read. Ops are staged through LDS in tiles of 64, classified with ballots and
// positioned with a wave prefix sum of reference advance (parallel form):
//   for the N op at index i:  start = R[i], end = R[i+1],
//                             thick_start = R[pb+1]  (pb = last breaker {N,D,X,I,S} before i, or read start),
//                             thick_end   = R[nb]    (nb = first breaker after i, or read end).
__global__ __launch_bounds__(256) void k_emit_long(const uint8_t *__restrict__ arena, const uint32_t *__restrict__ long_list,
                                                   uint32_t n_long, ExtractCfg cfg, ReadSoA soa,
                                                   const uint32_t *__restrict__ ev_base, EventSoA ev) {
    __shared__ uint32_t s_ops[4][64];
    __shared__ uint32_t s_R[4][65];
    const uint32_t wave = threadIdx.x >> 6, lane = lane_id();
    // (round 4: a read is three dependent round trips -- its index, its row, its CIGAR -- in front of ~200 instructions: the NEXT read's index and row are
    //  requested while this one's CIGAR is in flight and its junctions are worked out, so that an iteration waits for one round trip, not three)
    const uint32_t stride = gridDim.x * 4;
    uint32_t w = blockIdx.x * 4 + wave;
    if (w >= n_long) return;
    uint32_t nx_i = long_list[w];
    uint32_t nn_i = w + stride < n_long ? long_list[w + stride] : 0u;          // (the index of the read after the next: its row's loads must not wait for it)
    uint32_t nx_fnc = soa.flag_nc[nx_i], nx_slot = ev_base[nx_i];
    uint64_t nx_cig = soa.cig_off[nx_i];
    int32_t nx_tid = soa.tid[nx_i], nx_pos = soa.pos[nx_i];
    uint8_t nx_strand = soa.strand[nx_i];
    for (; w < n_long; w += stride) {
        const uint32_t i = nx_i, fnc = nx_fnc;
        const uint32_t n_cigar = fnc & 0xffff;
        const uint8_t *cig = arena + nx_cig;
        const int32_t tid = nx_tid;
        const char strand = (char)nx_strand;
        uint32_t slot = nx_slot;
        const uint32_t rpos = (uint32_t)nx_pos;
        // this read's first CIGAR tile: requested now, looked at below
        const uint32_t c_first = lane < n_cigar ? ld32(cig + 4 * (size_t)lane) : 0x5u /* 0H: inert */;
        // ... the next read's row behind it (its index came with the last iteration), and the index of the one after
        if (w + stride < n_long) {
            nx_i = nn_i;
            nx_fnc = soa.flag_nc[nx_i]; nx_slot = ev_base[nx_i]; nx_cig = soa.cig_off[nx_i]; nx_tid = soa.tid[nx_i]; nx_pos = soa.pos[nx_i]; nx_strand = soa.strand[nx_i];
            if (w + 2 * stride < n_long) nn_i = long_list[w + 2 * stride];
        }
        uint32_t rend = 0;
        if (ev.rpos) {                               // bam_endpos (sam.c:336-342): pos + reference span, or pos+1 for unmapped-flagged reads
            uint32_t span = 0;
            for (uint32_t t0 = lane; t0 < n_cigar; t0 += 64) span += cig_ref_len(ld32(cig + 4 * (size_t)t0));
            span = __shfl(wave_incl_scan(span), 63, 64);
            rend = ((fnc >> 16) & 4u) ? rpos + 1 : rpos + span;
        }
        uint32_t refpos = rpos;                      // R at the start of the tile
        uint32_t ts_carry = refpos;                  // R[pb+1] for an N with no breaker earlier in the tile
        // junction opened in an earlier tile and still waiting for its right anchor's end
        bool pend = false; uint32_t p_start = 0, p_end = 0, p_ts = 0; char p_strand = strand;
        char carried = 0;                            // intron-motif rule: strand of the read's previous junction
        for (uint32_t t0 = 0; t0 < n_cigar; t0 += 64) {
            const uint32_t k = t0 + lane;
            const uint32_t c = t0 == 0 ? c_first : k < n_cigar ? ld32(cig + 4 * (size_t)k) : 0x5u /* 0H: inert */;
            s_ops[wave][lane] = c;
            const uint32_t adv = cig_advances_junction_state(c) ? (c >> 4) : 0u;
            const uint32_t incl = wave_incl_scan(adv);
            const uint32_t R_before = refpos + incl - adv, R_after = refpos + incl;
            s_R[wave][lane] = R_before;
            if (lane == 63) s_R[wave][64] = R_after;
            const bool brk = k < n_cigar && cig_is_breaker(c);
            const bool isN = k < n_cigar && cig_is_N(c);
            const uint64_t B = __ballot(brk);
            __builtin_amdgcn_wave_barrier();
            // close the pending junction at this tile's first breaker
            if (pend && B) {
                const uint32_t nb = (uint32_t)__ffsll((unsigned long long)B) - 1;
                const uint32_t te = s_R[wave][nb];
                if (lane == 0 && intron_ok(p_start, p_end, cfg.min_intron, cfg.max_intron)) put_event(ev, slot, tid, p_start, p_end, p_ts, te, p_strand, rpos, rend, i);
                if (intron_ok(p_start, p_end, cfg.min_intron, cfg.max_intron)) ++slot;
                pend = false;
            }
            // per-lane junction geometry
            const uint64_t below = B & lanemask_lt();
            const uint64_t above = lane == 63 ? 0ull : (B >> (lane + 1)) << (lane + 1);
            const uint32_t ts = below ? s_R[wave][(63 - (uint32_t)__clzll((long long)below)) + 1] : ts_carry;
            const bool closed = above != 0;
            const uint32_t te = closed ? s_R[wave][(uint32_t)__ffsll((unsigned long long)above) - 1] : 0u;
            const bool ok = isN && intron_ok(R_before, R_after, cfg.min_intron, cfg.max_intron);
            // strand of this lane's junction: per-read tag/flag rule, or the intron-motif rule with its carried-over state --
            // a two-state chain over the N ops in CIGAR order, resolved lane by lane (a long read has a few dozen at most)
            char my_strand = strand;
            if (cfg.fa_data) {
                const FaContig fc = cfg.fa_tab[tid];
                char sA = strand, sB = strand;           // outcome if the carried strand is not '-' / is '-'
                if (isN) {
                    if (!fc.present) cfg.fa_missing[0] = 1u + (uint32_t)tid;
                    else {
                        const char mA = strand_from_motif(cfg.fa_data, fc, R_before, R_after, 0), mB = strand_from_motif(cfg.fa_data, fc, R_before, R_after, '-');
                        if (mA != '?') sA = mA;
                        if (mB != '?') sB = mB;
                    }
                }
                uint64_t nm = __ballot(isN);
                while (nm) {
                    const uint32_t l = (uint32_t)__ffsll((unsigned long long)nm) - 1; nm &= nm - 1;
                    const char a = (char)__shfl((int)sA, l, 64), b = (char)__shfl((int)sB, l, 64);
                    const char s = carried == '-' ? b : a;
                    if (lane == l) my_strand = s;
                    carried = s;
                }
            }
            // events keep CIGAR order: rank among the qc-passing N lanes that close inside this tile
            const uint64_t emit_mask = __ballot(ok && closed);
            if (ok && closed) put_event(ev, slot + (uint32_t)__popcll(emit_mask & lanemask_lt()), tid, R_before, R_after, ts, te, my_strand, rpos, rend, i);
            slot += (uint32_t)__popcll(emit_mask);
            // the last breaker of the tile: if it is an N it stays open into the next tile
            if (B) {
                const uint32_t lastb = 63 - (uint32_t)__clzll((long long)B);
                const uint32_t lc = s_ops[wave][lastb];
                ts_carry = s_R[wave][lastb + 1];
                if (cig_is_N(lc)) {
                    pend = true;
                    p_start = s_R[wave][lastb]; p_end = s_R[wave][lastb + 1];
                    const uint64_t bl = B & ((1ull << lastb) - 1ull);
                    p_ts = __shfl(ts, lastb, 64);
                    p_strand = (char)__shfl((int)my_strand, lastb, 64);
                    (void)bl;
                }
            }
            refpos = __shfl(R_after, 63, 64);
            __builtin_amdgcn_wave_barrier();
        }
        if (pend && lane == 0 && intron_ok(p_start, p_end, cfg.min_intron, cfg.max_intron)) put_event(ev, slot, tid, p_start, p_end, p_ts, refpos, p_strand, rpos, rend, i);
    }
}

void launch_emit_short(const uint8_t *arena, uint32_t n_rec, ExtractCfg cfg, ReadSoA soa, const uint32_t *ev_base, EventSoA ev,
                       hipStream_t stream, uint32_t row_begin, const uint32_t *part_totals, uint32_t n_parts, uint32_t slot_cap) {
    if (n_rec <= row_begin) return;
    hipLaunchKernelGGL(k_emit_short, dim3((n_rec - row_begin + 255) / 256), dim3(256), 0, stream, arena, n_rec, cfg, soa, ev_base, ev, row_begin, part_totals, n_parts, slot_cap);
}
void launch_emit_long(const uint8_t *arena, const uint32_t *long_list, uint32_t n_long, ExtractCfg cfg,
                      ReadSoA soa, const uint32_t *ev_base, EventSoA ev, hipStream_t stream) {
    if (!n_long) return;
    uint32_t blocks = (n_long + 3) / 4;
    if (blocks > 256 * 8) blocks = 256 * 8;       // grid-stride: 8 workgroups per CU
    hipLaunchKernelGGL(k_emit_long, dim3(blocks), dim3(256), 0, stream, arena, long_list, n_long, cfg, soa, ev_base, ev);
}

}  // namespace rgx
