// front_plan.h -- what the front of an extract call asks the device to do (api_front.cpp stage_upload / stage_members / stage_range_and_inflate and the
// early-tail loop of api_records.cpp stage_framing), as integer arithmetic over the member list, the index's answers and a few knobs: which bytes of
// the file go up and in which chunks, whether the launch is arrival-gated, which members each launch or part covers, where the early tail cuts the member
// list, how many segments of the arena a part may frame.  Nothing here touches the device or a context: the stages call these and enqueue what they
// say; tests/hostemu builds them with plain g++ (tests/test_front_plan_host.py restates every rule by brute force).
#pragma once
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "common.h"

namespace rgx {

// Which options suit a payload, from how well the file compresses (round 4, 50 M-read files / 10 M long reads on one box, ms, all byte-equal to zlib;
// tools/lab/forms_r4.sh, profiles/r04_inflate_forms.txt):
//   inflated / compressed > 32  (long reads: run-length copies)        k_inflate_coop, windowed bit reader, one symbol per trip, lanes in file order:
//                                                                      117.5-118.7 (round 3's choice -- plain reader -- 120.7-122.2; pairs + sorted lanes 122; k_inflate 131)
//   <= 32                       (the bench payload: 21;                 k_inflate_coop, windowed bit reader, literal pairs, lanes sorted by compressed length
//                                random bases + binned qualities: 3.6)  per 1024 members: bench payload 14.5-15.2 (k_inflate 19.9-21.3); random bases 44.9-47.5
//                                                                      (k_inflate with four literals per trip, round 3's choice for them: 53.1-54.1)
// bit 0 = literal pairs + sorted lanes.  (k_inflate stays selectable: REGTOOLS_AMD_INFLATE=lane, form 1 / 5 of the stage entry point.)
// Second half of round 4 (k_inflate_coop's mode word, launch_inflate): runs at distances of 16 bytes or less are written from registers, 64 bytes a
// trip, for every class (long reads 121.2 -> 79.8 ms: half their trips were such runs growing 1, 2, 4 ... bytes a trip, each with a partial-chunk
// store); up to 32 x also a literal pair and the match behind it in one trip, bits counted exactly (bench payload 2,030 -> 1,463 trips per
// member, 15.2 -> 14.1-15.0 ms: the launch follows its memory requests, not its trips).
inline int inflate_plan_for(uint64_t compressed_bytes, uint64_t inflated_bytes) {
    return compressed_bytes * 32 > inflated_bytes ? 1 : 0;
}

// "." (or no region) = every record from the first one on; "*" = every record behind the last reference's reads (hts_itr_querys, hts.c:1901-1904:
// HTS_IDX_START / HTS_IDX_NOCOOR; both read to the end of the file without a predicate); anything else is a query the index answers.
enum class RegionKind { whole, rest, query };
inline RegionKind region_kind(const char *region) {
    if (!region || !strcmp(region, ".")) return RegionKind::whole;
    return !strcmp(region, "*") ? RegionKind::rest : RegionKind::query;
}

// Shard cut points: shard g of n starts at the first virtual offset the index lists (bai_first_anchor_ge) at or behind g / n of the file's bytes, and
// never in front of where the record stream starts (floor_voff: the seek target, or 1 = "behind offset 0").  tgt[0] is this shard's target, tgt[1]
// the next one's.
inline void shard_cut_targets(size_t bam_len, int shard, int n_shards, uint64_t floor_voff, uint64_t tgt[2]) {
    for (int k = 0; k < 2; ++k) tgt[k] = std::max<uint64_t>((uint64_t)((double)bam_len * (shard + k) / n_shards) << 16, floor_voff);
}

// The bytes of the file a shard of a shared member scan sends up: [lo, hi) between its two cuts (got[] = the index's answers to shard_cut_targets;
// UINT64_MAX = no anchor behind the target) and the header's [0, hdr_hi).  hi carries two members and a bit of slack behind the upper cut (a record
// belongs to the shard in which its first byte lies: it may end in the next member); the header is header_bytes, and at least the four members the
// device-side header read starts with (fourth_member_end; 0 = no member list); lo is rounded down to 4 KiB, and a range that then meets the header
// starts at byte 0 instead.
struct UploadRange { size_t lo, hi, hdr_hi; };
inline UploadRange shard_upload_range(size_t bam_len, int shard, int n_shards, const uint64_t got[2], size_t header_bytes, size_t fourth_member_end) {
    size_t up_lo = 0, up_hi = bam_len, hdr_hi = 0;
    if (shard > 0 && got[0] != UINT64_MAX) up_lo = std::min<size_t>(bam_len, (size_t)(got[0] >> 16));
    else if (shard > 0) up_lo = bam_len;
    if (shard + 1 < n_shards && got[1] != UINT64_MAX) up_hi = std::min<size_t>(bam_len, (size_t)(got[1] >> 16) + 2 * kBgzfMaxBlock + 64);
    if (up_hi < up_lo) up_hi = up_lo;
    const size_t hb = std::max(header_bytes, fourth_member_end);
    hdr_hi = std::min(up_lo, hb + 64);
    up_lo &= ~(size_t)4095;
    if (up_lo < hdr_hi) { up_lo = 0; hdr_hi = 0; }
    return UploadRange{up_lo, up_hi, hdr_hi};
}

// The arrival gate is for payloads whose inflate is of the upload's order (measured: bench payload 27.5 -> 26.5 ms, random bases + qualities 98.2 ->
// 93.7); run-length payloads (long reads: 1 GB of file, 65 GB inflated, five rounds of waves) lose 5-6 ms of 158 to it and keep the pieces.  The
// class comes from the file's first members (BSIZE / ISIZE of up to 64 of them: what the host scan will find).
inline bool payload_takes_gate(const uint8_t *h_bam, size_t bam_len) {
    uint64_t cb = 0, ub = 0; size_t o = 0;
    for (int k = 0; k < 64 && o + 28 <= bam_len; ++k) {
        if (!(h_bam[o] == 0x1f && h_bam[o + 1] == 0x8b && h_bam[o + 12] == 'B' && h_bam[o + 13] == 'C')) break;
        const size_t bl = (size_t)(h_bam[o + 16] | h_bam[o + 17] << 8) + 1;
        if (bl < 26 || o + bl > bam_len) break;
        uint32_t isz; memcpy(&isz, h_bam + o + bl - 4, 4);
        cb += bl; ub += isz; o += bl;
    }
    return !(cb && !(inflate_plan_for(cb, ub) & 1));
}

// The upload's chunks: end[j] = bytes [up_lo, end[j]) are resident once chunk j has landed; the last end is up_hi.
//   gated     gate_chunks equal chunks of gate_chunk bytes (a multiple of 4 KiB) behind ONE launch whose waves wait for their chunk;
//   otherwise three pieces, each its own launch on its own hardware queue (two side streams + the pipeline's own; a launch takes ~8 ms however
//             small -- one lane per member).  Equal thirds measured best: 31.6 ms per step against 32.4-33.3 ms for pieces that shrink towards
//             the end, and 30.9-31.5 ms for four to six equal pieces on side streams of other priorities (= other queue pools), 32.6 for seven
//             (tools/lab/pieces.sh): the concurrent launches share the chip, finer pieces do not end sooner;
//   one_shot  one chunk (one stream: pieces would only take turns on it).
struct UploadChunks { size_t gate_chunk = 0; std::vector<size_t> end; };
inline UploadChunks plan_upload_chunks(size_t up_lo, size_t up_hi, bool gated, unsigned gate_chunks, bool one_shot) {
    UploadChunks u;
    std::vector<unsigned> cuts = {33, 67};
    if (one_shot) cuts.clear();
    if (gated) {
        u.gate_chunk = (((up_hi - up_lo) + gate_chunks - 1) / gate_chunks + 4095) & ~(size_t)4095;
        for (size_t e = up_lo + u.gate_chunk; e < up_hi; e += u.gate_chunk) u.end.push_back(e);
    } else
    for (unsigned pc : cuts) {
        const size_t e = (up_lo + (size_t)((double)(up_hi - up_lo) * pc / 100.0) + 4095) & ~(size_t)4095;
        if (e < up_hi && e > up_lo && (u.end.empty() || e > u.end.back())) u.end.push_back(e);
    }
    u.end.push_back(up_hi);
    return u;
}

// What k_member_query / k_member_stop answer on the device, from a member list that is on the host: q_index[k] = the member whose payload starts at
// q[k] + 18 (q[k] = the member's own offset in the file), n when there is none, and its arena offset (~0 when there is none); stop = the first empty
// (or oversized = corrupt) member at / behind q_index[0], where the stream ends (bgzf.c:548-578), 0xffffffff when there is none.
struct MemberQuery { uint32_t q_index[3]; uint64_t q_upos[3]; uint32_t stop; };
inline MemberQuery host_member_query(const Member *hm, uint32_t nm, const uint64_t q[3]) {
    MemberQuery r;
    for (int k = 0; k < 3; ++k) {
        uint32_t lo_ = 0, hi_ = nm;
        while (lo_ < hi_) { const uint32_t mid = lo_ + (hi_ - lo_) / 2; if (hm[mid].cpos < q[k] + 18) lo_ = mid + 1; else hi_ = mid; }
        const bool hit = lo_ < nm && hm[lo_].cpos == q[k] + 18;
        r.q_index[k] = hit ? lo_ : nm; r.q_upos[k] = hit ? hm[lo_].upos : ~0ull;
    }
    uint32_t stop_ = 0xffffffffu;
    for (uint32_t i = r.q_index[0]; i < nm; ++i) if (hm[i].isize == 0 || hm[i].isize > kBgzfMaxBlock) { stop_ = i; break; }
    r.stop = stop_;
    return r;
}

// The member range [m_lo, m_hi) of a call, from its two cuts (virtual offsets; cut_lo 0 = "right after the header", cut_hi UINT64_MAX = none), the
// members at the cuts (q_index[1], q_index[2]) and where the stream stops.
inline void member_range(uint64_t cut_lo, uint64_t cut_hi, const uint32_t q_index[3], uint32_t stop, uint32_t n_members_all, bool chunked,
                         bool region_to_file_end, uint32_t &m_lo, uint32_t &m_hi) {
    m_lo = cut_lo ? q_index[1] : 0;
    if (m_lo <= 4) m_lo = 0;        // keep the file head (BAM header) in the same launch: a lone lane needs milliseconds per member
    m_hi = stop;                                                  // exclusive
    if (cut_hi != UINT64_MAX) {
        const uint32_t mh = q_index[2];
        const uint32_t hi_m = (mh < n_members_all && (cut_hi & 0xffff)) ? mh + 1 : mh;
        // a region's chunks: each is a seek of its own, so an empty member between two of them ends nothing (the chunks' own limits do
        // that); two members more than the index asks for, for the records of a stale index that run past their chunk's end
        if (chunked) m_hi = region_to_file_end ? n_members_all : (uint32_t)std::min<uint64_t>(n_members_all, (uint64_t)hi_m + 2);
        else m_hi = std::min(stop, hi_m);
    }
    if (m_lo > m_hi) m_lo = m_hi;
}

// How far behind the end of its payload (cpos + clen) a member's lane reads the file:
//   kGateLookahead   k_inflate_coop, the arrival-gated launch: the footer (8 bytes) and the 16-byte window of its bit reader -- gate_chunk_needed is
//                    the kernel's own rule, and the early tail's parts are cut by the same one;
//   kPieceLookahead  the launches per upload chunk and the bytes a shard sends up: the decoder's 16-byte look-ahead.
constexpr uint32_t kGateLookahead = 24, kPieceLookahead = 16;

// the first member of [lo, hi) that reads bytes at or behind byte lim_b of the file (hi when none does)
inline uint32_t first_member_reading_past(const Member *hm, uint32_t lo, uint32_t hi, uint64_t lim_b, uint32_t lookahead) {
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (hm[mid].cpos + hm[mid].clen + lookahead <= lim_b) lo = mid + 1; else hi = mid; }
    return lo;
}

// the upload chunk with the last byte a member's lane reads (chunk k = bytes [gate_lo + k * chunk_bytes, + chunk_bytes) of the file, the last one
// of n_chunks to the range's end)
RGX_HD uint32_t gate_chunk_needed(uint64_t cpos, uint32_t clen, uint64_t gate_lo, uint64_t chunk_bytes, uint32_t n_chunks) {
    uint64_t end_b = cpos + clen + kGateLookahead;
    end_b = end_b > gate_lo ? end_b - gate_lo : 0;
    const uint64_t last = n_chunks - 1, k = end_b / chunk_bytes;
    return (uint32_t)(k < last ? k : last);
}

// only a byte range [up_lo, up_hi) of the file went up (a shard of a shared scan): whether it holds every byte the members [m_lo, m_hi) are read from
inline bool upload_covers_members(const Member *hm, uint32_t m_lo, uint32_t m_hi, size_t up_lo, size_t up_hi) {
    const uint64_t need_lo = hm[m_lo].cpos - 18, need_hi = hm[m_hi - 1].cpos + hm[m_hi - 1].clen + kPieceLookahead;
    return !(need_lo < up_lo || need_hi > up_hi);
}

// One launch per upload chunk: chunk j's launch takes the members [g_lo, g_hi) whose bytes (plus the look-ahead) have arrived with it and that no
// earlier chunk's launch took; the last chunk's takes what is left.  A chunk that completes no member has no launch.  In order, the pieces are
// [m_lo, m_hi).
struct Piece { uint32_t chunk, g_lo, g_hi; };
inline std::vector<Piece> plan_pieces(const Member *hm, uint32_t m_lo, uint32_t m_hi, const size_t *end, size_t n_end) {
    std::vector<Piece> pieces;
    uint32_t g_lo = m_lo;
    for (size_t j = 0; j < n_end && g_lo < m_hi; ++j) {
        uint32_t g_hi = m_hi;
        if (j + 1 < n_end) g_hi = first_member_reading_past(hm, g_lo, m_hi, end[j], kPieceLookahead);
        if (g_hi == g_lo) continue;
        pieces.push_back(Piece{(uint32_t)j, g_lo, g_hi});
        g_lo = g_hi;
    }
    return pieces;
}

// REGTOOLS_AMD_EARLY_TAIL: the early tail's cuts in sixteenths of the upload, ascending, up to seven; "0" = none
inline std::vector<unsigned> parse_early_cuts(const char *env_text) {
    std::vector<unsigned> v;
    unsigned x7[7] = {0, 0, 0, 0, 0, 0, 0};
    const int n = sscanf(env_text ? env_text : "6,9,12,14", "%u,%u,%u,%u,%u,%u,%u", &x7[0], &x7[1], &x7[2], &x7[3], &x7[4], &x7[5], &x7[6]);
    for (unsigned x : x7) if ((int)v.size() < n && x > 0 && x < 16 && (v.empty() || x > v.back())) v.push_back(x);
    return v;
}

// Early tail: a part ends in front of member `members` of the range = workgroup `waves` = arena offset `upos`.  Every cut (a sixteenth of the
// upload's chunks) becomes the first member that reads bytes behind its chunk -- k_inflate_coop's own rule -- rounded down to a multiple of `align`
// (a wave's members all come from one group of that many: kInflateSortGroup); a part of fewer than early_min members, or one that leaves fewer
// than that behind it, is not cut.
struct EarlyPart { uint32_t members, waves; uint64_t upos; };
inline std::vector<EarlyPart> plan_early_parts(const Member *hm, uint32_t m_lo, uint32_t m_hi, uint64_t upos_lo, const size_t *end, size_t n_end,
                                               const std::vector<unsigned> &cuts, uint32_t early_min, uint32_t align) {
    std::vector<EarlyPart> early_parts;
    const uint32_t n_range = m_hi - m_lo;
    for (unsigned cut : cuts) {
        const size_t kA = std::max<size_t>(1, n_end * (size_t)cut / 16);
        const uint32_t lo = first_member_reading_past(hm, m_lo, m_hi, end[kA - 1], kGateLookahead);
        uint32_t k = (lo - m_lo) / align * align;     // members of the range in front of the cut
        const uint32_t prev = early_parts.empty() ? 0u : early_parts.back().members;
        if (k >= prev + early_min && n_range - k >= early_min) early_parts.push_back(EarlyPart{k, k / 64, hm[m_lo + k].upos - upos_lo});
    }
    return early_parts;
}

// Early tail: how many segments of the arena (seg_bytes each, from pos0) the stream may frame once the part that ends at arena offset part_upos is
// inflated -- those that lie wholly in front of it, with one member's margin (a walk only ever reads the 36 bytes behind its segment) -- or 0: the
// part is skipped.  s_done segments are framed already; a part is worth its wait from 1,024 new segments on and while 64 remain behind it (small_ok,
// the tests' knob: 2 and 1).
inline uint32_t early_prefix_segments(uint64_t part_upos, uint64_t pos0, uint32_t seg_bytes, uint32_t n_seg, uint32_t s_done, bool small_ok) {
    if (part_upos <= pos0 + 2 * (uint64_t)kBgzfMaxBlock) return 0;
    const uint32_t sJ = (uint32_t)std::min<uint64_t>(n_seg, (part_upos - kBgzfMaxBlock - pos0) / seg_bytes);
    if (small_ok ? (sJ < s_done + 2 || n_seg - sJ < 1) : (sJ < s_done + 1024 || n_seg - sJ < 64)) return 0;
    return sJ;
}

}  // namespace rgx
