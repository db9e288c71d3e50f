// kernels.h -- launchers of the gfx950 kernels (definitions in the .hip file each section names). All asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"
#include "bam_core.h"
#include "front_plan.h"

namespace rgx {

constexpr uint32_t kSegBytes = 16384;   // arena segment walked by one lane during record-boundary discovery
constexpr uint32_t kSparseRecordBytes = 2048;   // mean record size above which k_decode_seg reads records in place instead of staging segments
constexpr uint32_t kSegCpSlots = 64;     // checkpoints per segment: offset of every 8th record (a segment starts at most 457 records)
constexpr uint64_t kChainEnd = ~0ull;
constexpr uint64_t kChainUnknown = ~0ull - 1;   // exit of a segment in which the guess found nothing: no claim at all (not "the chain ended")   // "the record chain ended before this point" (truncated/corrupt stream)

// ---- a1: BGZF inflate (one lane per member; kernels.hip) ------------------------------------------------
// member m writes its bytes at arena + (members[m].upos - upos_bias)
// len_scratch: inflate_scratch_bytes(n_members) bytes of device memory (code-length scratch of the block headers)
size_t inflate_scratch_bytes(uint32_t n_members);
// an error of a kernel launch (refused configuration) or of a launch's set-up since this host thread last asked; hipSuccess = none (clears it)
hipError_t pending_launch_error();
// Arrival gate of the overlapped upload (round 4): ONE k_inflate_coop launch covers the whole range while the file is still on the bus; a wave
// starts once the upload chunk holding the last byte its members need has landed -- flags[k] == epoch, written by a 4-byte copy queued on the
// copy stream right behind chunk k (api_front.cpp stage_upload).  flags = nullptr: no gate.
struct InflateGate {
    const uint32_t *flags = nullptr;   // device memory, one word per upload chunk
    uint32_t epoch = 0;                // this call's value (the words keep earlier calls' values: smaller)
    uint32_t n_chunks = 0;
    uint64_t lo = 0, chunk_bytes = 1;  // chunk k = bytes [lo + k * chunk_bytes, lo + (k + 1) * chunk_bytes) of the file (the last one to the range's end)
    // Early tail (round 4): the launch's waves are counted as they finish, by part of the member list -- part j = the waves from part_start[j - 1]
    // (workgroup index; part 0 starts at 0) up to part_start[j] -- so that the pipeline's stream can frame and decode the front parts of the arena
    // (launch_wait_done) while the waves of the later parts still run.  done = null: nobody counts.
    uint32_t *done = nullptr;          // device memory, kGateParts words, zeroed by the caller in front of the launch
    uint32_t part_start[7] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
};
constexpr uint32_t kGateParts = 8;
constexpr uint32_t kInflateSortGroup = 1024;   // k_inflate_coop: the lanes of a wave take their members from one group of that many consecutive ones (k_member_sort)
// one lane on `stream` waits until done[0] reaches `expected` (a wave count); gives up after ~2 s and sets *timed_out
void launch_wait_done(const uint32_t *done, uint32_t expected, uint32_t *timed_out, hipStream_t stream);
constexpr uint32_t kStatusEarly = 76;   // status[kStatusEarly..+1]: the same pair for members below ignore_below (only written when that is > 0)
void launch_inflate(const uint8_t *comp, const Member *members, uint32_t n_members, uint8_t *arena, uint64_t upos_bias, uint32_t *len_scratch,
                    uint32_t *status /* [0]=first bad member (min), [1]=its status */, hipStream_t stream, uint32_t ignore_below = 0 /* failures of members below this index are not reported */,
                    uint32_t index_bias = 0 /* added to the launch's member index in status[] and in the ignore_below test: a range launched in pieces */,
                    bool piece = false /* one of several concurrent launches over a range (own kernel symbol, same code) */,
                    int form = 0 /* 0 = chosen by member count / REGTOOLS_AMD_INFLATE; 1 = k_inflate, 2 = k_inflate_wave, 3 = k_inflate_ring, 4 = k_inflate_coop,
                                     5 = k_inflate with four literals per trip */,
                    uint8_t *bad_flags = nullptr /* optional, zeroed by the caller: [index in the caller's range] = 1 for every member that did not inflate */,
                    int plan = 1 /* inflate_plan_for */,
                    bool check_layout = false /* a caller's own member list (stage entry point): k_inflate_coop only runs when the list's layout suits it */,
                    InflateGate gate = InflateGate() /* k_inflate_coop only: waves wait for their upload chunk */);
// whether launch_inflate would pick k_inflate_coop for a range of this size (the gate needs it)
bool inflate_takes_coop(uint32_t n_members);
// the host scan's member list (page-locked host memory, n_members + 1 members long) into a device block of the same length
void launch_members_fetch(const Member *host_members, Member *dst, uint32_t n_members, hipStream_t stream);
void launch_gate_set(uint32_t *flag, uint32_t epoch, hipStream_t stream);      // flags[k] = epoch, in stream order behind chunk k's copy
// (inflate_plan_for -- which options suit a payload -- is front_plan.h's)

// ---- a1 (container): BGZF member discovery on the device (members_kernels.hip; launch_inflate_probe: kernels.hip) ----
// The member chain (bgzf.c:525: next = this + BSIZE + 1) is serial on a CPU (one dependent cache miss per member).
// Here: (1) every byte offset is tested against check_header's predicate (bgzf.c:348-355) -> sorted candidate list
// (two passes: count per 4 KiB tile, scan, fill); (2) each candidate links to the candidate at off+BSIZE+1 (binary
// search); (3) reachability from offset 0 by pointer doubling (log2 n rounds) keeps exactly the members the serial walk
// would visit -- false positives inside compressed data are unreachable and drop out; (4) compaction + scan of ISIZE.
constexpr uint32_t kMagicTile = 4096;
void launch_magic_count(const uint8_t *bam, uint64_t len, uint32_t n_tiles, uint32_t *tile_cnt, hipStream_t stream);
void launch_magic_fill(const uint8_t *bam, uint64_t len, uint32_t n_tiles, const uint32_t *tile_base, uint64_t *cand, hipStream_t stream);
// next[i] = index of the candidate at cand[i] + BSIZE + 1, or n when the chain ends there; isize[i] = ISIZE footer
void launch_member_link(const uint8_t *bam, uint64_t len, const uint64_t *cand, uint32_t n, uint32_t *next, uint32_t *isize,
                        uint32_t *reach, uint64_t root2 /* second chain root: compressed offset of a seek target, ~0 = none */, hipStream_t stream);
void launch_member_jump(uint32_t n, const uint32_t *next_in, uint32_t *next_out, uint32_t *reach, hipStream_t stream);
// members[rank] for reachable candidates (rank = exclusive scan of reach); upos filled later by launch_member_upos
void launch_member_compact(const uint8_t *bam, uint64_t len, const uint64_t *cand, const uint32_t *isize, const uint32_t *reach, const uint32_t *rank,
                           uint32_t n, Member *members, uint32_t *isize_compact, hipStream_t stream);
// 64-bit exclusive scan of isize over the compacted members (single workgroup; n is ~1e5) -> Member::upos, total
void launch_member_upos(Member *members, const uint32_t *isize_compact, const uint32_t *n_members /*device*/, uint64_t *total, hipStream_t stream);
// answers host questions about the member list without copying it: q_coff[k] -> index of the member whose file offset is
// q_coff[k]-18+18 (exact match) or n; also the first index >= from[k] whose isize is 0 or > 65536 (stream stop rule)
void launch_member_query(const Member *members, const uint32_t *n_members /*device*/, const uint64_t *q_coff, uint32_t n_q, uint32_t *q_index,
                         uint64_t *q_upos, hipStream_t stream);
// *stop = min(*stop, first index >= *from whose ISIZE is 0 or > 65536)
// repair of files whose ISIZE footers do not say what the members inflate to (the reference never reads ISIZE, bgzf.c:292-316):
// launch_inflate_probe puts member m into slots + m * 64 KiB and its true length (~0 = does not inflate) into sizes[m];
// launch_member_fix makes those lengths the members' sizes before the offsets are scanned.
void launch_inflate_probe(const uint8_t *comp, const Member *members, uint32_t n_members, uint8_t *slots, uint32_t *len_scratch, uint32_t *sizes,
                          hipStream_t stream);
void launch_member_fix(Member *members, uint32_t *isize_compact, uint32_t max_members, const uint32_t *n_members /*device*/, const uint32_t *fix,
                       hipStream_t stream);
void launch_member_stop(const Member *members, uint32_t max_members, const uint32_t *n_members /*device*/, const uint32_t *from /*device*/, uint32_t *stop,
                        hipStream_t stream);

// ---- a2: record framing (records_kernels.hip) -------------------------------------------------------------
// Which bytes of the arena hold the record stream.  One chain (whole-file runs, shards): segment s covers arena [pos0 + s*kSegBytes,
// +kSegBytes) clipped to lim, and only segment 0 starts at an exact offset.  Region queries: ONE CHAIN PER CHUNK the reference's iterator
// reads (hts_itr_next, hts.c:1924-1965: a seek to the chunk's begin, then records as long as the position in front of the next one is
// below the chunk's end -- the first record after the seek is read whatever its position): chunk c owns segments [seg_base, next
// chunk's seg_base), its first segment starts exactly at a, its chain is followed up to b, and dlim is where the bytes a reader that
// started at a can get end (the next empty or unreadable member).  The chunk table lives in HBM; null = the one chain.
struct SegChunk { uint64_t a, b, dlim; uint32_t seg_base, pad; };
// REGTOOLS_AMD_DECODE="lane|wave[,seg_bytes]" (tests): long-record files through the workgroup-per-segment decode the lane form replaced, and either
// segment size (16384 / 131072) forced onto any file -- the extraction tests run the long-record path on short-read files with it.
struct DecodeKnobs { bool wave_form = false; int seg_bytes = 0; };
const DecodeKnobs &decode_knobs();
struct SegGeom {
    uint64_t pos0, lim;
    uint64_t data_end;             // end of the inflated bytes (k_decode_seg's staging window may reach past a chunk's end)
    const SegChunk *chunks; uint32_t n_chunks;
    uint32_t seg_bytes;            // kSegBytes, or kSegBytesLong for files of long records (the checkpoints and k_decode_seg only exist for kSegBytes)
    uint32_t lite_walk;            // round 4: the chain walk reads a record's block_size only (one request per record instead of seven dwords over
                                   // two lines); bam_read1's other acceptance tests (sam.c:421-423) are then made by the decode pass on the head it
                                   // reads anyway (ExtractCfg::insane_out), and a record that fails them sends the call through the full walk
};
constexpr uint32_t kSegBytesLong = 131072;     // a lane's first-record search reads, on average, half a record of sequence and quality: with records of
                                               // kilobytes (long reads) 16 KiB segments spend their time there (config 5: k_seg_walk 11.9 ms of a 47 ms tail)
constexpr uint32_t kLongRecordBytes = 2048;    // mean record size (estimated on the host from the file's first records) from which the long segments are used
// seg_start[s] = guessed (or, for a chain's first segment, exact) first record start >= segment begin; seg_exit[s] = first record
// start >= segment end reached by the chain from seg_start[s]; seg_cnt[s] = records that start inside the segment.
void launch_seg_walk(const uint8_t *arena, SegGeom g, uint32_t n_seg, int32_t n_ref,
                     uint64_t *seg_start, uint64_t *seg_exit, uint32_t *seg_cnt, uint16_t *seg_cp /* n_seg * kSegCpSlots */, hipStream_t stream,
                     uint32_t s_begin = 0 /* only segments [s_begin, n_seg): the guesses of a range can be made as soon as its bytes are inflated */);
// One verification sweep: segment s re-walks from seg_exit_in[s-1] when that differs from seg_start_in[s].
// *changed is incremented when anything changed. Reads *_in, writes *_out (all segments).
void launch_seg_verify(const uint8_t *arena, SegGeom g, uint32_t n_seg,
                       const uint64_t *seg_start_in, const uint64_t *seg_exit_in, const uint32_t *seg_cnt_in,
                       uint64_t *seg_start_out, uint64_t *seg_exit_out, uint32_t *seg_cnt_out,
                       uint32_t *status /* [0] leftmost disagreeing segment, [1] leftmost chain end; both preset to ~0u */, uint16_t *seg_cp, hipStream_t stream);
void launch_seg_truncate(SegGeom g, uint32_t n_seg, uint32_t last, uint64_t *seg_start, uint64_t *seg_exit, uint32_t *seg_cnt, hipStream_t stream);

// ---- a2/a3/a5/a6: SoA decode + per-read event count (records_kernels.hip) ----------------------------------
struct ReadSoA {
    int32_t  *tid, *pos;
    uint32_t *flag_nc;     // flag << 16 | n_cigar
    uint64_t *cig_off;     // arena offset of the CIGAR array
    uint8_t  *strand;      // per-read strand char from the tag (XS mode) or the flag rule (RF/FR)
    uint32_t *n_ev;        // junction events this read contributes (after region filter and junction_qc)
    uint64_t *rec_off;     // optional (may be null): arena offset of the record's block_size word (-b barcodes re-read the aux block)
};
// the reads the decode kernels marked (ExtractCfg::odd_count): out[3 k ..] = tid, pos, bam_endpos of the k-th found (any order); *count = how many (may exceed cap)
void launch_collect_odd_aux(const uint8_t *arena, ReadSoA soa, uint32_t n_rec, uint32_t cap, uint32_t *count, int32_t *out, hipStream_t stream);

// one wave per framing segment, segment bytes staged through LDS (replaces launch_seg_fill + launch_decode on the hot path)
// seg_iter[s] = records of segment s that pass the region filter; seg_long[s] = its reads for the wave-per-read kernel
void launch_decode_seg(const uint8_t *arena, SegGeom g, uint32_t n_seg, const uint64_t *seg_start, const uint32_t *seg_base,
                       const uint32_t *seg_cnt, ExtractCfg cfg, ReadSoA soa, uint32_t *seg_iter, uint32_t *seg_long, const uint16_t *seg_cp,
                       bool staged /* segment bytes through LDS (short records) or read in place (long records) */, hipStream_t stream,
                       uint32_t s_begin = 0 /* only segments [s_begin, n_seg): the early tail decodes the file's front part first */);
void launch_long_fill(uint32_t n_seg, const uint32_t *seg_base, const uint32_t *seg_cnt, const uint32_t *seg_long_base, ExtractCfg cfg, ReadSoA soa,
                      uint32_t *long_list, hipStream_t stream);

// ---- a4: CIGAR scan + junction emit (emit_kernels.hip) ------------------------------------------------------
struct EventSoA {
    uint32_t *tid, *start, *ilen_cls;   // key words: tid | start | (end-start) << 2 | strand class
    uint32_t *ts, *te;                  // thick_start / thick_end of this read's instance
    uint32_t *rpos, *rend;              // optional (may be null): the supporting read's pos / bam_endpos (window join of `identify`)
    uint8_t  *strand;
    uint32_t *read;                     // optional (may be null): index of the supporting read (-b barcodes)
};
void launch_emit_short(const uint8_t *arena, uint32_t n_rec, ExtractCfg cfg, ReadSoA soa, const uint32_t *ev_base,
                       EventSoA ev, hipStream_t stream, uint32_t row_begin = 0 /* rows [row_begin, n_rec) */,
                       const uint32_t *part_totals = nullptr, uint32_t n_parts = 0 /* device words added to every ev_base (early tail: ev_base counts per part) */,
                       uint32_t slot_cap = 0xffffffffu /* events at or behind this slot are counted, not written */);
void launch_emit_long(const uint8_t *arena, const uint32_t *long_list, uint32_t n_long,
                      ExtractCfg cfg, ReadSoA soa, const uint32_t *ev_base, EventSoA ev, hipStream_t stream);

// ---- primitives (prims_kernels.hip; the wave scans under them: wave_prims.h) ---------------------------------
// exclusive scan of n uint32 (out may alias in); *total (device) receives the sum. tmp needs scan_tmp_words(n) words.
size_t scan_tmp_words(uint32_t n);
void launch_scan_u32(const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *total, uint32_t *tmp, hipStream_t stream);

// One stable LSD radix pass on a permutation: digit(i) = (word[perm_in ? perm_in[i] : i] >> shift) & (2^bits-1), bits<=8.
size_t radix_tmp_words(uint32_t n);
void launch_radix_pass(const uint32_t *word, uint32_t shift, uint32_t bits, const uint32_t *perm_in, uint32_t *perm_out,
                       uint32_t n, uint32_t *tmp, hipStream_t stream);
// The same pass with the keys travelling along: position i's key is key_in[i] (streamed, no gather through the permutation), and
// key_out receives the keys in the new order.  perm_in null = identity.  A multi-pass sort on one word gathers that word once.
void launch_radix_pass_keyed(const uint32_t *key_in, uint32_t *key_out, uint32_t shift, uint32_t bits, const uint32_t *perm_in, uint32_t *perm_out,
                             uint32_t n, uint32_t *tmp, hipStream_t stream);

// ---- a7: segmented reduce, table writers (reduce_kernels.hip) ----------------------------------------------------
struct UniqueSoA {
    uint32_t *tid, *start, *end, *ts_min, *te_max, *count, *first_seen, *last_seen, *name_rank;
    uint8_t  *strand;
};
// Partial rows (round 4, k_preagg): one row per distinct key of a tile of consecutive events; reduce_events sorts and reduces these instead of the events.
struct PartialSoA { uint32_t *tid, *start, *ilen_cls, *ts, *te, *count, *first, *last; };
void launch_preagg(EventSoA ev, uint32_t n, PartialSoA p, uint32_t *p_total /* device, zeroed by the caller: rows appended */, hipStream_t stream);
// u.count / te_max / last_seen pre-filled with 0, u.ts_min / first_seen with 0xffffffff
void launch_reduce_partials(PartialSoA p, const uint32_t *perm, const uint32_t *head, const uint32_t *seg_excl, uint32_t n, UniqueSoA u, hipStream_t stream);
void launch_reduce_finish_partials(const uint8_t *ev_strand, uint32_t n_unique, UniqueSoA u, uint32_t *first_flag /* one word per EVENT, zeroed */, hipStream_t stream);
// head[i] = 1 where sorted position i starts a new key
void launch_heads(EventSoA ev, const uint32_t *perm, uint32_t n, uint32_t *head, hipStream_t stream);
// seg_excl = exclusive scan of head. ts_min must be pre-filled with 0xffffffff, te_max with 0.
void launch_reduce(EventSoA ev, const uint32_t *perm, const uint32_t *head, const uint32_t *seg_excl, uint32_t n, UniqueSoA u,
                   uint32_t *head_pos, hipStream_t stream);
// count / last_seen / strand per row; first_flag[first_seen[row]] = 1 (first_flag zeroed by the caller, n entries)
void launch_reduce_finish(EventSoA ev, const uint32_t *perm, uint32_t n, uint32_t n_unique, const uint32_t *head_pos, UniqueSoA u,
                          uint32_t *first_flag, hipStream_t stream);
// name_rank[row] = 1 + exclusive_scan(first_flag)[first_seen[row]]
void launch_name_rank(uint32_t n_unique, const uint32_t *flag_scan, UniqueSoA u, hipStream_t stream);
void launch_gather_u32(uint32_t n, const uint32_t *table, const uint32_t *idx, uint32_t *out, hipStream_t stream);
void launch_fill_u32(uint32_t *p, uint32_t v, size_t n, hipStream_t stream);
// p[i] = v for n elements of `width` bytes (1, 2, 4 or 8) at any alignment the width allows: the cohort runs' fill mode
void launch_fill_elems(void *p, uint32_t width, uint64_t v, size_t n, hipStream_t stream);
// ten u32 columns of n rows each, in `order`: tid,start,end,ts,te,count,name_rank,first_seen,last_seen,strand
void launch_rows_out(UniqueSoA u, const uint32_t *order, uint32_t n, uint32_t *out, hipStream_t stream);
// The result table's host block, written on the device so that ONE copy fills every column (api_ctx.cpp table_alloc): m = padded row count;
// u64 name_index[m], first_seen[m], last_seen[m]; u32 tid[m], start[m], end[m], thick_start[m], thick_end[m], read_count[m]; u8 strand[m], left_ok[m], right_ok[m]
RGX_HD size_t table_block_rows(uint64_t n) { return ((size_t)n + 1 + 15) & ~(size_t)15; }
RGX_HD size_t table_block_bytes(uint64_t n) { return table_block_rows(n) * (8 * 3 + 4 * 6 + 3); }
void launch_rows_table(UniqueSoA u, const uint32_t *order, uint32_t n, uint32_t min_anchor, uint8_t *out, hipStream_t stream);


// ---- -b: barcode counts per junction (junctions_extractor.cc:362-374, :204-217; barcode_kernels.hip) -------------------------------
// per event: where its read's barcode string lies in the arena (off = ~0 -> the literal "?"), the 64-bit grouping hash, the junction's output row
struct BarcodeEv { uint64_t *off; uint32_t *len, *h_lo, *h_hi, *row; };
// ev_urow[e] = unique row of event e (from the group-by's sorted order); must run before head / seg_excl are reused
void launch_event_urow(const uint32_t *sorted, const uint32_t *head, const uint32_t *seg_excl, uint32_t n, uint32_t *ev_urow, hipStream_t stream);
void launch_inverse_perm(const uint32_t *perm, uint32_t n, uint32_t *inv, hipStream_t stream);
// flags[0] = 1 when some read's tag is present but not a string
void launch_bc_event_keys(const uint8_t *arena, uint32_t n_events, const uint32_t *ev_read, const uint64_t *rec_off, const uint32_t *ev_urow,
                          const uint32_t *urow_pos, uint8_t t0, uint8_t t1, BarcodeEv b, uint32_t *flags, hipStream_t stream);
// head[i] = sorted position i starts a new (row, barcode); equal hashes with different bytes set flags[1]
void launch_bc_heads(const uint8_t *arena, BarcodeEv b, const uint32_t *perm, uint32_t n, uint32_t *head, uint32_t *flags, hipStream_t stream);
// one output row per head: pair_row, pair_first (earliest event), pair_pos (sorted position of the head), pair_off / pair_len (the string)
void launch_bc_pairs(BarcodeEv b, const uint32_t *perm, const uint32_t *head, const uint32_t *seg_excl, uint32_t n, uint32_t *pair_row,
                     uint32_t *pair_first, uint32_t *pair_pos, uint64_t *pair_off, uint32_t *pair_len, hipStream_t stream);
void launch_bc_counts(uint32_t n_pairs, uint32_t n, const uint32_t *pair_pos, uint32_t *pair_count, hipStream_t stream);
// text[str_begin[k] .. +pair_len[k]) = the k-th pair's barcode
void launch_bc_gather(const uint8_t *arena, uint32_t n_pairs, const uint64_t *pair_off, const uint32_t *pair_len, const uint32_t *str_begin,
                      uint8_t *text, hipStream_t stream);

// ---- a9-a11: `cis-splice-effects identify` interval kernels (cse_kernels.hip; logic in cse_core.h) --------------------------
struct GtfView;
struct VariantOpts;
}  // namespace rgx
#include "cse_core.h"
namespace rgx {
// count pass (fill = false): count[i], ces[i], cee[i]; fill pass: hit_tx[base[i]+k], hit_ad[2*(base[i]+k)] = annotation, +1 = distance
void launch_variant_scan(bool fill, GtfView g, uint32_t n, const int32_t *chrom, const uint32_t *pos0, VariantOpts o, uint32_t *count, const uint32_t *base,
                         uint32_t *ces, uint32_t *cee, uint32_t *hit_tx, uint32_t *hit_ad, unsigned long long *visits /* count pass: += exon records visited */,
                         hipStream_t stream, uint32_t *last_score = nullptr /* count pass: upstream's variant.score behind the walk (cse_core.h) */);
// count pass: count[i], flags[i] = known_donor | known_acceptor<<1 | known_junction<<2; fill pass: items (kind,a,b) in visitation order.
// form: 0 = one wave per junction, 1 = one lane per junction, -1 = the process's default (the wave form unless REGTOOLS_AMD_JSCAN=lane)
void launch_junction_scan(bool fill, GtfView g, uint32_t n, const int32_t *chrom, const uint32_t *js, const uint32_t *je, const uint8_t *strand, uint32_t *count,
                          const uint32_t *base, uint32_t *flags, uint32_t *item_kind, uint32_t *item_a, uint32_t *item_b, unsigned long long *visits,
                          uint32_t *visit_each /* wave form: exon records per junction */, hipStream_t stream, int form = -1);
void launch_max_span(EventSoA ev, uint32_t n, uint32_t *out /* zeroed by the caller */, hipStream_t stream);
constexpr uint32_t kWinSlices = 4;      // workgroups per variant window (k_window_pairs); count / base arrays hold n_win x kWinSlices entries
void launch_window_pairs(bool fill, EventSoA ev, uint32_t n_events, uint32_t n_win, const int32_t *w_tid, const int32_t *w_beg, const int32_t *w_end,
                         const uint32_t *max_span, uint32_t *w_lo, uint32_t *w_hi /* the windows' candidate ranges: written by the count pass (fill = false), read by the fill pass */,
                         uint32_t *count, const uint32_t *base, uint32_t *pair_ev, uint32_t *pair_win, hipStream_t stream);
// associate: (window, junction) pairs; junction arrays are bucketed by contig, chrom_off has n_chrom + 1 entries
void launch_assoc_pairs(bool fill, uint32_t n_win, const int32_t *w_chrom, const uint32_t *w_ces, const uint32_t *w_cee, const uint32_t *chrom_off,
                        const uint32_t *j_start, const uint32_t *j_end, uint32_t *count, const uint32_t *base, uint32_t *pair_j, uint32_t *pair_win, hipStream_t stream);
void launch_pair_gather(EventSoA ev, const uint32_t *pair_ev, const uint32_t *pair_win, uint32_t n, EventSoA out, hipStream_t stream);

// ---- multi-GPU table merge on the device (merge_kernels.hip) ----------------------------------------------------------------
struct MergeSoA { uint32_t *tid, *start, *end, *ts, *te, *count, *cls, *first, *shard; uint32_t *strand; };
struct MergeUnique { uint32_t *tid, *start, *end, *ts, *te, *count, *first, *last_shard, *strand; };
void launch_merge_unpack(const uint32_t *rows, uint32_t stride_rows, uint32_t n_parts, const uint32_t *part_rows, const uint32_t *part_base, MergeSoA m, hipStream_t st);
void launch_cols_to_packed(const uint32_t *cols /* launch_rows_out block */, uint32_t n, uint32_t *out, hipStream_t st);
void launch_merge_heads(MergeSoA m, const uint32_t *sorted, uint32_t n, uint32_t *head, hipStream_t st);
void launch_merge_reduce(MergeSoA m, const uint32_t *sorted, const uint32_t *head, const uint32_t *seg_excl, uint32_t n, MergeUnique u /* ts preset to ~0, rest 0 */, hipStream_t st);
void launch_merge_rank(const uint32_t *by_first, uint32_t n, uint32_t *name_rank, hipStream_t st);
void launch_merge_pack(MergeUnique u, const uint32_t *order, const uint32_t *name_rank, uint32_t n, uint32_t *out, hipStream_t st);
// the merged rows in the result table's host block layout (see launch_rows_table)
void launch_merge_table(MergeUnique u, const uint32_t *order, const uint32_t *name_rank, uint32_t n, uint32_t min_anchor, uint8_t *out, hipStream_t st);

// ---- cohort junction-by-sample matrix (cohort_kernels.hip; host side in cohort.cpp) ---------------------------------------------------------
// The accumulator: blocks of kCohortBlockRows triples, seven u32 columns each (cohort tid, start, end, thick_start, thick_end, read_count,
// strand char << 24 | sample index); triple k lies in block k >> kCohortBlockLog2.  `blocks` is the device table of the blocks' addresses.
constexpr uint32_t kCohortBlockLog2 = 22, kCohortBlockRows = 1u << kCohortBlockLog2, kCohortColumns = 7;
struct CohortSorted { uint32_t *tid, *start, *end, *ts, *te, *count, *ss; };                    // the triples in key order, n entries each
struct CohortRows { uint32_t *ts, *te, *keep, *kept_nnz; unsigned long long *total; };           // one entry per distinct key
// the finished matrix as it lies in the host block (cohort.cpp MatrixLayout): written on the device, copied once
struct CohortImage { unsigned long long *total, *row_begin; uint32_t *tid, *start, *end, *ts, *te, *n_with, *col_sample, *val_count; uint8_t *strand; };
// src: u32 columns `stride` words apart, strand at column strand_col; *fill = triples accumulated so far (one atomicAdd per wave); cap = rows the blocks hold
void launch_cohort_append(const uint32_t *src, uint32_t n, size_t stride, uint32_t strand_col, const uint32_t *tid_map, uint32_t n_map, uint32_t min_anchor,
                          bool only_anchored, uint32_t sample, uint32_t *fill, uint32_t cap, uint32_t *const *blocks, hipStream_t st);
// out[i] = key word `which` (0 tid, 1 start, 2 end, 3 strand class) of triple perm[i] (null = i)
void launch_cohort_key(uint32_t *const *blocks, const uint32_t *perm, uint32_t n, uint32_t which, uint32_t *out, hipStream_t st);
// the triples in the order of perm, and head[i] = 1 where position i starts a new key
void launch_cohort_gather(uint32_t *const *blocks, const uint32_t *perm, uint32_t n, CohortSorted s, uint32_t *head, hipStream_t st);
void launch_cohort_row_start(const uint32_t *head, const uint32_t *seg_excl, uint32_t n, uint32_t *row_start /* rows + 1 */, hipStream_t st);
void launch_cohort_reduce(CohortSorted s, const uint32_t *row_start, uint32_t n, uint32_t n_rows, uint32_t min_samples, uint64_t min_total, CohortRows r,
                          hipStream_t st);
// out_row / nnz_excl = exclusive scans of r.keep / r.kept_nnz
void launch_cohort_out(CohortSorted s, const uint32_t *head, const uint32_t *seg_excl, const uint32_t *row_start, CohortRows r, const uint32_t *out_row,
                       const uint32_t *nnz_excl, uint32_t n, uint32_t n_rows, uint32_t n_nnz_kept, CohortImage o, hipStream_t st);

// ---- intron clusters of a cohort matrix (cluster_kernels.hip; host side in cohort_cluster.cpp) -------------------------------------------------
void launch_cluster_class(const uint8_t *strand, uint32_t n, uint32_t *cls /* '+' 0, '-' 1, else 2 */, hipStream_t st);
// perm = the rows in stable order of (tid, cls, site): (ea[i], eb[i]) = (perm[i - 1], perm[i]) where both lie on one site, a self loop otherwise
void launch_cluster_edges(const uint32_t *perm, const uint32_t *tid, const uint32_t *cls, const uint32_t *site, uint32_t n, uint32_t *ea, uint32_t *eb,
                          hipStream_t st);
// The component search, a launch per step (components_run, cohort_cluster.cpp): parent[v] = v; hook the larger label of an edge's ends under
// the smaller (atomicMin; ends at or above n_vertices are skipped); parent[v] = parent[parent[parent[v]]].  *flag |= 1 when a step changed a label.
void launch_cc_init(uint32_t *parent, uint32_t n, hipStream_t st);
void launch_cc_hook(uint32_t *parent, const uint32_t *a, const uint32_t *b, uint32_t n_edges, uint32_t n_vertices, uint32_t *flag, hipStream_t st);
void launch_cc_jump(uint32_t *parent, uint32_t n, uint32_t *flag, hipStream_t st);
// cnt[root] / tot[root] += 1 / total[i] (both zeroed by the caller); is_root, keep = root that passes the filters
void launch_cluster_tally(const uint32_t *label, const unsigned long long *total, uint32_t n, uint32_t *cnt, unsigned long long *tot, hipStream_t st);
void launch_cluster_roots(const uint32_t *label, const uint32_t *cnt, const unsigned long long *tot, uint32_t n, uint32_t min_rows, uint64_t min_total,
                          uint32_t *is_root, uint32_t *keep, hipStream_t st);
// cid_excl = exclusive scan of keep: cluster[i] (0xffffffff = dropped), sort_key[i] (dropped rows: n_clusters), and per kept cluster its rows and total
void launch_cluster_assign(const uint32_t *label, const uint32_t *keep, const uint32_t *cid_excl, const uint32_t *cnt, const unsigned long long *tot,
                           uint32_t n, uint32_t n_clusters, uint32_t *cluster, uint32_t *sort_key, uint32_t *cl_count, unsigned long long *cl_total,
                           hipStream_t st);
// out[k] = in[k] for k < n, out[n] = *last (device)
void launch_cluster_widen(const uint32_t *in, uint32_t n, const uint32_t *last, unsigned long long *out /* n + 1 */, hipStream_t st);
// the count entries of clustered rows that are not zero: len[row], then (cluster, sample, count) from ent_off[row] = exclusive scan of len on
void launch_cluster_row_len(const uint32_t *cluster, const unsigned long long *row_begin, const uint32_t *val, uint32_t n, bool wave_per_row, uint32_t *len,
                            hipStream_t st);
void launch_cluster_expand(const uint32_t *cluster, const unsigned long long *row_begin, const uint32_t *col, const uint32_t *val, const uint32_t *ent_off,
                           uint32_t n, bool wave_per_row, uint32_t *e_cluster, uint32_t *e_sample, uint32_t *e_count, hipStream_t st);
// perm = the n entries in stable order of (cluster, sample): head flags, then one sum per run (seg_start as launch_cohort_row_start leaves it)
void launch_cluster_cs_heads(const uint32_t *perm, const uint32_t *e_cluster, const uint32_t *e_sample, uint32_t n, uint32_t *head, hipStream_t st);
void launch_cluster_cs_sum(const uint32_t *perm, const uint32_t *e_cluster, const uint32_t *e_sample, const uint32_t *e_count, const uint32_t *seg_start,
                           uint32_t n, uint32_t n_seg, uint32_t *seg_cluster, uint32_t *cs_sample, unsigned long long *cs_total, hipStream_t st);
void launch_cluster_cs_begin(const uint32_t *seg_cluster, uint32_t n_seg, uint32_t n_clusters, unsigned long long *cs_begin /* n_clusters + 1 */, hipStream_t st);
// Refinement (rgx_cohort_refine): alive[i] = 1 while row i takes part.  eligible: end - start <= max_intron (0: every row).  compact: out = the
// entries of order[0 .. k) whose row is alive, in order (stable: a sorted order stays sorted); pos = k words of scratch, *n_live (device) = how
// many; out holds up to k words.  edges: launch_cluster_edges over the first *n_live (device) entries of perm, self loops in the slots up to cap.
// tally / roots: their cluster namesakes over the alive rows only (cnt may be null in tally).  mark: an alive row whose total is below min_reads,
// or for which total * ratio_den < ratio_num * tot[label] on the whole products, stops being alive.
void launch_refine_eligible(const uint32_t *start, const uint32_t *end, uint32_t n, uint32_t max_intron, uint32_t *alive, hipStream_t st);
void launch_refine_compact(const uint32_t *order, uint32_t k, const uint32_t *alive, uint32_t *pos, uint32_t *out, uint32_t *n_live, uint32_t *tmp,
                           hipStream_t st);
void launch_refine_edges(const uint32_t *perm, const uint32_t *n_live, const uint32_t *tid, const uint32_t *cls, const uint32_t *site, uint32_t cap,
                         uint32_t *ea, uint32_t *eb, hipStream_t st);
void launch_refine_tally(const uint32_t *label, const unsigned long long *total, const uint32_t *alive, uint32_t n, uint32_t *cnt,
                         unsigned long long *tot, hipStream_t st);
void launch_refine_mark(const uint32_t *label, const unsigned long long *total, const unsigned long long *tot, uint32_t n, uint64_t min_reads,
                        uint32_t ratio_num, uint32_t ratio_den, uint32_t *alive, hipStream_t st);
void launch_refine_roots(const uint32_t *label, const uint32_t *cnt, const unsigned long long *tot, const uint32_t *alive, uint32_t n, uint32_t min_rows,
                         uint64_t min_total, uint32_t *is_root, uint32_t *keep, hipStream_t st);

// ---- the cohort's splicing phenotype table (pheno_kernels.hip; host side in cohort_pheno.cpp; per-entry arithmetic in pheno_core.h) ----------------
// what the kernels read: the matrix's CSR image and, of its cluster result, the rows' clusters and the denominators
struct PhenoIn { const uint32_t *cluster; const unsigned long long *row_begin; const uint32_t *col_sample, *val_count;
                 const unsigned long long *cs_begin; const uint32_t *cs_sample; const unsigned long long *cs_total; };
// per matrix row: missing samples, mean, sd (rows with a cluster only), keep = clustered and past both filters, drop_na = clustered and dropped as missing
void launch_pheno_row_stats(PhenoIn in, uint32_t n, uint32_t n_samples, uint32_t na_num, uint32_t na_den, double min_sd, uint32_t *n_na, double *mean,
                            double *sd, uint32_t *keep, uint32_t *drop_na, hipStream_t st);
// pos = exclusive scan of keep: the kept rows' statistics side by side, in matrix order
void launch_pheno_scatter(const uint32_t *keep, const uint32_t *pos, const uint32_t *n_na, const double *mean, const double *sd, uint32_t n,
                          uint32_t *o_row, uint32_t *o_n_na, double *o_mean, double *o_sd, hipStream_t st);
// entry k * n_samples + s: the order-preserving 64-bit key of its z as two words, and s; n_kept * n_samples below 2^32 - 2^16
void launch_pheno_z(PhenoIn in, const uint32_t *o_row, const double *o_mean, const double *o_sd, uint32_t n_kept, uint32_t n_samples, uint32_t *z_lo,
                    uint32_t *z_hi, uint32_t *e_sample, hipStream_t st);
// perm = the n = n_kept * n_samples entries in stable order of (sample, z): head flags of the runs of equal z inside a column, then -- behind a scan
// and launch_cohort_row_start -- rank2[entry] = first + last 1-based place of its run in its column
void launch_pheno_tie_heads(const uint32_t *perm, const uint32_t *z_lo, const uint32_t *z_hi, uint32_t n, uint32_t n_kept, uint32_t *head,
                            hipStream_t st);
void launch_pheno_rank(const uint32_t *perm, const uint32_t *head, const uint32_t *seg_excl, const uint32_t *run_start, uint32_t n, uint32_t n_kept,
                       uint32_t *rank2, hipStream_t st);

// ---- the phenotype table's principal components (pca_kernels.hip; host side in cohort_pcs.cpp; arithmetic in pca_core.h) ---------------------------
// With n_tiles = ceil(S / 64) and n_chunks = pca_n_chunks(K): part takes n_tiles (n_tiles + 1) / 2 * n_chunks tiles of 64 x 64 doubles, col_part
// n_chunks * n_tiles * 64 doubles; T has the 2 K - 1 quantiles of rank2 = 2 .. 2 K; *bad (zeroed by the caller) becomes 1 when a rank2 is outside that
void launch_pca_gram(const uint32_t *rank2, const double *T, uint64_t K, uint32_t S, double *part, double *col_part, uint32_t *bad, hipStream_t st);
// gram (S x S, both triangles) and col_sum (S): the chunk partials in ascending chunk order
void launch_pca_reduce(const double *part, const double *col_part, uint64_t K, uint32_t S, double *gram, double *col_sum, hipStream_t st);

// ---- the cohort's nominal cis-sQTL scan (qtl_kernels.hip; host side in cohort_qtl.cpp; arithmetic in qtl_core.h) ------------------------------------
// Residuals against the C unit vectors of Q (C x S), row-major: Y (K x S) with yy, G (V x S) with gg, the verdicts and the usable flags.  flag: two
// words (qtl_core.h), zeroed by the caller
void launch_qtl_residual_pheno(const uint32_t *rank2, const double *T, uint32_t K, uint32_t S, const double *Q, uint32_t C, double *Y, double *yy,
                               uint32_t *flag, hipStream_t st);
void launch_qtl_residual_geno(const int8_t *dosage, uint32_t V, uint32_t S, const double *Q, uint32_t C, double *G, double *gg, uint8_t *verdict,
                              uint32_t *usable, uint32_t *flag, hipStream_t st);
// place = exclusive scan of usable: the usable variants side by side
void launch_qtl_compact(const uint32_t *usable, const uint32_t *place, uint32_t V, const uint32_t *var_tid, const uint32_t *var_pos, const double *gg,
                        uint32_t *u_var, uint64_t *u_key, double *u_gg, hipStream_t st);
// dst[s * ld + i] = src[(idx ? idx[i] : i) * S + s] for i < (n ? *n : n_fixed), +0.0 behind that up to ld
void launch_qtl_transpose(const double *src, const uint32_t *idx, const uint32_t *n, uint32_t n_fixed, uint32_t S, size_t ld, double *dst,
                          hipStream_t st);
// lo and count (K + 1 words, the last 0) per row, blk_lo and tile_count (ceil(K / 64) + 1 words, the last 0) per block of 64 rows, and
// totals = {the sum of count, the sum of tile_count}
void launch_qtl_plan(const uint32_t *regions, uint32_t K, uint32_t S, const double *yy, const uint64_t *u_key, const uint32_t *n_usable,
                     uint32_t window, uint32_t *lo, uint32_t *count, uint32_t *blk_lo, uint32_t *tile_count, unsigned long long *totals,
                     hipStream_t st);
// Yt: ldy a multiple of 64 at or above K; Gt: ldg at or above the usable variants + 63; both zero behind their last column
void launch_qtl_pairs(const double *Yt, size_t ldy, const double *Gt, size_t ldg, uint32_t S, uint32_t K, uint32_t n_tiles, const uint32_t *tile_begin,
                      const uint32_t *blk_lo, const uint32_t *lo, const uint32_t *count, const uint32_t *pair_begin, const double *yy,
                      const double *u_gg, const uint32_t *u_var, double *r, double *slope, uint32_t *pair_variant, hipStream_t st);
void launch_qtl_best(const double *r, const uint32_t *pair_begin, uint32_t K, uint32_t *best, hipStream_t st);

// ---- the cis-sQTL permutation pass, ungrouped and grouped (qtl_perm_kernels.hip; host side in cohort_qtl_perm.cpp) ------------------------------
// perm_r (n_series x n_perm1) = per series and permutation the largest |r| over all members' cis variants; best_row and best_u (n_series) =
// permutation 0's table row and usable variant (all ones: none).  grp_begin (n_series + 1) and grp_row: the series' member rows, ascending inside
// a series; a null grp_begin: series g is table row g alone, grp_row is not read and best_row may be null.  Y: the row-major residuals; permT: S
// rows of ldp uint16, ldp a multiple of 64 at or above n_perm1, index 0 behind it; Gt as for the pairs.  n_series * (ldp / 64) workgroups: the
// caller keeps that inside 2^31 - 1
void launch_qtl_perm(const double *Y, uint32_t n_series, uint32_t S, const uint16_t *permT, size_t ldp, uint32_t n_perm1, const double *Gt,
                     size_t ldg, const uint32_t *lo, const uint32_t *count, const double *yy, const double *u_gg, const uint32_t *grp_begin,
                     const uint32_t *grp_row, double *perm_r, uint32_t *best_row, uint32_t *best_u, hipStream_t st);
// the winning pair's chain again, a thread per series: the input variant (RGX_NO_PAIR: none), r and slope; a null best_row: series g is row g
void launch_qtl_perm_best(const double *Y, const double *G, uint32_t n_series, uint32_t S, const uint32_t *best_row, const uint32_t *best_u,
                          const uint32_t *u_var, const double *yy, const double *gg, uint32_t *best_variant, double *best_r, double *best_slope,
                          hipStream_t st);

// ---- the conditional cis-sQTL permutation pass (qtl_cond_kernels.hip; host side in cohort_qtl_cond.cpp) -------------------------------------------
// What its kernels share.  N series: series_row (N), cond_begin (N + 1) and cond_variant, input variants; lo, count and u_var: the plan's; pb
// (N + 1): the exclusive scan of count[series_row[c]], a series' places.  z: N x 8 x S unit vectors; yc (N x S), yyc and status per series; beta: 8
// planes of cap doubles and ggc: cap doubles, per place; cap: at or above pb[N].
struct QtlCond {
    uint32_t N, S; const uint32_t *series_row, *cond_begin, *cond_variant, *lo, *count, *u_var, *pb;
    double *z, *yc, *yyc, *beta, *ggc; uint8_t *status; size_t cap;
};
// cnt (N + 1 words, the last 0) = count[series_row[c]]
void launch_qtl_cond_counts(const QtlCond &q, uint32_t *cnt, hipStream_t st);
// z, yc, yyc and status per series, then beta and ggc per place.  Y, G: the row-major residuals; flag: one word, zeroed by the caller, raised for a
// conditioning variant whose verdict is not 0
void launch_qtl_cond_prepare(const QtlCond &q, const double *Y, const double *G, const uint8_t *verdict, uint32_t *flag, hipStream_t st);
// perm_r (N x n_perm1) and best_u (N; all ones: none) as launch_qtl_perm writes them, over the places whose ggc is enough
void launch_qtl_perm_cond(const QtlCond &q, const uint16_t *permT, size_t ldp, uint32_t n_perm1, const double *Gt, size_t ldg, double *perm_r,
                          uint32_t *best_u, hipStream_t st);
// the winning pair's chain and correction again; n_cis: the places that take part; n_window: count[series_row[c]]
void launch_qtl_cond_best(const QtlCond &q, const double *G, const uint32_t *best_u, uint32_t *best_variant, double *best_r, double *best_slope,
                          uint32_t *n_cis, uint32_t *n_window, hipStream_t st);

// ---- the trans-sQTL scan (qtl_trans_kernels.hip; host side in cohort_qtl_trans.cpp) -----------------------------------------------------------------
// What both product kernels read: the sample-major panels of launch_qtl_pairs, n_blocks x n_vt tiles of 64 rows x 64 usable variants (tile =
// row block * n_vt + variant tile), the rows' regions (3 words each) and yy, the usable variants' keys and gg, their number on the device, and
// the test: bits(|r|) >= r_min_bits, and with exclude_cis no pair inside exclude_window
struct QtlTransTiles {
    const double *Yt; size_t ldy; const double *Gt; size_t ldg; uint32_t S, K, n_blocks, n_vt;
    const uint32_t *regions; const double *yy, *u_gg; const uint64_t *u_key; const uint32_t *n_usable;
    uint64_t r_min_bits; uint32_t exclude_cis, exclude_window;
};
// per tile its hits, the pairs that met and hits != 0 as a word for the scan; tiles behind the last usable variant get zeros.  band: the row
// blocks of a super-tile in the tile-to-workgroup mapping (speed alone; 0: workgroup b runs tile b)
void launch_qtl_trans_count(const QtlTransTiles &t, uint32_t band, uint32_t *tile_hits, uint32_t *tile_tested, uint32_t *tile_flag, hipStream_t st);
// out[0] = H and out[1] = the pairs that met as 64-bit sums, out[2] = *n_hit_tiles, out[3] = the two flag words, out[4] = *n_usable
void launch_qtl_trans_totals(const uint32_t *tile_hits, const uint32_t *tile_tested, uint32_t n_tiles, const uint32_t *n_hit_tiles,
                             const uint32_t *flag, const uint32_t *n_usable, unsigned long long *out, hipStream_t st);
// hit_tile[place[t]] = t for the tiles with tile_flag[t]
void launch_qtl_trans_hit_tiles(const uint32_t *tile_flag, const uint32_t *place, uint32_t n_tiles, uint32_t *hit_tile, hipStream_t st);
// one workgroup per listed tile: its hits at tile_off[tile] + their rank inside the tile (rows, then variants): row, usable variant, r, slope
void launch_qtl_trans_emit(const QtlTransTiles &t, const uint32_t *hit_tile, uint32_t n_hit_tiles, const uint32_t *tile_off, uint32_t *hit_row,
                           uint32_t *hit_u, double *hit_r, double *hit_slope, hipStream_t st);
// the hits in the order perm (null: as they are): their rows, input variants, r and slope; then hit_begin[k] = the first hit of a row >= k, k <= K
void launch_qtl_trans_order(const uint32_t *perm, uint32_t H, const uint32_t *hit_row, const uint32_t *hit_u, const double *hit_r,
                            const double *hit_slope, const uint32_t *u_var, uint32_t K, uint32_t *row_sorted, uint32_t *hit_variant, double *r,
                            double *slope, uint32_t *hit_begin, hipStream_t st);

}  // namespace rgx
