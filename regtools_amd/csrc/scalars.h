// scalars.h -- the per-call scalar block: c->buf(Buf::scalars) in HBM (512 bytes) and its mirror at the start of the page-locked c->pinned (4 KiB).  Kernels
// leave totals, verdicts and flags here; the host reads them back member by member (fetch_scalar).  stage_upload clears the whole block and presets the
// four members marked "preset ~0".  Members read back by ONE copy form one nested struct, so that they cannot drift apart.
#pragma once
#include <stddef.h>
#include "kernels.h"
struct InflateStatus { uint32_t first_bad, code; };    // launch_inflate's `status`: the first member that did not inflate (~0 = none), its status
struct Scalars {
    InflateStatus inflate;              // the call's range launch(es); preset ~0
    uint32_t spare2, n_rec;             // n_rec: record total of the framing's segment scan
    struct Counts {                     // stage_decode's totals (one copy); n_unique / n_partial: reduce_events' distinct keys / the rows k_preagg left
        uint32_t n_events, n_long, n_unique, n_partial, n_iterated, spare9;
    } counts;
    struct Framing { uint32_t disagree, chain_end; } framing;      // leftmost disagreeing segment, leftmost chain end (~0 = none); set per sweep
    // the header's own inflate, when the range does not start at the file's head; preset ~0.  launch_inflate gets no ignore_below here (default
    // 0), so the early pair kStatusEarly words behind this member -- part_events[4..5] -- is never written.
    InflateStatus hdr_inflate;
    uint32_t spare14[2], n_cand, n_members;     // BGZF magic candidates; members
    uint32_t stop, spare19;             // first empty / oversized member at or behind the first one read; preset ~0
    uint64_t total_inflated;
    uint32_t spare22[2], q_index[3], spare27[5];        // member index of {seek target, lower cut, upper cut} (n_members = no such member)
    uint64_t q_upos[3], spare38, q_coff[3];             // ... its offset in the inflated stream; the compressed offsets asked for
    uint32_t spare46[14], variant_hits, junction_items, max_span, window_pairs;    // identify / associate (cse_api.cpp)
    unsigned long long variant_visits, junction_visits;                            // exon visits of the two interval scans
    uint32_t assoc_pairs, fa_missing;   // fa_missing (emit): 1 + tid of a contig the FASTA lacks (0 = none)
    uint32_t merge_unique, spare71;     // rgx_table_merge_device: distinct keys
    struct Barcodes { uint32_t not_string, hash_clash, n_pairs; } barcodes;        // barcode_rows: two error flags and the (row, barcode) total, one copy
    uint32_t barcode_text_len;
    InflateStatus inflate_early; uint32_t spare78[2];      // `inflate` for the members below ignore_below (in front of a seek target); preset ~0
    struct Stop { uint32_t index, last_pass; } stop_rule;          // region iteration: the record that ends it (~0 = none), the last one that passed
    uint32_t insane, wait_timed_out;    // lite walk: a record bam_read1 would refuse lies on the chain; early tail: launch_wait_done gave up
    uint32_t part_events[rgx::kGateParts];      // early tail: event total of each emitted part
    uint64_t exit_staging, spare94;     // host mirror only: a segment's exit offset on its way back
    uint32_t abort_row;                 // first record the reference abort()s on (~0 = none)
    uint32_t odd_aux, spare98[2];       // identify: reads whose strand tag lies behind an aux field of unknown type
    // verdicts of the arena placement trials, looked at by nobody.  They pass ignore_below = 0 (the early pair would lie outside the block).
    InflateStatus trial_inflate; uint32_t spare102[26];
};
static_assert(sizeof(Scalars) == 512, "the scalar block is 512 bytes of HBM, inside the 4 KiB of pinned staging");
static_assert(offsetof(Scalars, inflate_early) - offsetof(Scalars, inflate) == rgx::kStatusEarly * 4, "k_inflate_* write status + kStatusEarly");
// two read-backs take the block's front whole: the header's (both inflate verdicts) and the member query's (everything in front of identify's visits)
constexpr size_t kScalarsHeaderPart = offsetof(Scalars, n_cand), kScalarsQueryPart = offsetof(Scalars, variant_visits);
static_assert(kScalarsHeaderPart == 64 && kScalarsQueryPart == 256, "the front read-backs keep their sizes");

// one member (or nested struct) of the host mirror, named through the mirror, fetched from its place in the device block
template <class T> inline hipError_t fetch_scalar(const Scalars *d_sc, Scalars *h_sc, T &host_member, hipStream_t st) {
    return hipMemcpyAsync(&host_member, (const char *)d_sc + ((const char *)&host_member - (const char *)h_sc), sizeof(T), hipMemcpyDeviceToHost, st);
}
