// call_path.h -- on which path an attempt of an extract call's front runs (EventsRun, api_internal.h), and where the call goes when a stage says "start over":
// the one decision behind every fallback of a damaged file.  No HIP, no context: tests/hostemu builds it with plain g++ (tests/test_call_path_host.py).
#pragma once

namespace rgx {

// The flags an attempt runs under: all clear at a call's start but what its input says (first_path).
struct CallPath {
    bool device_resident = false;   // the file's bytes lie in HBM: no host bytes, no overlapped upload, the device's own member discovery
    bool own_scan = false;          // the caller's shared member list (SharedMembers) is not used
    bool true_sizes = false;        // the members' lengths come from the probe (the context's "probe_sizes" block), not from the footers
    bool to_file_end = false;       // a region query inflates everything up to the end of the file, not the members the index asked for
    bool strict_walk = false;       // the framing walk makes bam_read1's full test of every record, not the block_size-only one
};
inline CallPath first_path(bool device_bytes, bool shared_list) { CallPath p; p.device_resident = device_bytes; p.own_scan = !shared_list; return p; }

// Why a stage starts the call over, in the order the stages can ask; restart_name says it in an error text.
enum class Restart {
    index_points_at_no_member,      // 1 stage_members: the host scan's list, and the index's start is no member of it
    shard_range_uncovered,          // 2 stage_range_and_inflate: a shard's uploaded byte range does not hold its members
    footers_lie,                    // 3 stage_footers_and_header: a member is not as long as its footer says (the probe has run)
    verdict_not_clean,              // 4 frame(): the speculative launch's verdict, read with the first framing's counts
    verdict_not_clean_unframed,     // 5 stage_framing: the same verdict when there was nothing to frame
    region_chain_ended,             // 6 stage_framing: a region chunk's record chain ended inside the members the index asked for
    record_fails_full_test,         // 7 stage_decode: the lite walk followed a record bam_read1 refuses
};
inline const char *restart_name(Restart why) {
    static const char *const names[] = {"the index points at no member", "a shard's range does not cover its members", "footers lie",
        "inflate verdict not clean", "inflate verdict not clean, nothing framed", "a region's chain ended", "a record fails bam_read1's test"};
    return names[(int)why];
}

// The path of the next attempt.  Reasons 2 and 3 keep their input (3 drops the list too: with true sizes nothing overlaps, so none is read); every other
// reason makes the next attempt device-resident: its input is this attempt's file buffer in HBM, whole (EventsRun::quiesce).
// Termination: there are five flags and no reason clears one.  Each reason sets a flag that its own condition needs clear -- device_resident for 1, 4
// and 5 (only the overlapped upload of host bytes asks), own_scan for 2, true_sizes for 3, to_file_end for 6, strict_walk for 7 -- and false comes back
// when it is set already.  So a call has at most five restarts, six attempts.
inline bool next_path(CallPath cur, Restart why, CallPath &next) {
    const bool keeps_input = why == Restart::shard_range_uncovered || why == Restart::footers_lie;
    bool CallPath::*const sets = why == Restart::shard_range_uncovered ? &CallPath::own_scan : why == Restart::footers_lie ? &CallPath::true_sizes :
        why == Restart::region_chain_ended ? &CallPath::to_file_end : why == Restart::record_fails_full_test ? &CallPath::strict_walk :
        &CallPath::device_resident;
    if (cur.*sets) return false;
    next = cur;
    next.*sets = next.own_scan = true;                           // (no attempt behind a restart reads the caller's list)
    if (!keeps_input) next.device_resident = true;
    return true;
}

}  // namespace rgx
