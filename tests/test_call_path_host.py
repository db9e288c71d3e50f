"""No GPU: where an extract call goes when a stage says "start over" (regtools_amd/csrc/call_path.h, built into tests/hostemu with plain g++).  The
table of the seven reasons is written out here as literal flag sets, and every sequence of restarts a call could make is followed to its end: the guard
this proves (next_path says no to a reason whose flag is set already) is what keeps a wrong path from repeating work on a device."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, O, T, E, S = 1, 2, 4, 8, 16          # device_resident, own_scan, true_sizes, to_file_end, strict_walk
(INDEX_NO_MEMBER, SHARD_UNCOVERED, FOOTERS_LIE, VERDICT, VERDICT_UNFRAMED, CHAIN_ENDED, FULL_TEST) = range(1, 8)
REASONS = range(1, 8)
SETS = {INDEX_NO_MEMBER: D, SHARD_UNCOVERED: O, FOOTERS_LIE: T, VERDICT: D, VERDICT_UNFRAMED: D, CHAIN_ENDED: E, FULL_TEST: S}


@pytest.fixture(scope="module")
def emu(built):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostemu", "libhostemu.so"))
    lib.emu_call_first_path.restype, lib.emu_call_first_path.argtypes = C.c_uint, [C.c_int, C.c_int]
    lib.emu_call_next_path.restype, lib.emu_call_next_path.argtypes = C.c_int, [C.c_uint, C.c_int, C.POINTER(C.c_uint)]
    lib.emu_call_restart_name.restype, lib.emu_call_restart_name.argtypes = C.c_char_p, [C.c_int]
    return lib


def next_path(emu, cur, why):
    out = C.c_uint(0)
    return out.value if emu.emu_call_next_path(cur, why, C.byref(out)) else None


def can_ask(cur, why):
    """whether the stage's own condition can hold on this path: the overlapped upload of host bytes (and with it the host scan's list, a shard's
    byte range, the speculative launch) needs host input and footers' sizes; a shard's range also the caller's list; the rest the flag they set clear.
    A model written here of the tests in front of each `return restart(...)` (api_front.cpp stage_members: `overlap`; stage_range_and_inflate: `overlap`
    and a partial upload, which only a shared list gives; api_records.cpp stage_footers_and_header: `!d_true_sizes`; frame() and stage_framing: `spec`,
    which needs `overlap`; stage_framing: `!path.to_file_end`; stage_decode: `cfg.insane_out`, set on the lite walk only) -- `overlap` itself is
    stage_upload's `!d_bam` (host input) `&& !d_true_sizes`.  The note at EventsRun::restart points back here."""
    if why in (INDEX_NO_MEMBER, VERDICT, VERDICT_UNFRAMED):
        return not cur & (D | T)
    if why == SHARD_UNCOVERED:
        return not cur & (D | T | O)
    return not cur & SETS[why]


FIRST = {"host bytes": O, "host bytes, shared list": 0, "device bytes": D | O}


def test_first_paths(emu):
    assert emu.emu_call_first_path(0, 0) == FIRST["host bytes"]
    assert emu.emu_call_first_path(0, 1) == FIRST["host bytes, shared list"]
    assert emu.emu_call_first_path(1, 0) == FIRST["device bytes"]
    assert emu.emu_call_first_path(1, 1) == D                  # (no entry caller does this; a device-resident attempt reads no list)


TABLE = [
    # (reason, from, expected): what the old recursive call at each of the seven sites handed to the inner call
    (INDEX_NO_MEMBER, O, D | O), (INDEX_NO_MEMBER, 0, D | O),               # device bytes, no list, footers' sizes, to_file_end as it was
    (SHARD_UNCOVERED, 0, O),                                               # the same input, the list dropped
    (FOOTERS_LIE, O, O | T), (FOOTERS_LIE, 0, O | T), (FOOTERS_LIE, D | O, D | O | T),          # the same input, the probe's sizes, the list dropped
    (VERDICT, O, D | O), (VERDICT, 0, D | O), (VERDICT_UNFRAMED, O, D | O), (VERDICT_UNFRAMED, 0, D | O),
    (CHAIN_ENDED, O, D | O | E), (CHAIN_ENDED, D | O, D | O | E), (CHAIN_ENDED, 0, D | O | E), (CHAIN_ENDED, D | O | T, D | O | T | E),
    (CHAIN_ENDED, D | O | S, D | O | S | E),                               # sizes and strictness kept
    (FULL_TEST, O, D | O | S), (FULL_TEST, D | O, D | O | S), (FULL_TEST, D | O | T, D | O | T | S), (FULL_TEST, D | O | E, D | O | E | S),
    (FULL_TEST, O | T, D | O | T | S),
]


@pytest.mark.parametrize("why, cur, want", TABLE)
def test_table(emu, why, cur, want):
    assert can_ask(cur, why), "the case's own premise"
    assert next_path(emu, cur, why) == want


def test_a_reason_whose_flag_is_set_is_refused_and_no_flag_is_ever_cleared(emu):
    for cur in range(32):
        for why in REASONS:
            nxt = next_path(emu, cur, why)
            if cur & SETS[why]:
                assert nxt is None, (cur, why)
            else:
                assert nxt is not None and nxt & cur == cur and nxt & SETS[why], (cur, why, nxt)
    assert len({emu.emu_call_restart_name(w) for w in REASONS}) == 7


@pytest.mark.parametrize("what", sorted(FIRST))
def test_every_sequence_of_restarts_ends_within_five(emu, what):
    longest, ends = 0, set()
    stack = [(FIRST[what], 0)]
    while stack:
        cur, depth = stack.pop()
        longest = max(longest, depth)
        asked = [w for w in REASONS if can_ask(cur, w)]
        if not asked:
            ends.add(cur)
        for why in asked:
            nxt = next_path(emu, cur, why)
            assert nxt is not None, "a reason whose condition can hold is never refused"
            assert depth + 1 <= 5, (what, cur, why)
            assert next_path(emu, nxt, why) is None, "asked again on the path it led to, the reason is refused"
            stack.append((nxt, depth + 1))
    assert ends == {D | O | T | E | S}                        # the one path on which nothing can ask any more
    assert longest == {"host bytes": 4, "host bytes, shared list": 5, "device bytes": 3}[what]
