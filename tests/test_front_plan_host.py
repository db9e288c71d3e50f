"""No GPU: the plan of an extract call's front (regtools_amd/csrc/front_plan.h, built into tests/hostemu with plain g++) against brute-force
restatements written here -- linear scans over Python integers, no binary search -- at the smallest sizes at which each rule can go wrong: which
bytes go up and in which chunks, whether the launch is arrival-gated, which members each launch or early-tail part covers, how many segments a
part may frame.

One thing the restatements pin rather than explain: gate_chunk_needed (k_inflate_coop's rule) divides the EXCLUSIVE end of what a lane reads
(cpos + clen + 24) by the chunk size, first_member_reading_past compares the same end with `<=`.  A member whose read ends exactly on a chunk's
end therefore lies in front of the early tail's cut at that chunk and still waits for the next chunk's flag: one byte of caution in the kernel,
no wrong answer (a part is waited for by its waves' count, not by its chunk).  test_gate_rule_against_the_cut states both halves."""
import ctypes as C
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64_MAX = (1 << 64) - 1
BGZF_MAX = 0x10000


class Member(C.Structure):
    _fields_ = [("cpos", C.c_uint64), ("upos", C.c_uint64), ("clen", C.c_uint32), ("isize", C.c_uint32)]


@pytest.fixture(scope="module")
def emu(built):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostemu", "libhostemu.so"))
    u32, u64, sz, i, p = C.c_uint32, C.c_uint64, C.c_size_t, C.c_int, C.c_void_p
    sig = {
        "emu_front_region_kind": (i, [C.c_char_p]),
        "emu_front_shard_cut_targets": (None, [sz, i, i, u64, p]),
        "emu_front_shard_upload_range": (None, [sz, i, i, p, sz, sz, p]),
        "emu_front_payload_takes_gate": (i, [C.c_char_p, sz]),
        "emu_front_inflate_plan_for": (i, [u64, u64]),
        "emu_front_upload_chunks": (sz, [sz, sz, i, C.c_uint, i, p, p, sz]),
        "emu_front_member_query": (None, [p, u32, p, p, p, p]),
        "emu_front_member_range": (None, [u64, u64, p, u32, u32, i, i, p]),
        "emu_front_lookahead": (u32, [i]),
        "emu_front_first_member_reading_past": (u32, [p, u32, u32, u64, u32]),
        "emu_front_gate_chunk_needed": (u32, [u64, u32, u64, u64, u32]),
        "emu_front_upload_covers_members": (i, [p, u32, u32, sz, sz]),
        "emu_front_pieces": (sz, [p, u32, u32, p, sz, p, sz]),
        "emu_front_early_cuts": (sz, [C.c_char_p, p, sz]),
        "emu_front_early_parts": (sz, [p, u32, u32, u64, p, sz, p, sz, u32, u32, p, p, p, sz]),
        "emu_front_early_prefix_segments": (u32, [u64, u64, u32, u32, u32, i]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def arr(ctype, values):
    return (ctype * max(1, len(values)))(*values)


def member_list(clens, isizes=None, first=18):
    """BGZF members laid end to end: 18 bytes of header, clen of payload, 8 of footer; cpos is where the payload starts."""
    ms, cpos, upos = [], first, 0
    for k, clen in enumerate(clens):
        isize = 0xff00 if isizes is None else isizes[k]
        ms.append(dict(cpos=cpos, clen=clen, upos=upos, isize=isize))
        cpos += clen + 26
        upos += isize if isize <= BGZF_MAX else 0
    return ms


def c_members(ms):
    return arr(Member, [Member(m["cpos"], m["upos"], m["clen"], m["isize"]) for m in ms])


# the hand-set lists: 1, 3, 7 and 12 members
LISTS = {"one": [100], "three": [100, 50, 200], "seven_equal": [30] * 7, "twelve": [500, 1, 2, 700, 64, 64, 64, 1000, 3, 3, 900, 10]}


def file_end(ms):
    return ms[-1]["cpos"] + ms[-1]["clen"] + 8


def test_lookaheads_are_the_two_named_constants(emu):
    assert emu.emu_front_lookahead(1) == 24 and emu.emu_front_lookahead(0) == 16


# ---- first_member_reading_past / plan_pieces ------------------------------------------------------------------------------------------------------
def brute_first_reading_past(ms, lo, hi, lim, la):
    for k in range(lo, hi):
        if ms[k]["cpos"] + ms[k]["clen"] + la > lim:
            return k
    return hi


def brute_pieces(ms, m_lo, m_hi, ends):
    out, taken = [], m_lo
    for j, e in enumerate(ends):
        if taken >= m_hi:
            break
        hi = taken
        if j + 1 < len(ends):
            while hi < m_hi and ms[hi]["cpos"] + ms[hi]["clen"] + 16 <= e:
                hi += 1
        else:
            hi = m_hi
        if hi > taken:
            out.append((j, taken, hi))
            taken = hi
    return out


@pytest.mark.parametrize("name", sorted(LISTS))
@pytest.mark.parametrize("la", [16, 24])
def test_first_member_reading_past(emu, name, la):
    ms = member_list(LISTS[name])
    cm, n = c_members(ms), len(ms)
    lims = {0, 1, file_end(ms), file_end(ms) + 100}
    for m in ms:                                               # exactly at a member's reach, one byte below, one above
        lims |= {m["cpos"] + m["clen"] + la + d for d in (-1, 0, 1)}
    for lim in sorted(lims):
        for lo in range(n + 1):
            for hi in range(lo, n + 1):
                assert emu.emu_front_first_member_reading_past(cm, lo, hi, lim, la) == brute_first_reading_past(ms, lo, hi, lim, la), (lim, lo, hi)
    # the edge itself, spelt out: a limit exactly at the reach leaves the member in front, one byte less does not
    reach = ms[0]["cpos"] + ms[0]["clen"] + la
    assert emu.emu_front_first_member_reading_past(cm, 0, n, reach, la) >= 1
    assert emu.emu_front_first_member_reading_past(cm, 0, n, reach - 1, la) == 0


def pieces_of(emu, ms, m_lo, m_hi, ends):
    out = (C.c_uint32 * (3 * (len(ends) + 1)))()
    n = emu.emu_front_pieces(c_members(ms), m_lo, m_hi, arr(C.c_size_t, ends), len(ends), out, len(ends) + 1)
    assert n <= len(ends)
    return [(out[3 * k], out[3 * k + 1], out[3 * k + 2]) for k in range(n)]


def piece_cases(ms):
    """(what the case shows, chunk ends); the last end is the end of the file"""
    end = file_end(ms)
    cases = [("a single chunk", [end]), ("all members in the first chunk", [end - 8 + 16, end + 40, end + 80])]
    for k, m in enumerate(ms):
        reach = m["cpos"] + m["clen"] + 16
        for d in (-1, 0, 1):
            cases.append(("first end %+d from member %d's reach" % (d, k), [reach + d, end]))
            cases.append(("second end %+d from member %d's reach" % (d, k), [ms[0]["cpos"] + 1, reach + d, end]))
        # two ends inside one member's payload: the second chunk completes no member
        if m["clen"] >= 2:
            cases.append(("no member ends in chunk 1 (member %d)" % k, [m["cpos"], m["cpos"] + 1, end]))
    return cases


@pytest.mark.parametrize("name", sorted(LISTS))
def test_plan_pieces(emu, name):
    ms = member_list(LISTS[name])
    n = len(ms)
    seen_empty = seen_first_takes_all = False
    for what, ends in piece_cases(ms):
        for m_lo, m_hi in {(0, n), (min(1, n - 1), n), (0, max(1, n - 1))}:
            got = pieces_of(emu, ms, m_lo, m_hi, ends)
            assert got == brute_pieces(ms, m_lo, m_hi, ends), (what, m_lo, m_hi)
            # in order, the pieces are [m_lo, m_hi): nothing twice, nothing left out, none empty, chunks ascending
            assert got[0][1] == m_lo and got[-1][2] == m_hi, what
            assert all(a[2] == b[1] and a[0] < b[0] for a, b in zip(got, got[1:])), what
            assert all(g_lo < g_hi for _, g_lo, g_hi in got), what
            used = {j for j, _, _ in got}
            seen_empty |= any(j not in used for j in range(max(used)))
            seen_first_takes_all |= len(ends) > 1 and got == [(0, m_lo, m_hi)]
    assert seen_first_takes_all, "no case left every member to the first chunk's launch"
    assert seen_empty or n == 1 and LISTS[name][0] < 2, "no case had a chunk without a launch between two with one"


def test_single_chunk_is_one_piece(emu):
    for name, clens in LISTS.items():
        ms = member_list(clens)
        assert pieces_of(emu, ms, 0, len(ms), [file_end(ms)]) == [(0, 0, len(ms))]


# ---- gate_chunk_needed against the early tail's cut rule -------------------------------------------------------------------------------------------
def brute_need(cpos, clen, gate_lo, chunk_bytes, n_chunks):
    end_b = cpos + clen + 24                                   # the first byte the lane does NOT read
    for k in range(n_chunks - 1):
        if end_b < gate_lo + (k + 1) * chunk_bytes:
            return k
    return n_chunks - 1


@pytest.mark.parametrize("name", sorted(LISTS))
def test_gate_rule_against_the_cut(emu, name):
    ms = member_list(LISTS[name])
    cm, n = c_members(ms), len(ms)
    sizes = {64, 100, 4096}
    for m in ms:                                               # chunk sizes that put chunk 0's end at, below and above a member's reach
        sizes |= {m["cpos"] + m["clen"] + 24 + d for d in (-1, 0, 1)}
    exact = 0
    for gate_lo in (0, 7):
        for cb in sorted(sizes):
            n_chunks = max(2, -(-(file_end(ms) + 24 - gate_lo) // cb) + 1)
            need = [emu.emu_front_gate_chunk_needed(m["cpos"], m["clen"], gate_lo, cb, n_chunks) for m in ms]
            assert need == [brute_need(m["cpos"], m["clen"], gate_lo, cb, n_chunks) for m in ms], (gate_lo, cb)
            assert all(a <= b for a, b in zip(need, need[1:]))
            for k in range(n_chunks - 1):
                chunk_end = gate_lo + (k + 1) * cb
                cut = emu.emu_front_first_member_reading_past(cm, 0, n, chunk_end, 24)
                for i in range(cut):                           # in front of the cut at chunk k: a chunk <= k ...
                    reach = ms[i]["cpos"] + ms[i]["clen"] + 24
                    if reach == chunk_end:                     # ... but for the read that ends exactly on the chunk's end (module docstring)
                        assert need[i] == k + 1, (gate_lo, cb, k, i)
                        exact += 1
                    else:
                        assert need[i] <= k, (gate_lo, cb, k, i)
                if cut < n:                                    # the member at the cut: a later chunk
                    assert need[cut] > k, (gate_lo, cb, k, cut)
    assert exact, "no member's read ended exactly on a chunk's end"


def test_gate_chunk_clamps_and_floors(emu):
    # a member ending beyond the last chunk waits for the last one; one ending at or in front of the range's first byte for chunk 0
    assert emu.emu_front_gate_chunk_needed(10_000, 500, 0, 100, 4) == 3
    assert emu.emu_front_gate_chunk_needed(10_000, 500, 0, 100, 2) == 1
    assert emu.emu_front_gate_chunk_needed(18, 100, 142, 64, 8) == 0          # end_b == gate_lo
    assert emu.emu_front_gate_chunk_needed(18, 100, 143, 64, 8) == 0          # end_b < gate_lo
    assert emu.emu_front_gate_chunk_needed(18, 100, 141, 64, 8) == 0 and emu.emu_front_gate_chunk_needed(18, 100, 78, 64, 8) == 1
    assert emu.emu_front_gate_chunk_needed((1 << 40) + 18, 65000, 1 << 40, 1 << 26, 16) == 0
    assert emu.emu_front_gate_chunk_needed((1 << 40) + (5 << 26), 65000, 1 << 40, 1 << 26, 16) == 5


def test_upload_covers_members(emu):
    ms = member_list(LISTS["twelve"])
    cm = c_members(ms)
    lo, hi = ms[3]["cpos"] - 18, ms[8]["cpos"] + ms[8]["clen"] + 16
    assert emu.emu_front_upload_covers_members(cm, 3, 9, lo, hi) == 1
    assert emu.emu_front_upload_covers_members(cm, 3, 9, lo + 1, hi) == 0 and emu.emu_front_upload_covers_members(cm, 3, 9, lo, hi - 1) == 0
    assert emu.emu_front_upload_covers_members(cm, 3, 9, 0, hi + 100) == 1


# ---- plan_early_parts ------------------------------------------------------------------------------------------------------------------------------
def brute_early_parts(ms, m_lo, m_hi, upos_lo, ends, cuts, early_min, align):
    """([(members, waves, upos)], [why each cut was kept or dropped])"""
    parts, why = [], []
    for cut in cuts:
        lim = ends[max(1, len(ends) * cut // 16) - 1]
        in_front = sum(1 for k in range(m_lo, m_hi) if ms[k]["cpos"] + ms[k]["clen"] + 24 <= lim)
        k = in_front - in_front % align
        prev = parts[-1][0] if parts else 0
        if parts and k == prev:
            why.append("same multiple")
        elif k < prev + early_min:
            why.append("part too small")
        elif (m_hi - m_lo) - k < early_min:
            why.append("too few remain")
        else:
            why.append("kept")
            parts.append((k, k // 64, ms[m_lo + k]["upos"] - upos_lo))
    return parts, why


def early_parts_of(emu, ms, m_lo, m_hi, upos_lo, ends, cuts, early_min, align):
    mem, wav, upo = (C.c_uint32 * 8)(), (C.c_uint32 * 8)(), (C.c_uint64 * 8)()
    n = emu.emu_front_early_parts(c_members(ms), m_lo, m_hi, upos_lo, arr(C.c_size_t, ends), len(ends), arr(C.c_uint, cuts), len(cuts), early_min, align,
                                  mem, wav, upo, 8)
    assert n <= 7
    return [(mem[k], wav[k], upo[k]) for k in range(n)]


FORTY = member_list([100] * 40)                                # 126 bytes a member; sixteen chunks of 315 bytes: 2.5 members each
FORTY_ENDS = [315 * (j + 1) for j in range(16)]
# name -> (m_lo, cuts, early_min, what the cuts must come to)
EARLY_CASES = {
    "default cuts, all kept": (0, [6, 9, 12, 14], 4, ["kept"] * 4),
    "parts smaller than early_min": (0, [6, 9, 12, 14], 10, ["kept", "part too small", "kept", "part too small"]),
    "fewer than early_min remain": (0, [6, 15], 6, ["kept", "too few remain"]),
    "two cuts round to one multiple": (0, [5, 6], 1, ["kept", "same multiple"]),
    "seven cuts kept": (0, [2, 4, 6, 8, 10, 12, 14], 4, ["kept"] * 7),
    "a range that starts at member 5": (5, [6, 9, 12, 14], 4, ["kept"] * 4),
    "first cut in front of the first group": (0, [1, 6], 4, ["part too small", "kept"]),
}


@pytest.mark.parametrize("name", sorted(EARLY_CASES))
def test_plan_early_parts(emu, name):
    m_lo, cuts, early_min, want_why = EARLY_CASES[name]
    upos_lo = FORTY[m_lo]["upos"]
    want, why = brute_early_parts(FORTY, m_lo, 40, upos_lo, FORTY_ENDS, cuts, early_min, 4)
    assert why == want_why, "the case no longer shows what its name says"
    got = early_parts_of(emu, FORTY, m_lo, 40, upos_lo, FORTY_ENDS, cuts, early_min, 4)
    assert got == want
    for members, waves, upos in got:
        assert members % 4 == 0 and waves == members // 64 and upos == FORTY[m_lo + members]["upos"] - upos_lo
    assert [p[0] for p in got] == sorted({p[0] for p in got})


def test_early_cases_cover_every_reason():
    """a later edit of the inputs must not quietly empty a category"""
    seen = [w for _, _, _, why in EARLY_CASES.values() for w in why]
    for reason in ("kept", "part too small", "too few remain", "same multiple"):
        assert reason in seen, reason
    assert any(set(why) == {"kept"} for _, _, _, why in EARLY_CASES.values())
    assert any(why == ["kept"] * 7 for _, _, _, why in EARLY_CASES.values())


def test_plan_early_parts_at_the_products_alignment(emu):
    rng = random.Random(5)
    ms = member_list([rng.randrange(2000, 20000) for _ in range(3000)])
    end = file_end(ms)
    chunk = ((end + 15) // 16 + 4095) & ~4095
    ends = [e for e in range(chunk, end, chunk)] + [end]
    assert len(ends) == 16
    for m_lo, cuts, early_min in ((0, [6, 9, 12, 14], 1), (0, [6, 9, 12, 14], 1025), (7, [2, 4, 6, 8, 10, 12, 14], 1), (0, [6, 9, 12, 14], 4096)):
        upos_lo = ms[m_lo]["upos"]
        want, why = brute_early_parts(ms, m_lo, 3000, upos_lo, ends, cuts, early_min, 1024)
        got = early_parts_of(emu, ms, m_lo, 3000, upos_lo, ends, cuts, early_min, 1024)
        assert got == want, (m_lo, cuts, early_min)
        assert all(members % 1024 == 0 and waves == members // 64 for members, waves, _ in got)
        if early_min == 1:
            assert [p[0] for p in got] == [1024, 2048] and "same multiple" in why
        if early_min == 4096:
            assert got == []


# ---- parse_early_cuts ------------------------------------------------------------------------------------------------------------------------------
def brute_cuts(text):
    vals, rest = [], "6,9,12,14" if text is None else text
    for _ in range(7):                                         # up to seven numbers, commas between them; the first thing that is neither ends it
        m = re.match(r"\s*(\d+)", rest)
        if not m:
            break
        vals.append(int(m.group(1)))
        rest = rest[m.end():]
        if not rest.startswith(","):
            break
        rest = rest[1:]
    out = []
    for x in vals:
        if 0 < x < 16 and (not out or x > out[-1]):
            out.append(x)
    return out


@pytest.mark.parametrize("text, want", [
    (None, [6, 9, 12, 14]), ("6,9,12,14", [6, 9, 12, 14]), ("0", []), ("9,6,12", [9, 12]), ("6,6,7", [6, 7]), ("6,16,20,14", [6, 14]), ("15", [15]), ("16", []),
    ("1,2,3,4,5,6,7,8,9", [1, 2, 3, 4, 5, 6, 7]), ("2,4,6,8,10,12,14", [2, 4, 6, 8, 10, 12, 14]), ("garbage", []), ("", []), ("6,x,9", [6]), ("6;9", [6]),
    ("8,12,14", [8, 12, 14])])
def test_parse_early_cuts(emu, text, want):
    assert brute_cuts(text) == want
    out = (C.c_uint * 8)()
    n = emu.emu_front_early_cuts(None if text is None else text.encode(), out, 8)
    assert list(out[:n]) == want and n <= 7


# ---- plan_upload_chunks ----------------------------------------------------------------------------------------------------------------------------
def upload_chunks_of(emu, lo, hi, gated, n, one_shot):
    gc, end = C.c_size_t(), (C.c_size_t * 80)()
    k = emu.emu_front_upload_chunks(lo, hi, int(gated), n, int(one_shot), C.byref(gc), end, 80)
    return gc.value, list(end[:k])


@pytest.mark.parametrize("n", [2, 7, 16, 64])
@pytest.mark.parametrize("lo", [0, 8192])
def test_gated_upload_chunks(emu, n, lo):
    for length in (4096 * n * 3, 4096 * n * 3 + 1234, 4096 * n * 3 - 1, 2 * 4096 * n, 2 * 4096 * n + 1, 533_000_001):
        hi = lo + length
        gc, ends = upload_chunks_of(emu, lo, hi, True, n, False)
        per = -(-length // n)                                  # an n-th of the range, rounded up, then up to 4 KiB
        while per % 4096:
            per += 1
        assert gc == per
        want, e = [], lo + per
        while e < hi:
            want.append(e)
            e += per
        assert ends == want + [hi]
        assert ends[-1] == hi and all(a < b for a, b in zip(ends, ends[1:])) and len(ends) <= n
        assert all((e - lo) % 4096 == 0 for e in ends[:-1])


def brute_ungated(lo, hi, one_shot):
    ends = []
    for pc in ([] if one_shot else [33, 67]):
        e = lo + int(float(hi - lo) * pc / 100.0)
        while e % 4096:
            e += 1
        if lo < e < hi and (not ends or e > ends[-1]):
            ends.append(e)
    return ends + [hi]


def test_ungated_upload_chunks(emu):
    for lo, hi in ((0, 100 << 20), (8192, (8 << 20) + 77), (0, 5000), (0, 4000), (4096, 4096 + 12288), (0, 12289), (4096, 4096)):
        gc, ends = upload_chunks_of(emu, lo, hi, False, 16, False)
        assert gc == 0 and ends == brute_ungated(lo, hi, False), (lo, hi)
        assert ends[-1] == hi and all(a < b for a, b in zip(ends, ends[1:]))
        assert upload_chunks_of(emu, lo, hi, False, 16, True) == (0, [hi])
    # a range so small that both cuts round to the same 4 KiB: one cut, or none when that lies at or behind the end
    assert upload_chunks_of(emu, 0, 5000, False, 16, False)[1] == [4096, 5000]
    assert upload_chunks_of(emu, 0, 4000, False, 16, False)[1] == [4000]
    assert upload_chunks_of(emu, 0, 100 << 20, False, 16, False)[1] == [34603008, 70254592, 100 << 20]


# ---- shard cuts and the shard's upload range -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_shards", [2, 3])
def test_shard_cut_targets(emu, n_shards):
    for bam_len in (28, 1000, 533_000_001, (1 << 40) + 3):
        for floor in (1, 5 << 16, ((bam_len // 2) << 16) | 77):
            for shard in range(n_shards):
                tgt = (C.c_uint64 * 2)()
                emu.emu_front_shard_cut_targets(bam_len, shard, n_shards, floor, tgt)
                want = [max(int(float(bam_len) * (shard + k) / n_shards) << 16, floor) for k in (0, 1)]
                assert list(tgt) == want, (bam_len, floor, shard)
                assert tgt[0] <= tgt[1] and tgt[0] >= floor
            # what one shard ends on, the next one starts on
            a, b = (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
            emu.emu_front_shard_cut_targets(bam_len, 0, n_shards, floor, a)
            emu.emu_front_shard_cut_targets(bam_len, 1, n_shards, floor, b)
            assert a[1] == b[0]


def brute_upload_range(bam_len, shard, n_shards, got, header_bytes, fourth_end):
    lo, hi = 0, bam_len
    if shard > 0:
        lo = bam_len if got[0] == U64_MAX else min(bam_len, got[0] >> 16)
    if shard + 1 < n_shards and got[1] != U64_MAX:
        hi = min(bam_len, (got[1] >> 16) + 2 * BGZF_MAX + 64)
    hi = max(hi, lo)
    hdr_hi = min(lo, max(header_bytes, fourth_end) + 64)
    lo -= lo % 4096
    if lo < hdr_hi:
        lo, hdr_hi = 0, 0
    return [lo, hi, hdr_hi]


RANGE_CASES = [
    # (what, bam_len, shard, n_shards, got, header_bytes, fourth_member_end, expected or None)
    ("first of two", 10_000_000, 0, 2, [3 << 16, (5_000_000 << 16) | 9], 3000, 90_000, [0, 5_000_000 + 131136, 0]),
    ("last of two", 10_000_000, 1, 2, [(5_000_000 << 16) | 9, U64_MAX], 3000, 90_000, [4_997_120, 10_000_000, 90_064]),
    ("middle of three", 10_000_000, 1, 3, [3_333_333 << 16, 6_666_666 << 16], 3000, 90_000, [3_330_048, 6_666_666 + 131136, 90_064]),
    ("last of three", 10_000_000, 2, 3, [6_666_666 << 16, U64_MAX], 200_000, 90_000, [6_664_192, 10_000_000, 200_064]),
    ("no anchor behind the lower target", 10_000_000, 1, 2, [U64_MAX, U64_MAX], 3000, 90_000, [9_998_336, 10_000_000, 90_064]),
    ("no anchor behind the upper target", 10_000_000, 1, 3, [3_333_333 << 16, U64_MAX], 3000, 90_000, [3_330_048, 10_000_000, 90_064]),
    ("the range meets the header", 10_000_000, 1, 2, [90_100 << 16, U64_MAX], 3000, 90_000, [0, 10_000_000, 0]),
    ("the range starts inside the header", 10_000_000, 1, 2, [50_000 << 16, U64_MAX], 3000, 90_000, [0, 10_000_000, 0]),
    ("just clear of the header", 10_000_000, 1, 2, [94_208 << 16, U64_MAX], 3000, 90_000, [94_208, 10_000_000, 90_064]),
    ("upper cut far in front of the lower", 10_000_000, 1, 3, [6_000_000 << 16, 1_000_000 << 16], 3000, 90_000, [5_996_544, 6_000_000, 90_064]),
    ("upper cut's slack runs past the file", 10_000_000, 0, 2, [1, 9_990_000 << 16], 3000, 90_000, [0, 10_000_000, 0]),
    ("no member list", 10_000_000, 1, 2, [5_000_000 << 16, U64_MAX], 3000, 0, [4_997_120, 10_000_000, 3064]),
]


@pytest.mark.parametrize("case", RANGE_CASES, ids=[c[0] for c in RANGE_CASES])
def test_shard_upload_range(emu, case):
    what, bam_len, shard, n_shards, got, hb, fourth, want = case
    assert brute_upload_range(bam_len, shard, n_shards, got, hb, fourth) == want, "the case's own expectation"
    out = (C.c_size_t * 3)()
    emu.emu_front_shard_upload_range(bam_len, shard, n_shards, arr(C.c_uint64, got), hb, fourth, out)
    assert list(out) == want
    assert out[0] % 4096 == 0 and out[0] <= out[1] <= bam_len and out[2] <= max(out[0], 0) + (out[2] if out[0] == 0 else 0)


# ---- host_member_query / member_range --------------------------------------------------------------------------------------------------------------
def brute_query(ms, q):
    n = len(ms)
    idx = [next((k for k in range(n) if ms[k]["cpos"] == x + 18), n) for x in q]
    upos = [ms[k]["upos"] if k < n else U64_MAX for k in idx]
    stop = next((k for k in range(idx[0], n) if ms[k]["isize"] == 0 or ms[k]["isize"] > BGZF_MAX), 0xffffffff)
    return idx, upos, stop


def query_of(emu, ms, q):
    qi, qu, stop = (C.c_uint32 * 3)(), (C.c_uint64 * 3)(), C.c_uint32()
    emu.emu_front_member_query(c_members(ms), len(ms), arr(C.c_uint64, q), qi, qu, C.byref(stop))
    return list(qi), list(qu), stop.value


def test_host_member_query(emu):
    clens = LISTS["twelve"]
    starts = [m["cpos"] - 18 for m in member_list(clens)]
    for isizes, note in (([0xff00] * 12, "no stop"), ([0xff00] * 5 + [0] + [0xff00] * 6, "an empty member"), ([0xff00] * 2 + [0x10001] + [0xff00] * 9, "oversized"),
                         ([0x10000] * 12, "the largest size is no stop"), ([0xff00] * 11 + [0], "the EOF member")):
        ms = member_list(clens, isizes)
        for q in ([0, 0, U64_MAX - 64], [starts[3], starts[3], starts[9]], [starts[7], starts[0], starts[11]], [starts[3] + 1, starts[3] - 1, starts[11] + 5000],
                  [starts[11], starts[11], starts[11]], [starts[6], 1, 2]):
            assert query_of(emu, ms, q) == brute_query(ms, q), (note, q)
    ms = member_list(clens, [0xff00] * 5 + [0] + [0xff00] * 6)
    assert query_of(emu, ms, [starts[3], 0, 0])[2] == 5 and query_of(emu, ms, [starts[5], 0, 0])[2] == 5            # a stop behind / at q_index[0]
    assert query_of(emu, ms, [starts[6], 0, 0])[2] == 0xffffffff                                                  # a stop in front of it is none
    assert query_of(emu, ms, [starts[6] + 1, 0, 0]) == ([12, 0, 0], [U64_MAX, 0, 0], 0xffffffff)                     # a miss: the stop scan starts at n
    assert query_of(emu, member_list([100]), [0, 0, 0]) == ([0, 0, 0], [0, 0, 0], 0xffffffff)
    assert query_of(emu, [], [0, 0, 0]) == ([0, 0, 0], [U64_MAX] * 3, 0xffffffff)


def brute_member_range(cut_lo, cut_hi, q_index, stop, n_all, chunked, to_end):
    m_lo = q_index[1] if cut_lo else 0
    if m_lo <= 4:
        m_lo = 0
    m_hi = stop
    if cut_hi != U64_MAX:
        hi_m = q_index[2] + (1 if q_index[2] < n_all and cut_hi % 65536 else 0)
        if not chunked:
            m_hi = min(stop, hi_m)
        elif to_end:
            m_hi = n_all
        else:
            m_hi = min(n_all, hi_m + 2)
    return [min(m_lo, m_hi), m_hi]


RANGE_OF_MEMBERS = [
    # (what, cut_lo, cut_hi, q_index, stop, n_members_all, chunked, region_to_file_end, expected)
    ("whole file", 0, U64_MAX, [0, 0, 100], 99, 100, False, False, [0, 99]),
    ("lower cut at member 4: the head stays", 5 << 16, U64_MAX, [0, 4, 100], 99, 100, False, False, [0, 99]),
    ("lower cut at member 5", 5 << 16, U64_MAX, [0, 5, 100], 99, 100, False, False, [5, 99]),
    ("upper cut at a member's start", 0, 700 << 16, [0, 0, 50], 99, 100, False, False, [0, 50]),
    ("upper cut inside a member", 0, (700 << 16) | 1, [0, 0, 50], 99, 100, False, False, [0, 51]),
    ("upper cut behind the stop", 0, (700 << 16) | 1, [0, 0, 50], 30, 100, False, False, [0, 30]),
    ("upper cut is no member", 0, (700 << 16) | 1, [0, 0, 100], 99, 100, False, False, [0, 99]),
    ("a region's chunks: two members more", 9 << 16, (700 << 16) | 1, [9, 9, 50], 30, 100, True, False, [9, 53]),
    ("a region's chunks, no in-block offset", 9 << 16, 700 << 16, [9, 9, 50], 30, 100, True, False, [9, 52]),
    ("a region's chunks near the end", 9 << 16, (700 << 16) | 1, [9, 9, 98], 99, 100, True, False, [9, 100]),
    ("a region read to the file's end", 9 << 16, (700 << 16) | 1, [9, 9, 50], 30, 100, True, True, [9, 100]),
    ("lower cut behind the upper", 80 << 16, 700 << 16, [0, 80, 50], 99, 100, False, False, [50, 50]),
    ("lower cut behind the stop", 80 << 16, U64_MAX, [0, 80, 100], 30, 100, False, False, [30, 30]),
    ("lower cut is no member", 80 << 16, U64_MAX, [0, 100, 100], 99, 100, False, False, [99, 99]),
]


@pytest.mark.parametrize("case", RANGE_OF_MEMBERS, ids=[c[0] for c in RANGE_OF_MEMBERS])
def test_member_range(emu, case):
    what, cut_lo, cut_hi, qi, stop, n_all, chunked, to_end, want = case
    assert brute_member_range(cut_lo, cut_hi, qi, stop, n_all, chunked, to_end) == want, "the case's own expectation"
    out = (C.c_uint32 * 2)()
    emu.emu_front_member_range(cut_lo, cut_hi, arr(C.c_uint32, qi), stop, n_all, int(chunked), int(to_end), out)
    assert list(out) == want and out[0] <= out[1]


# ---- early_prefix_segments -------------------------------------------------------------------------------------------------------------------------
def brute_prefix(part_upos, pos0, seg, n_seg, s_done, small_ok):
    if part_upos <= pos0 + 2 * BGZF_MAX:
        return 0
    s = sum(1 for k in range(n_seg) if pos0 + (k + 1) * seg <= part_upos - BGZF_MAX)       # segments wholly a member in front of the part
    need_new, need_left = (2, 1) if small_ok else (1024, 64)
    return s if s >= s_done + need_new and n_seg - s >= need_left else 0


def test_early_prefix_segments(emu):
    seg, pos0 = 16384, 1000
    at = lambda s: pos0 + BGZF_MAX + s * seg                   # the smallest part offset with s segments in front of its margin
    cases = [
        # (part_upos, n_seg, s_done, small_ok, expected)
        (pos0 + 2 * BGZF_MAX, 100, 0, True, 0),                # a part two members behind the stream's start: skipped
        (pos0 + 2 * BGZF_MAX + 1, 100, 0, True, 4),            # one byte beyond
        (pos0 + 2 * BGZF_MAX + 1, 100, 0, False, 0),
        (at(1024), 2000, 0, False, 1024), (at(1024) - 1, 2000, 0, False, 0),              # 1,024 new segments, and one fewer
        (at(1524), 2000, 500, False, 1524), (at(1523), 2000, 500, False, 0),
        (at(1936), 2000, 0, False, 1936), (at(1937), 2000, 0, False, 0),                  # 64 segments left, and 63
        (at(6), 100, 4, True, 6), (at(5), 100, 4, True, 0),                               # small_ok: two new segments, and one
        (at(99), 100, 4, True, 99), (at(100), 100, 4, True, 0), (at(5000), 100, 4, True, 0),   # one segment left, and none (clamped to n_seg)
        (at(5000), 2000, 0, False, 0),
    ]
    for part_upos, n_seg, s_done, small_ok, want in cases:
        assert brute_prefix(part_upos, pos0, seg, n_seg, s_done, small_ok) == want, "the case's own expectation"
        assert emu.emu_front_early_prefix_segments(part_upos, pos0, seg, n_seg, s_done, int(small_ok)) == want, (part_upos, n_seg, s_done, small_ok)
    for part_upos in range(pos0 + 2 * BGZF_MAX - 2, pos0 + 2 * BGZF_MAX + 5 * seg, 4093):
        for s_done in (0, 3):
            assert emu.emu_front_early_prefix_segments(part_upos, pos0, seg, 9, s_done, 1) == brute_prefix(part_upos, pos0, seg, 9, s_done, True)


# ---- payload_takes_gate ----------------------------------------------------------------------------------------------------------------------------
def bgzf28(isize, bsize=27, magic=b"\x1f\x8b"):
    """a 28-byte BGZF member (an empty stored-less DEFLATE stream) whose footer claims `isize` bytes"""
    m = magic + b"\x08\x04" + b"\0" * 4 + b"\0\xff" + b"\x06\0" + b"BC" + b"\x02\0" + bsize.to_bytes(2, "little") + b"\x03\0" + b"\0" * 4 + isize.to_bytes(4, "little")
    assert len(m) == 28
    return m


def brute_takes_gate(buf):
    cb = ub = o = 0
    for _ in range(64):
        if o + 28 > len(buf) or buf[o:o + 2] != b"\x1f\x8b" or buf[o + 12:o + 14] != b"BC":
            break
        bl = int.from_bytes(buf[o + 16:o + 18], "little") + 1
        if bl < 26 or o + bl > len(buf):
            break
        cb, ub, o = cb + bl, ub + int.from_bytes(buf[o + bl - 4:o + bl], "little"), o + bl
    return cb == 0 or ub < 32 * cb                             # run-length payloads (more than 32 x) keep the pieces


@pytest.mark.parametrize("what, buf, want", [
    ("ratio exactly 32", bgzf28(896), False), ("just below 32", bgzf28(895), True), ("just above 32", bgzf28(897), False),
    ("two members, exactly 32 together", bgzf28(1792) + bgzf28(0), False), ("two members, below together", bgzf28(1791) + bgzf28(0), True),
    ("the first member is not BGZF", bgzf28(5000, magic=b"\x1f\x8c") + bgzf28(0), True), ("no BC subfield", bgzf28(5000).replace(b"BC", b"BD"), True),
    ("the first BSIZE runs past the end", bgzf28(5000, bsize=28), True), ("the second BSIZE runs past the end", bgzf28(5000) + bgzf28(0, bsize=40), False),
    ("the second member's verdict is lost with it", bgzf28(10) + bgzf28(50000, bsize=40), True), ("a BSIZE below a member's least", bgzf28(5000, bsize=24), True),
    ("fewer than 28 bytes", bgzf28(5000)[:27], True), ("the 65th member is not looked at", bgzf28(10) * 64 + bgzf28(10_000_000), True),
    ("the 64th is", bgzf28(10) * 63 + bgzf28(10_000_000), False)])
def test_payload_takes_gate(emu, what, buf, want):
    assert brute_takes_gate(buf) == want, "the case's own expectation"
    assert bool(emu.emu_front_payload_takes_gate(buf, len(buf))) == want
    assert emu.emu_front_inflate_plan_for(28, 896) == 0 and emu.emu_front_inflate_plan_for(28, 895) == 1


def test_region_kind(emu):
    assert [emu.emu_front_region_kind(r) for r in (None, b".", b"*", b"chr1", b"chr1:5-9", b"", b"..", b"*x")] == [0, 0, 1, 2, 2, 2, 2, 2]
