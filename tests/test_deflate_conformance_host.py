"""Every DEFLATE decoder (inflate_core.h lane / four literals per trip, inflate_ring.h, inflate_wave.h, inflate_coop.h in its ten modes) on the
hand-built streams of tests/deflate_craft.py, through tests/hostemu: legal streams that zlib's compressor never writes must come out byte for
byte, malformed ones must be refused with the code the catalogue names, and no decoder may read further around its payload than its contract
(tests/hostemu/inflate_inplace.h) says.  zlib's inflate is the referee of the catalogue itself.  No GPU needed."""
import ctypes
import mmap
import os
import random
import re
import zlib

import pytest

import deflate_craft as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# as emu_inflate_inplace numbers them; the coop modes are the ten that tests/test_hostemu.py::inflate cycles
VARIANTS = [("lane", 0), ("lane4", 1), ("ring", 2), ("wave", 3)] + [("coop%d" % p, 16 + p) for p in (0, 1, 2, 3, 5, 7, 8, 10, 13, 15)]
PHASES = (0, 1, 15, 16, 17, 63, 77, 127)
GUARD_VERDICTS = (-100, -101)

# twelve legal entries across the block types, cut at every byte (small payloads: every cut runs through all fourteen variants)
TRUNCATED = ["dist_one_code_len1", "hdist1_zero_length_literals_only", "dist_codes_up_to_15_bits", "ll_eob_alone_between_stored",
             "ll_lengths_1_to_15_15_len258_tails_3_to_18", "ll_all_286_226x8+60x9_rot72", "ll_seven_short_256_fifteen_bit",
             "cl_repeat16_across_hlit_boundary", "cl_hclen_19", "empty_stored_run_and_empty_fixed_between_data", "match_across_block_boundary",
             "out_17_bytes_stored"]


@pytest.fixture(scope="module")
def emu(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "hostemu", "libhostemu.so"))
    lib.emu_inflate_inplace.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                        ctypes.c_uint32]
    lib.emu_inflate_front_bytes.restype = ctypes.c_uint32
    return lib


def decode(emu, variant, payload, cap, phase, tail=b"\0" * 16):
    """One decoder in place on front + payload + 16 bytes behind it; (status, bytes)."""
    front = emu.emu_inflate_front_bytes(variant)
    buf = ctypes.create_string_buffer(b"\0" * front + payload + tail, front + len(payload) + 16)
    out = ctypes.create_string_buffer(max(cap, 1))
    n = ctypes.c_uint32(0)
    st = emu.emu_inflate_inplace(variant, ctypes.addressof(buf) + front, len(payload), out, cap, ctypes.byref(n), phase)
    return st, out.raw[:min(n.value, cap)]


def test_the_catalogue_is_what_it_claims():
    legal, bad = dc.catalogue()
    print("catalogue: %d legal, %d malformed entries" % (len(legal), len(bad)))
    for e in legal:
        verdict, out = dc.zlib_verdict(e.payload)
        assert verdict == "ok" and out == e.expect and e.interp == e.expect, e.name
    for e in bad:
        verdict, msg = dc.zlib_verdict(e.payload)
        if e.zmsg == "truncated":
            assert verdict == "truncated", (e.name, verdict, msg)
        else:
            assert verdict == "error" and e.zmsg in msg, (e.name, verdict, msg)
        assert 1 <= e.code <= 11 and e.code in e.accept
    # it cannot shrink silently: the counts are the ones DESIGN.md states
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"(\d+) legal and (\d+) malformed", text)
    assert m, "DESIGN.md states the catalogue's counts"
    assert (int(m.group(1)), int(m.group(2))) == (dc.MIN_LEGAL, dc.MIN_MALFORMED)
    assert len(legal) >= dc.MIN_LEGAL and len(bad) >= dc.MIN_MALFORMED
    # every reachable code by more than one route
    for code in (1, 2, 3, 4, 5, 6, 7, 8, 9, 11):
        assert sum(1 for e in bad if e.code == code) >= 2, code
    names = {e.name for e in legal}
    assert set(TRUNCATED) <= names and all("cl_hclen_%d" % h in names for h in range(5, 20))
    for e in legal:                                                       # HCLEN is what the name says (bits 13..16 of a first, dynamic block)
        m = re.match(r"cl_hclen_(\d+)$", e.name)
        if m:
            head = int.from_bytes(e.payload[:3], "little")
            assert (head >> 1) & 3 == 2 and ((head >> 13) & 15) + 4 == int(m.group(1))


def test_all_286_symbols_meet_both_halves_of_the_device_symbol_list():
    """LdsTab (kernels.hip) keeps list slots 0..159 bit-packed in LDS and the rest in a global scratch column.  Over the HLIT = 286 entries every symbol
    is used by the tokens, and falls into the first 160 slots in one entry and behind them in another.  (With 226 codes of 8 bits and 60 of 9 alone a
    symbol above 219 can never reach the first 160 slots -- at most 60 symbols sort in front of it -- hence the second length vector.)"""
    hot, cold = set(), set()
    for vec in dc.ALL286_VECTORS.values():
        assert len(vec) == 286 and sum(1 for l in vec if l) > dc.HOT_SLOTS
        for k in dc.ALL286_SHIFTS:
            for s, slot in dc.list_slots(dc.rotated(vec, k)).items():
                (hot if slot < dc.HOT_SLOTS else cold).add(s)
    assert hot == cold == set(range(286))
    used = set()
    for t in dc._all286_tokens():
        used.add(t if isinstance(t, int) else dc.length_symbol(t[0])[0])
    assert used == set(range(256)) | set(range(257, 286))
    assert sum(1 for e in dc.catalogue()[0] if e.name.startswith("ll_all_286_")) == 8


@pytest.mark.parametrize("name,variant", VARIANTS, ids=[n for n, _ in VARIANTS])
def test_legal_entries_come_out_byte_for_byte(emu, name, variant):
    legal, _ = dc.catalogue()
    for k, e in enumerate(legal):
        for cap in (len(e.expect), 65536):
            for j in range(3):
                phase = PHASES[(k + 3 * j + (cap & 1)) % len(PHASES)]
                st, got = decode(emu, variant, e.payload, cap, phase)
                assert st not in GUARD_VERDICTS, (e.name, cap, phase, st)
                assert st == 0 and got == e.expect, (e.name, cap, phase, st, len(got))


@pytest.mark.parametrize("name,variant", VARIANTS, ids=[n for n, _ in VARIANTS])
def test_malformed_entries_are_refused_with_their_code(emu, name, variant):
    _, bad = dc.catalogue()
    for k, e in enumerate(bad):
        for cap in (e.size, 65536):
            st, _ = decode(emu, variant, e.payload, cap, PHASES[k % len(PHASES)])
            assert st not in GUARD_VERDICTS, (e.name, cap, st)
            assert st in e.accept, (e.name, cap, st, sorted(e.accept))


def test_a_member_one_byte_short_or_long_is_an_overflow_or_a_shorter_output(emu):
    """Capacity one below the truth: INF_OUT_OVERFLOW from every variant, nothing written behind the capacity; one above: the stream's own length."""
    legal, _ = dc.catalogue()
    for e in legal:
        if not e.expect:
            continue
        for _, variant in VARIANTS:
            st, got = decode(emu, variant, e.payload, len(e.expect) - 1, 5)
            assert st == dc.INF_OUT_OVERFLOW and e.expect.startswith(got), (e.name, variant, st)
            if len(e.expect) < 65536:
                st, got = decode(emu, variant, e.payload, len(e.expect) + 1, 5)
                assert st == 0 and got == e.expect, (e.name, variant, st)


def test_every_truncation_is_refused(emu):
    legal, _ = dc.catalogue()
    by_name = {e.name: e for e in legal}
    cuts = 0
    for name in TRUNCATED:
        e = by_name[name]
        assert len(e.payload) < 1200
        for cut in range(len(e.payload)):
            p = e.payload[:cut]
            assert dc.zlib_verdict(p)[0] != "ok", (name, cut)
            for _, variant in VARIANTS:
                st, _ = decode(emu, variant, p, len(e.expect), (cut * 7) & 127)
                assert st not in GUARD_VERDICTS and 1 <= st <= 11, (name, cut, variant, st)
            cuts += 1
    assert cuts > 2000


def _zlib_made(rnd, trials):
    for trial in range(trials):
        data = bytes(rnd.choice(b"ACGTN!#") for _ in range(rnd.choice([40, 900, 5000])))
        p = bytearray(zlib.compress(data, 6)[2:-4])
        mode = trial % 3
        if mode == 1:
            k = rnd.randrange(len(p)); p[k] ^= 1 << rnd.randrange(8)
        elif mode == 2:
            p = p[: rnd.randrange(1, len(p))]
        yield bytes(p), (data if mode == 0 else None)


def test_reads_stay_inside_the_contract_for_every_decoder(emu):
    """The payload ends 16 bytes in front of an unmapped page, and in a second pass starts as many bytes behind one as the decoder's contract grants it
    in front (inflate_inplace.h: none, the ring decoder 10): an over-read kills the test process.  Inputs: the catalogue, cuts of its legal entries, and the
    zlib-made valid / bit-flipped / truncated streams of tests/test_hostemu.py."""
    libc = ctypes.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    page, inner = mmap.PAGESIZE, 20
    m = mmap.mmap(-1, (inner + 2) * page)
    base = ctypes.addressof(ctypes.c_char.from_buffer(m))
    lo, hi = page, (inner + 1) * page                                      # the mapped bytes between the two guard pages
    assert libc.mprotect(ctypes.c_void_p(base), page, 0) == 0 and libc.mprotect(ctypes.c_void_p(base + hi), page, 0) == 0
    rnd = random.Random(17)
    legal, bad = dc.catalogue()
    inputs = [(e.payload, e.expect, None, len(e.expect)) for e in legal] + [(e.payload, None, e.accept, e.size) for e in bad]
    by_name = {e.name: e for e in legal}
    for name in TRUNCATED:
        e = by_name[name]
        inputs += [(e.payload[:cut], None, None, len(e.expect)) for cut in range(0, len(e.payload), 5)]
    inputs += [(p, data, None, 65536) for p, data in _zlib_made(rnd, 240)]
    out = ctypes.create_string_buffer(65536)
    n = ctypes.c_uint32(0)
    try:
        for k, (p, expect, accept, cap) in enumerate(inputs):
            assert len(p) + 32 < hi - lo
            tail = bytes(rnd.randrange(256) for _ in range(16))
            for _, variant in VARIANTS:
                front = emu.emu_inflate_front_bytes(variant)
                for start in (hi - 16 - len(p), lo + front):
                    m[start:start + len(p) + 16] = p + tail
                    st = emu.emu_inflate_inplace(variant, ctypes.c_void_p(base + start), len(p), out, cap, ctypes.byref(n), (k * 5) & 127)
                    assert st not in GUARD_VERDICTS
                    if expect is not None:
                        assert st == 0 and out.raw[:n.value] == expect, (k, variant, st)
                    elif accept is not None:
                        assert 1 <= st <= 11, (k, variant, st)            # (which code: above, with zeros behind the payload)
    finally:
        libc.mprotect(ctypes.c_void_p(base), page, 3)
        libc.mprotect(ctypes.c_void_p(base + hi), page, 3)
        del out
