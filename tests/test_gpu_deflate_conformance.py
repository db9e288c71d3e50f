"""The five forms of the DEFLATE kernel (rgx_k_inflate_form: lane, wave, ring, coop, lane with four literals per trip) on the hand-built streams of
tests/deflate_craft.py -- what zlib's compressor never writes, and what no decoder may accept -- through the stage entry point, laid out as
test_inflate_kernel_on_adversarial_members (tests/test_gpu_parity.py) lays its members out: payloads with 8..40 filler bytes between them, the first
at offset 32, the arena preset to 0xA5 and passed at +256, gaps of 0, 5 or 10 bytes between members, status preset to [0xffffffff, 0].  Only the
catalogue itself is used (the CPU tests and tests/hostemu/inflate_edges.cpp run every entry of it first).  And end to end: a BAM re-deflated in five
foreign dialects must extract to the same junctions as its zlib-deflated original."""
import random
import struct
import zlib

import pytest

import bamio
import deflate_craft as dc
from test_gpu_parity import FORMS, gpu_extract

pytestmark = pytest.mark.gpu

PAD = 256                      # the arena is passed this far into its allocation and checked this far behind its last member


def launch(form, members):
    """members: (payload, isize claimed, gap behind the member, filler behind the payload or None = 8..40 seeded bytes).
    Returns (rc, [status0, status1], the arena's bytes from -PAD on, [(arena offset, isize)])."""
    import torch
    from regtools_amd import _ffi
    rnd = random.Random(len(members) * 131 + form)
    blob, rows, upos = bytearray(rnd.randrange(256) for _ in range(32)), [], 0
    for payload, isize, gap, filler in members:
        rows.append((len(blob), upos, len(payload), isize))
        blob += payload + (bytes(rnd.randrange(256) for _ in range(rnd.randint(8, 40))) if filler is None else filler)
        upos += (isize if isize <= 65536 else 0) + gap
    arr = (_ffi.Member * len(rows))(*[_ffi.Member(*r) for r in rows])
    d_comp = torch.zeros(len(blob) + 64, dtype=torch.uint8, device="cuda")
    d_comp[: len(blob)].copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
    d_mem = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    d_arena = torch.full((PAD + upos + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    d_status = torch.tensor([0xffffffff, 0], dtype=torch.int64).to(torch.uint32).cuda()
    torch.cuda.synchronize()
    rc = _ffi.lib().rgx_k_inflate_form(form, d_comp.data_ptr(), d_mem.data_ptr(), len(rows), d_arena.data_ptr() + PAD, d_status.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, d_status.cpu().tolist(), d_arena.cpu().numpy().tobytes(), [(r[1], r[3]) for r in rows]


def expected_arena(total_len, places, datas):
    want = bytearray(b"\xa5" * total_len)
    for (up, _), d in zip(places, datas):
        if d is not None:
            want[PAD + up: PAD + up + len(d)] = d
    return bytes(want)


def small_legal(n):
    """n small legal members, cycling through the catalogue's legal entries of at most 2,000 output bytes (long matches for the wave's copies among them)."""
    legal, _ = dc.catalogue()
    small = [e for e in legal if len(e.expect) <= 2000]
    assert len(small) >= 40 and any(len(e.expect) > 500 for e in small)
    return [small[(7 * k) % len(small)] for k in range(n)]


@pytest.mark.parametrize("form", [f for f, _ in FORMS], ids=[n for _, n in FORMS])
def test_legal_catalogue_twice_with_different_neighbours(gpu_ctx, form):
    """The whole legal list, then the list rotated by one: every entry at two lane positions with different neighbours, two full waves of the lane forms
    and a partial one.  The arena must equal the expectation everywhere, 0xA5 outside the members included."""
    legal, _ = dc.catalogue()
    order = legal + legal[1:] + legal[:1]
    assert len(order) >= 130
    members = [(e.payload, len(e.expect), (k % 3) * 5, None) for k, e in enumerate(order)]
    rc, status, got, places = launch(form, members)
    assert rc == 0 and status[0] == 0xffffffff, status
    want = expected_arena(len(got), places, [e.expect for e in order])
    if got != want:                                                       # name the first entry that differs
        for (up, isz), e in zip(places, order):
            assert got[PAD + up: PAD + up + isz] == e.expect, e.name
    assert got == want


@pytest.mark.parametrize("form", [f for f, _ in FORMS], ids=[n for _, n in FORMS])
def test_one_malformed_member_among_good_ones(gpu_ctx, form):
    """Per malformed entry one launch of 66 members, 65 of them small legal ones, the bad one at index 0, 63, 64, 65 in turn (a wave's first and last
    lane, the next wave's first two), claiming the size its entry names.  status = [its index, its code]; every good member byte-exact; nothing outside
    the members written.  What the bad member left in its own range is not specified.  Zeros stand behind the bad payload: what a decoder reports after
    it ran off its input depends on the foreign bytes it finds there, and zeros make that the overrun."""
    _, bad = dc.catalogue()
    good = small_legal(65)
    for k, e in enumerate(bad):
        at = (0, 63, 64, 65)[k % 4]
        entries = good[:at] + [e] + good[at:]
        members = [(x.payload, e.size if x is e else len(x.expect), ((j + k) % 3) * 5, bytes(24) if x is e else None) for j, x in enumerate(entries)]
        rc, status, got, places = launch(form, members)
        assert rc == 0, e.name
        assert status[0] == at and status[1] in e.accept, (e.name, at, status, sorted(e.accept))
        datas = [None if x is e else x.expect for x in entries]
        want = bytearray(expected_arena(len(got), places, datas))
        up, isz = places[at]
        want[PAD + up: PAD + up + isz] = got[PAD + up: PAD + up + isz]      # the bad member's own range: unspecified
        assert got == bytes(want), (e.name, at)


@pytest.mark.parametrize("form", [f for f, _ in FORMS], ids=[n for _, n in FORMS])
def test_several_malformed_members_report_the_first(gpu_ctx, form):
    """Bad members at 5, 70 and 130 with three different codes: status[0] is the first, status[1] one of the three codes (the kernel documents the
    code as best effort), every good member intact."""
    _, bad = dc.catalogue()
    by_name = {e.name: e for e in bad}
    three = {5: by_name["btype_3_after_data"], 70: by_name["distance_one_past_the_start"], 130: by_name["repeat16_first"]}
    assert len({e.code for e in three.values()}) == 3
    entries = small_legal(140)
    for at, e in three.items():
        entries[at] = e
    members = [(x.payload, x.size if x.expect is None else len(x.expect), (j % 3) * 5, bytes(24) if x.expect is None else None) for j, x in enumerate(entries)]
    rc, status, got, places = launch(form, members)
    assert rc == 0 and status[0] == 5 and status[1] in {e.code for e in three.values()}, status
    for (up, isz), x in zip(places, entries):
        if x.expect is not None:
            assert got[PAD + up: PAD + up + isz] == x.expect, x.name
    assert got[:PAD] == b"\xa5" * PAD and got[-PAD:] == b"\xa5" * PAD


@pytest.mark.parametrize("form", [f for f, _ in FORMS], ids=[n for _, n in FORMS])
def test_what_a_member_claims_about_its_size(gpu_ctx, form):
    """A legal stream whose claimed size is wrong, its neighbour right behind it (gap 0): one more than the truth -> INF_SIZE_MISMATCH, one fewer ->
    INF_OUT_OVERFLOW, 65537 -> INF_OUT_OVERFLOW and 0xffffffff -> INF_IN_OVERRUN with nothing written for the member; the neighbours are intact."""
    legal, _ = dc.catalogue()
    e = [x for x in legal if x.name == "ll_lengths_1_to_15_15_len258_tails_3_to_18"][0]
    good = [x for x in small_legal(80) if x is not e][:70]
    n = len(e.expect)
    assert len(good) == 70
    for claim, code in ((n + 1, dc.INF_SIZE_MISMATCH), (n - 1, dc.INF_OUT_OVERFLOW), (65537, dc.INF_OUT_OVERFLOW), (0xffffffff, dc.INF_IN_OVERRUN)):
        for at in (3, 64):
            entries = good[:at] + [e] + good[at:]
            members = [(x.payload, claim if x is e else len(x.expect), 0, None) for x in entries]
            rc, status, got, places = launch(form, members)
            assert rc == 0 and status == [at, code], (claim, at, status)
            datas = [None if x is e else x.expect for x in entries]
            want = bytearray(expected_arena(len(got), places, datas))
            up = places[at][0]
            if claim == n + 1:
                want[PAD + up: PAD + up + n] = e.expect                    # it decoded to its end; the byte it claimed beyond that is its own
                want[PAD + up + n] = got[PAD + up + n]                     # (the lane forms' last chunk store zeroes it, the others leave it)
            elif claim == n - 1:
                want[PAD + up: PAD + up + n - 1] = got[PAD + up: PAD + up + n - 1]      # its own range: unspecified
            assert got == bytes(want), (claim, at)


def _bgzf_member(payload, data):
    total = 18 + len(payload) + 8
    assert total <= 65536
    return (bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", total - 1) + payload +
            struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))


def test_a_bam_redeflated_in_foreign_dialects_extracts_the_same(gpu_ctx, tmp_path):
    """3,000 short reads, inflated on the host and deflated again member by member (8 KiB of input each, so that no dialect passes a BGZF block) by the
    five small encoders of deflate_craft.dialect: fixed-Huffman literals, dynamic without a distance code, dynamic with one distance code, a block
    every 200 bytes cycling stored / fixed / dynamic with empty blocks between, and the 7 short + 256 fifteen-bit code.  BED12 and n_records must equal
    those of the zlib-deflated original."""
    from regtools_amd import synth
    orig = str(tmp_path / "zlib.bam")
    synth.write(orig, 3000, shape="short", seed=7)
    stream = bamio.inflate_all(orig)
    rc, want, je = gpu_extract(gpu_ctx, orig, ["-s", "XS"])
    assert rc == 0 and want.count(b"\n") > 5 and je.stats["n_records"] == 3000
    for name in dc.DIALECTS:
        path = str(tmp_path / (name + ".bam"))
        with open(path, "wb") as f:
            for k in range(0, len(stream), 8192):
                f.write(_bgzf_member(dc.dialect(name, stream[k:k + 8192]), stream[k:k + 8192]))
            f.write(bamio.EOF_MARKER)
        assert bamio.inflate_all(path) == stream                          # (before any GPU call on it)
        synth.index(path)
        rc, got, je2 = gpu_extract(gpu_ctx, path, ["-s", "XS"])
        assert rc == 0 and got == want and je2.stats["n_records"] == 3000, name
