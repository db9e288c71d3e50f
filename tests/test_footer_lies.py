"""BGZF members whose footers / BSIZE do not say what the member is.  The reference never reads ISIZE (inflate_block, bgzf.c:292-316: a block is as
long as zlib says) and hands zlib block_length - 16 bytes, footer included, so a BSIZE that is one short still inflates.  The product
lays its arena out from the footers, notices when they lie, probes the true lengths and starts over: same rows as the reference."""
import os
import struct
import subprocess

import pytest

import bamio
from conftest import ROOT, run_oracle
from regtools_amd import synth

REF = os.path.join(ROOT, "oracle", "_ref", "regtools_ref")


def variants(tmp_path):
    """(name, path) of mutated copies of one synthetic BAM; the .bai stays valid (no byte moves)."""
    src = str(tmp_path / "src.bam")
    synth.write(src, 30000, shape="fuzz", seed=12)
    bam, bai = open(src, "rb").read(), open(src + ".bai", "rb").read()
    members = list(bamio.bgzf_members(bam))
    assert len(members) > 12
    out = []

    def emit(name, b):
        p = str(tmp_path / (name + ".bam"))
        open(p, "wb").write(bytes(b)); open(p + ".bai", "wb").write(bai)
        out.append((name, p))
    for name, mi, val in (("isize_zero", 5, 0), ("isize_plus1", 6, None), ("isize_minus1", 7, None), ("isize_64k1", 8, 65537), ("isize_ones", 9, 0xffffffff),
                          ("isize_small", 3, 1), ("isize_header_member", 0, 7)):
        coff, payload, isz = members[mi]
        b = bytearray(bam)
        v = val if val is not None else (isz + 1 if "plus" in name else isz - 1)
        struct.pack_into("<I", b, coff + 18 + len(payload) + 4, v)
        emit(name, b)
    b = bytearray(bam)                                         # every footer wrong
    for coff, payload, isz in members[:-1]:
        struct.pack_into("<I", b, coff + 18 + len(payload) + 4, (isz * 7 + 13) & 0xffff)
    emit("isize_all", b)
    # (a BSIZE 9 or more short cuts into the payload: upstream then feeds zlib two STALE bytes of its block buffer -- whatever an earlier,
    #  longer block left there -- so its output depends on buffer history; not restated, such a member simply fails here)
    for name, mi, delta in (("bsize_minus1", 4, -1), ("bsize_minus8", 6, -8), ("bsize_plus1", 5, 1)):
        coff, payload, isz = members[mi]
        b = bytearray(bam)
        struct.pack_into("<H", b, coff + 16, struct.unpack_from("<H", b, coff + 16)[0] + delta)
        emit(name, b)
    coff, payload, isz = members[-1]                           # the EOF marker claims to hold bytes
    b = bytearray(bam); struct.pack_into("<I", b, coff + 18 + len(payload) + 4, 300); emit("eof_marker_isize", b)
    return out


@pytest.mark.skipif(not os.path.exists(REF), reason="the real reference is only built where /root/reference exists")
def test_oracle_equals_reference_on_lying_footers(tmp_path):
    for name, p in variants(tmp_path):
        r = subprocess.run([REF, "junctions", "extract", "-s", "XS", "-o", str(tmp_path / "r.bed"), p], capture_output=True)
        rc, out, _ = run_oracle(["-s", "XS", p])
        assert (r.returncode != 0) == (rc != 0), name
        assert open(tmp_path / "r.bed", "rb").read() == out, name


@pytest.mark.gpu
def test_product_equals_oracle_on_lying_footers(gpu_ctx, tmp_path, monkeypatch, capfd):
    from test_gpu_parity import gpu_extract
    monkeypatch.setenv("REGTOOLS_AMD_TRACE", "1")
    whole = None
    for name, p in variants(tmp_path):
        for args in (["-s", "XS"], ["-s", "RF", "-a", "3"]):
            rc, out, je = gpu_extract(gpu_ctx, p, args)
            orc, exp, _ = run_oracle(args + [p])
            assert rc == orc and out == exp, (name, args)
        if name == "isize_all":
            whole = out
    assert whole and whole.count(b"\n") > 100                  # nothing was lost although no footer was right
    assert "footer mismatch: probing" in capfd.readouterr().err  # (the calls did start over with the probe's sizes: call_path.h footers_lie)


# ---- damage in front of a region: the iterator seeks past it (hts_itr_next -> bgzf_seek, hts.c:1935-1946) ---------------------------------------
REGIONS = ["10:1000-200000", "2:1-400000", "MT", "1:1-100000", "10:250000-260000"]


def damaged(tmp_path):
    """(name, path): one synthetic BAM (contigs 1, 10, 2, MT in file order) damaged in members that hold contig 1; index untouched and valid."""
    src = str(tmp_path / "dsrc.bam")
    synth.write(src, 30000, shape="fuzz", seed=21)
    bam, bai = open(src, "rb").read(), open(src + ".bai", "rb").read()
    members = list(bamio.bgzf_members(bam))
    out = []

    def emit(name, b):
        p = str(tmp_path / (name + ".bam"))
        open(p, "wb").write(bytes(b)); open(p + ".bai", "wb").write(bai)
        out.append((name, p))
    for name, mi, fn in (("payload_bit", 2, lambda b, c, pl: b.__setitem__(c + 18 + len(pl) // 2, b[c + 18 + len(pl) // 2] ^ 0x10)),
                         ("magic", 2, lambda b, c, pl: b.__setitem__(c + 1, 0)),
                         ("bsize_big", 3, lambda b, c, pl: struct.pack_into("<H", b, c + 16, struct.unpack_from("<H", b, c + 16)[0] + 300)),
                         ("bsize_small", 1, lambda b, c, pl: struct.pack_into("<H", b, c + 16, 40)),
                         ("isize_and_payload", 2, lambda b, c, pl: (struct.pack_into("<I", b, c + 18 + len(pl) + 4, 5), b.__setitem__(c + 30, b[c + 30] ^ 0xff)))):
        coff, payload, isz = members[mi]
        b = bytearray(bam); fn(b, coff, payload); emit(name, b)
    return out


@pytest.mark.skipif(not os.path.exists(REF), reason="the real reference is only built where /root/reference exists")
def test_oracle_seeks_like_the_reference_on_damaged_files(tmp_path):
    n_rows = 0
    for name, p in damaged(tmp_path):
        for reg in REGIONS + [None]:
            args = ["-s", "XS"] + (["-r", reg] if reg else [])
            r = subprocess.run([REF, "junctions", "extract"] + args + ["-o", str(tmp_path / "r.bed"), p], capture_output=True)
            if r.returncode not in (0, 1):
                continue                                  # the reference itself died on this input
            rc, out, _ = run_oracle(args + [p])
            assert (r.returncode != 0) == (rc != 0), (name, reg)
            if rc == 0:
                assert open(tmp_path / "r.bed", "rb").read() == out, (name, reg)
                n_rows += out.count(b"\n")
    assert n_rows > 200                                    # the regions behind the damage were really read


@pytest.mark.gpu
def test_product_seeks_like_the_oracle_on_damaged_files(gpu_ctx, tmp_path):
    from test_gpu_parity import gpu_extract
    n_rows = 0
    for name, p in damaged(tmp_path):
        for reg in REGIONS + [None]:
            args = ["-s", "XS"] + (["-r", reg] if reg else [])
            rc, out, _ = gpu_extract(gpu_ctx, p, args)
            orc, exp, _ = run_oracle(args + [p])
            assert rc == orc and out == exp, (name, reg)
            n_rows += out.count(b"\n")
    assert n_rows > 200


def unreadable_in_the_last_piece(tmp_path):
    """One file of a few dozen members (contigs 1, 10, 2 in file order) in which a member of contig 2 does not inflate: its first DEFLATE block
    claims the reserved type 3.  Host bytes of this size go up in three ungated pieces that end at 33 % and 67 % of the file (front_plan.h
    plan_upload_chunks), and the members of a range are launched piece by piece (plan_pieces).  The range of `-r 2` begins in front of the second
    cut, and the member that fails lies behind it: in a launch whose members count from the piece's begin, not from the range's."""
    import zlib
    src = str(tmp_path / "usrc.bam")
    synth.write(src, 16000, shape="fuzz", seed=21)
    bam, bai = open(src, "rb").read(), open(src + ".bai", "rb").read()
    members = list(bamio.bgzf_members(bam))
    assert 24 <= len(members) <= 48 and len(bam) < 2 * 4096 * 64          # (below that size REGTOOLS_AMD_OVERLAP="0,64" does not gate the launch)
    inflated = bamio.inflate_all(src)
    (l_text,) = struct.unpack_from("<i", inflated, 4)
    (n_ref,) = struct.unpack_from("<i", inflated, 8 + l_text)
    o = 12 + l_text
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", inflated, o)[0]
    starts, u = [], 0
    for _, _, isz in members:
        starts.append(u); u += isz
    tids = [set() for _ in members]                              # the contigs of the records that start in each member
    k = 0
    while o + 36 <= len(inflated):
        bs, tid = struct.unpack_from("<ii", inflated, o)
        while k + 1 < len(members) and starts[k + 1] <= o:
            k += 1
        tids[k].add(tid); o += 4 + bs
    cut = (len(bam) * 67 // 100 + 4095) & ~4095                  # where the second piece of the upload ends
    target = min(i for i, t in enumerate(tids) if 2 in t)        # the seek of `-r 2` lands in this member: the range's first
    t_off, t_payload, _ = members[target]
    assert target > 4 and t_off + 18 + len(t_payload) + 16 <= cut, "the range's first member must arrive with the second piece"
    behind = [i for i, t in enumerate(tids) if t == {2} and members[i][0] > cut]
    d = behind[len(behind) // 2]
    assert behind[0] < d < behind[-1]
    coff, payload, isz = members[d]
    b = bytearray(bam); b[coff + 18] |= 0x06                     # BFINAL / BTYPE are the first three bits of the stream
    try:
        zlib.decompressobj(-15).decompress(bytes(b[coff + 18: coff + 18 + len(payload)]))
        raise AssertionError("the damaged member still inflates")
    except zlib.error:
        pass
    p = str(tmp_path / "unreadable.bam")
    open(p, "wb").write(bytes(b)); open(p + ".bai", "wb").write(bai)
    return p, src


@pytest.mark.gpu
def test_member_that_does_not_inflate_in_a_later_piece_of_the_upload(gpu_ctx, tmp_path):
    """What a member that did not inflate reports carries its index in the call's range (kernels.hip report_bad_member): a piece's launch adds
    where the piece begins (index_bias).  A region query reads that index -- its record stream ends where the member starts -- so `-r 2` over
    unreadable_in_the_last_piece's file gives the oracle's rows only when the index is right: fewer rows than the sound file gives, more than
    none.  Read from the file, and from host bytes that go up in pieces (a child process lowers the threshold); the whole-file read beside it."""
    import json
    import sys
    from test_gpu_parity import gpu_extract
    from test_gpu_gate import CHILD
    p, sound = unreadable_in_the_last_piece(tmp_path)
    jobs, want = [], []
    for reg in ("2", None):
        args = ["-s", "XS"] + (["-r", reg] if reg else [])
        orc, exp, _ = run_oracle(args + [p])
        full = run_oracle(args + [sound])[1]
        assert orc == 0 and 20 < exp.count(b"\n") < full.count(b"\n") - 20, reg      # (the stream ends at the member: rows in front of it, none behind)
        rc, out, _ = gpu_extract(gpu_ctx, p, args)
        assert rc == orc and out == exp, reg
        jobs.append(dict(bam=p, kw=dict(strandness=0, **({"region": reg} if reg else {}))))
        want.append(exp)
    jf, of = str(tmp_path / "jobs.json"), str(tmp_path / "out.json")
    json.dump(jobs, open(jf, "w"))
    env = dict(os.environ, REGTOOLS_AMD_OVERLAP="0,64", REGTOOLS_AMD_TRACE="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD, jf, of], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"first chunk enqueued" in r.stderr and b"gated" not in r.stderr, "the calls did not go up in ungated pieces:\n" + r.stderr.decode()[-2000:]
    # (the whole-file read is speculative: the failed member makes it start over device-resident)
    assert b"inflate verdict: not clean" in r.stderr, "no launch met the member that does not inflate:\n" + r.stderr.decode()[-2000:]
    for exp, res in zip(want, json.load(open(of))):
        for one in res:
            assert one["rc"] == 0 and one["bed"].encode("latin1") == exp


def from_host_bytes_in_pieces(tmp_path, bam, regions):
    """The file read once per region from page-locked host bytes that go up in ungated pieces behind the host's member scan (a child process lowers
    the threshold), traced: (the child's stderr, the oracle's answers, the product's)."""
    import json
    import sys
    from test_gpu_gate import CHILD
    jobs = [dict(bam=bam, kw=dict(strandness=0, **({"region": reg} if reg else {}))) for reg in regions]
    want = [run_oracle(["-s", "XS"] + (["-r", reg] if reg else []) + [bam]) for reg in regions]
    jf, of = str(tmp_path / "jobs.json"), str(tmp_path / "out.json")
    json.dump(jobs, open(jf, "w"))
    env = dict(os.environ, REGTOOLS_AMD_OVERLAP="0,64", REGTOOLS_AMD_TRACE="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD, jf, of], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"first chunk enqueued" in r.stderr and b"host member scan" in r.stderr, "the calls did not go up in pieces:\n" + r.stderr.decode()[-2000:]
    return r.stderr, want, json.load(open(of))


@pytest.mark.gpu
def test_index_whose_first_offset_is_no_member_of_a_sound_file(gpu_ctx, tmp_path):
    """A sound file whose header member was written again, stored instead of compressed, after the file was indexed: the host's member scan vouches
    for it, and the offset at which the index says the records begin lies inside the new first member.  The call that found its members on the host
    starts over device-resident, where the discovery kernels judge the offset (bgzf_seek goes there; the read behind it fails): the oracle's answer
    from host bytes as from the file."""
    import zlib
    from test_gpu_parity import gpu_extract
    src = str(tmp_path / "hsrc.bam")
    synth.write(src, 16000, shape="fuzz", seed=21)
    bam, bai = open(src, "rb").read(), open(src + ".bai", "rb").read()
    coff, payload, isz = next(iter(bamio.bgzf_members(bam)))
    old_len = struct.unpack_from("<H", bam, 16)[0] + 1
    stored = bamio.bgzf_member(zlib.decompress(payload, -15), level=0)
    assert coff == 0 and len(stored) > old_len + 64                    # the index's first offset (old_len << 16) now lies inside member 0
    p = str(tmp_path / "stale_header.bam")
    open(p, "wb").write(stored + bam[old_len:]); open(p + ".bai", "wb").write(bai)
    assert len(bamio.inflate_all(p)) == len(bamio.inflate_all(src))     # (still one sound chain of members)
    stderr, want, got = from_host_bytes_in_pieces(tmp_path, p, [None, "2"])
    assert b"index points at no member" in stderr, "the host scan's list held the index's first offset:\n" + stderr.decode()[-2000:]
    for (orc, exp, _), res, reg in zip(want, got, (None, "2")):
        rc, out, _ = gpu_extract(gpu_ctx, p, ["-s", "XS"] + (["-r", reg] if reg else []))
        assert (rc != 0) == (orc != 0) and out == exp, reg
        for one in res:
            assert (one["rc"] != 0) == (orc != 0) and one["bed"].encode("latin1") == exp, reg


@pytest.mark.gpu
def test_member_that_does_not_inflate_in_front_of_a_read_with_nothing_to_frame(gpu_ctx, tmp_path):
    """`-r "*"` on a file without unplaced reads seeks behind the last record: nothing is framed, so the speculative launch's verdict is read on its
    own.  A file of a handful of members is inflated from its first member on (the header's sake), and one of them, in front of the seek's target,
    does not inflate: the call starts over device-resident and answers what the oracle answers."""
    import zlib
    from test_gpu_parity import gpu_extract
    src = str(tmp_path / "nsrc.bam")
    synth.write(src, 700, shape="short", seed=21)                   # (reads on the last contig, none unplaced: the index knows where they end)
    bam, bai = open(src, "rb").read(), open(src + ".bai", "rb").read()
    members = list(bamio.bgzf_members(bam))
    assert 4 <= len(members) <= 5, len(members)                        # header, two or three of records, the EOF marker: the range starts at member 0
    assert run_oracle(["-s", "XS", "-r", "*", src])[:2] == (0, b"")
    coff, payload, isz = members[2]
    b = bytearray(bam); b[coff + 18] |= 0x06                            # the reserved block type, as above
    with pytest.raises(zlib.error):
        zlib.decompressobj(-15).decompress(bytes(b[coff + 18: coff + 18 + len(payload)]))
    p = str(tmp_path / "unreadable_small.bam")
    open(p, "wb").write(bytes(b)); open(p + ".bai", "wb").write(bai)
    stderr, want, got = from_host_bytes_in_pieces(tmp_path, p, ["*"])
    assert b"not clean, nothing framed" in stderr, "the read framed something, or met no bad member:\n" + stderr.decode()[-2000:]
    (orc, exp, _), res = want[0], got[0]
    rc, out, _ = gpu_extract(gpu_ctx, p, ["-s", "XS", "-r", "*"])
    assert (rc != 0) == (orc != 0) and out == exp
    for one in res:
        assert (one["rc"] != 0) == (orc != 0) and one["bed"].encode("latin1") == exp
    # (the same file read whole ends at the member, with rows in front of it)
    orc_w, exp_w, _ = run_oracle(["-s", "XS", p])
    rc_w, out_w, _ = gpu_extract(gpu_ctx, p, ["-s", "XS"])
    assert rc_w == orc_w == 0 and out_w == exp_w and exp_w.count(b"\n") > 5


# ---- a seek target that does not exist (file truncated in front of the region): empty result, and nothing may be written for the member the
#      end of the file cuts off (its claimed size is ~0; handing that to the decoder as an output capacity was a GPU memory fault) -------------
def truncated(tmp_path):
    src = str(tmp_path / "tsrc.bam")
    synth.write(src, 30000, shape="short", seed=33)
    bam, bai = open(src, "rb").read(), open(src + ".bai", "rb").read()
    members = list(bamio.bgzf_members(bam))
    out = []
    for name, cut in (("after_header_member", members[1][0] + 700), ("mid_third_member", members[2][0] + 100), ("at_member_boundary", members[3][0]),
                      ("inside_header", 90)):
        p = str(tmp_path / (name + ".bam"))
        open(p, "wb").write(bam[:cut]); open(p + ".bai", "wb").write(bai)
        out.append((name, p))
    return out


T_REGIONS = ["chr2:1-90000000", "chr1:1-50000", "chr22", None]


@pytest.mark.skipif(not os.path.exists(REF), reason="the real reference is only built where /root/reference exists")
def test_oracle_equals_reference_on_truncated_files_with_regions(tmp_path):
    for name, p in truncated(tmp_path):
        for reg in T_REGIONS:
            args = ["-s", "XS"] + (["-r", reg] if reg else [])
            r = subprocess.run([REF, "junctions", "extract"] + args + ["-o", str(tmp_path / "r.bed"), p], capture_output=True)
            if r.returncode not in (0, 1):
                continue
            rc, out, _ = run_oracle(args + [p])
            assert (r.returncode != 0) == (rc != 0), (name, reg)
            if rc == 0:
                assert open(tmp_path / "r.bed", "rb").read() == out, (name, reg)


@pytest.mark.gpu
def test_product_survives_truncated_files_with_regions(gpu_ctx, tmp_path):
    from test_gpu_parity import gpu_extract
    for name, p in truncated(tmp_path):
        for reg in T_REGIONS:
            args = ["-s", "XS"] + (["-r", reg] if reg else [])
            rc, out, _ = gpu_extract(gpu_ctx, p, args)
            orc, exp, _ = run_oracle(args + [p])
            assert rc == orc and out == exp, (name, reg)
        for g in range(3):                                   # and cut into shards (each shard a seek)
            rc, _, _ = gpu_extract(gpu_ctx, p, ["-s", "XS"], shard=g, n_shards=3)
            assert rc in (0, 1)


@pytest.mark.gpu
def test_shards_of_a_damaged_file_merge_to_the_single_pass(gpu_ctx, tmp_path):
    """A later shard is a seek past the damage; a sequential reader never gets there.  Every shard reports whether its record stream ended
    (stream_ended) and the merge ignores the shards behind the first that did: same table whatever the shard count."""
    from test_gpu_parity import gpu_extract
    from regtools_amd import distributed
    n = 0
    for name, p in damaged(tmp_path) + truncated(tmp_path)[:3]:
        rc, single, _ = gpu_extract(gpu_ctx, p, ["-s", "XS"])
        if rc != 0:
            continue
        assert single == run_oracle(["-s", "XS", p])[1], name
        for G in (2, 3, 7):
            parts, keep = [], []
            for g in range(G):
                rc, _, je = gpu_extract(gpu_ctx, p, ["-s", "XS"], shard=g, n_shards=G)
                assert rc == 0, (name, G, g)
                keep.append(je); parts.append(distributed.pack_table(je.table))
            merged = distributed.merge_packed(parts, keep[0].table, 8, [k.stats["stream_ended"] for k in keep])
            assert merged.bed12() == single, (name, G)
            n += 1
    assert n >= 15


# ---- a record whose block_size keeps the chain whole and whose other head fields cannot be believed (round 6: a GPU memory fault found by
#      tools/fuzz/gpu_corrupt_bam.py).  The framing follows block_size only; the decode pass meets the record, tells the host (which starts over with
#      the framing that makes bam_read1's full test, sam.c:421-423) -- and until then must not follow the record's own numbers: a negative l_seq puts
#      the aux walk of `-s XS` far in front of the arena, an n_cigar of 65,535 runs 256 KiB past a small arena's end ----------------------------------
def unbelievable_heads(tmp_path):
    import struct
    import bamio
    out = []
    base = str(tmp_path / "heads_base.bam")
    from regtools_amd import synth
    synth.write(base, 150, shape="long", seed=5)
    raw = bytearray(bamio.inflate_all(base))
    (l_text,) = struct.unpack_from("<i", raw, 4)
    (n_ref,) = struct.unpack_from("<i", raw, 8 + l_text)
    o = 12 + l_text
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", raw, o); o += 8 + ln
    recs = []
    while o + 36 <= len(raw):
        (bs,) = struct.unpack_from("<i", raw, o)
        recs.append(o); o += 4 + bs
    spliced = [r for r in recs if struct.unpack_from("<H", raw, r + 16)[0] > 1]
    bai = open(base + ".bai", "rb").read()
    # (the index names the first record's place: the header's member stays as it is, the records behind it are packed again)
    whole = open(base, "rb").read()
    first = next(iter(bamio.bgzf_members(whole)))
    head_bytes, head_len = whole[:struct.unpack_from("<H", whole, 16)[0] + 1], first[2]
    assert head_len <= recs[0]
    for name, at, field, value in (("negative_l_seq", spliced[len(spliced) // 2], 20, -0x40000000), ("l_seq_most_negative", spliced[-1], 20, -0x80000000),
                                   ("n_cigar_65535_in_the_last_record", recs[-1], 16, None), ("l_read_name_0", spliced[3], 12, None)):
        b = bytearray(raw)
        if field == 20: struct.pack_into("<i", b, at + 20, value)
        elif field == 16: struct.pack_into("<H", b, at + 16, 65535)
        else: b[at + 12] = 0
        p = str(tmp_path / (name + ".bam"))
        assert bytes(b[:head_len]) == bytes(raw[:head_len])
        blob = head_bytes + b"".join(bamio.bgzf_member(bytes(b[k:k + 0xff00])) for k in range(head_len, len(b), 0xff00)) + bamio.EOF_MARKER
        open(p, "wb").write(blob); open(p + ".bai", "wb").write(bai)
        out.append((name, p))
    return out


def test_oracle_equals_reference_on_unbelievable_heads(tmp_path):
    if not os.path.exists(REF):
        pytest.skip("the reference binary lives in the dev container")
    for name, p in unbelievable_heads(tmp_path):
        r = subprocess.run([REF, "junctions", "extract", "-s", "XS", "-o", str(tmp_path / "r.bed"), p], capture_output=True, timeout=60)
        rc, out, _ = run_oracle(["-s", "XS", p])
        assert r.returncode in (0, 1) and (r.returncode != 0) == (rc != 0), name
        if rc == 0:
            assert open(tmp_path / "r.bed", "rb").read() == out, name


@pytest.mark.gpu
def test_product_does_not_follow_unbelievable_heads(gpu_ctx, tmp_path, monkeypatch, capfd):
    from test_gpu_parity import gpu_extract
    monkeypatch.setenv("REGTOOLS_AMD_TRACE", "1")
    rows = 0
    for name, p in unbelievable_heads(tmp_path):
        for args in (["-s", "XS"], ["-s", "RF", "-a", "3"]):
            rc, out, _ = gpu_extract(gpu_ctx, p, args)
            orc, exp, _ = run_oracle(args + [p])
            assert rc == orc and out == exp, (name, args)
            rows += out.count(b"\n")
    assert rows > 100
    assert "a record fails bam_read1's test, starting over" in capfd.readouterr().err      # (call_path.h record_fails_full_test)
