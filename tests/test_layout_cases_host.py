"""No GPU: the builders of tests/layout_cases.py build what they claim (every claim is re-derived from the file's inflated bytes), and what the
GPU tests will expect stands on three legs before the device is asked: the oracle's BED12 has the digest the reference binary's had
(tests/golden/layout/layout_ref.json), and for every CIGAR of family A the device's serial core (tests/hostemu), the oracle's restatement
and the builder's prefix-sum form give the same four numbers per junction."""
import ctypes as C
import hashlib
import json
import os
import struct

import pytest

import bamio
import layout_cases as lc
from conftest import run_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "layout", "layout_ref.json")))


@pytest.fixture(scope="module")
def layout_dir(built, tmp_path_factory):
    return tmp_path_factory.mktemp("layout")


def parse(case):
    """(inflated bytes, header length, [(offset, record bytes)])"""
    data = bamio.inflate_all(case.path)
    contigs, recs = bamio.split_records(data)
    H = len(data) - sum(len(r) for r in recs)
    out, o = [], H
    for r in recs:
        out.append((o, r))
        o += len(r)
    return data, H, out


def fields(r):
    tid, pos = struct.unpack_from("<ii", r, 4)
    lq = r[12]
    fnc = struct.unpack_from("<I", r, 16)[0]
    l_seq = struct.unpack_from("<i", r, 20)[0]
    nc = fnc & 0xffff
    cig = [(c >> 4, c & 15) for c in struct.unpack_from("<%dI" % nc, r, 36 + lq)]
    aux = 36 + lq + 4 * nc + (l_seq + 1) // 2 + l_seq
    return dict(tid=tid, pos=pos, flag=fnc >> 16, ops=cig, name=r[36:36 + lq - 1].decode(), aux=r[aux:], aux_off=aux, cig_off=36 + lq)


def test_names_and_fixture_agree():
    assert sorted(GOLD) == lc.NAMES
    for name in lc.NAMES:
        assert sorted(GOLD[name]["runs"]) == sorted(" ".join(a) for a in lc.ARGS_B) or name.startswith("A_")


@pytest.mark.parametrize("name", lc.NAMES)
def test_builder_builds_what_it_claims(layout_dir, name):
    case = lc.build(name, layout_dir)
    data, H, recs = parse(case)
    assert H == case.header_len and len(recs) == case.n_records
    extra = b""
    if case.after:                                           # the FASTA's bases, as the builder digested them
        extra = b"".join(l.strip() for l in open(case.after[0], "rb") if not l.startswith(b">"))
    assert hashlib.sha256(data + extra).hexdigest() == case.digest == GOLD[name]["inputs_sha256"], "the builder drifted: regenerate the fixture"
    for args in case.arglists:
        assert case.planted[" ".join(args)] > 0
    # family A: every read is in the file as described, the claimed operations sit at the claimed indexes, loci are disjoint
    if case.reads:
        assert len(case.reads) == len(recs)
        spans = {}
        n_long = 0
        for rd, (o, r) in zip(case.reads, recs):
            f = fields(r)
            assert (f["tid"], f["pos"], f["ops"], f["name"]) == (rd["tid"], rd["pos"], [tuple(x) for x in rd["ops"]], rd["name"])
            for i, code in rd["claims"].items():
                assert f["ops"][i][1] == code, (rd["name"], i)
            assert all(op <= 9 for l, op in f["ops"])           # (the reference binary reads these files)
            spans.setdefault(f["tid"], []).append((f["pos"], f["pos"] + rd["span"]))
            n_long += len(f["ops"]) > lc.LONG_THRESHOLD and any(op == lc.N for l, op in f["ops"])
        for tid, sp in spans.items():
            sp.sort()
            assert all(a[1] < b[0] for a, b in zip(sp, sp[1:])), "two reads share a locus"
        if case.n_long is not None:
            assert n_long == case.n_long
    if name == "A_directed":
        by = {rd["name"]: rd for rd in case.reads}
        assert all(len(rd["ops"]) > lc.LONG_THRESHOLD for n_, rd in by.items() if n_ != "thr16") and len(by["thr16"]["ops"]) == lc.LONG_THRESHOLD
        assert by["edgeN_63"]["ops"][63][1] == lc.N and by["closer_HPB_D"]["ops"][64:68] == [(3, lc.H), (2, lc.P), (1, lc.B), (4, lc.D)]
        for n_ in (17, 64, 65, 128):
            assert by["lastN_%d" % n_]["ops"][-1][1] == lc.N and len(by["lastN_%d" % n_]["ops"]) == n_
        for n_ in (64, 65, 128, 200):
            ops = by["anchor_to_end_%d" % n_]["ops"]
            assert len(ops) == n_ and ops[60][1] == lc.N and all(op in (lc.M, lc.EQ) for l, op in ops[61:])
        ops = by["anchor_to_130"]["ops"]
        assert all(op in (lc.M, lc.EQ) for l, op in ops[61:130]) and ops[130][1] == lc.I
        for rd in case.reads:
            if rd["name"].startswith("carry_"):
                lb = min(rd["claims"])
                assert all(op in (lc.M, lc.EQ) for i, (l, op) in enumerate(rd["ops"]) if i not in rd["claims"]) and lb in (10, 63) and max(rd["claims"]) >= 64
        assert {op for l, op in by["zero_len_all"]["ops"] if l == 0} == set(range(10))
    if name == "A_generated":
        sizes = [len(rd["ops"]) for rd in case.reads]
        assert len(sizes) == 400 and min(sizes) >= 17 and max(sizes) <= 200 and {63, 64, 65, 127, 128, 129} <= set(sizes)
        ns = [l for rd in case.reads for l, op in rd["ops"] if op == lc.N]
        assert any(60 <= l < 70 for l in ns) and any(70 <= l <= 80 for l in ns) and any(19990 <= l <= 20000 for l in ns) and any(20000 < l <= 20010 for l in ns)
        assert {op for rd in case.reads for l, op in rd["ops"]} == set(range(10))
    if name.startswith("A_grid_"):
        longs = [rd for rd in case.reads if len(rd["ops"]) > lc.LONG_THRESHOLD]
        assert len(longs) == int(name[7:]) and len(case.reads) == len(longs) + len(longs) // 8
        for a, b in zip(longs, longs[1:]):
            ia, ib = [l for l, op in a["ops"] if op == lc.N], [l for l, op in b["ops"] if op == lc.N]
            assert a["pos"] != b["pos"] and a["tid"] != b["tid"] and a["ops"] != b["ops"] and len(ia) == len(ib) == 2 and not set(ia) & set(ib)
        tags = [fields(r)["aux"] for o, r in recs if len(fields(r)["ops"]) > lc.LONG_THRESHOLD]
        assert all(x != y for x, y in zip(tags, tags[1:]))
    # family B: record starts and ends lie where the builder aimed them
    for cl in case.claims:
        if "offset" in cl:
            o, r = recs[cl["index"]]
            f = fields(r)
            assert o == cl["offset"] and any(op == lc.N for l, op in f["ops"]) and f["aux"][-4:-1] == b"XSA"
        if cl["kind"] == "start_phase":
            assert (cl["seg_end"] - H) % lc.SEG == 0 and cl["seg_end"] - cl["offset"] == cl["d"] and (cl["offset"] - H) // lc.SEG == cl["seg"]
        elif cl["kind"] == "win_end":
            w1 = H + lc.SEG * cl["seg"] + lc.SEG + lc.TAIL
            assert w1 == cl["w1"] and (o - H) // lc.SEG == cl["seg"] and o + len(r) == w1 + cl["e"] and cl["in_win"] == (o + len(r) <= w1)
            assert f["aux"].startswith(b"ZBBC") == cl["b_array"]
            if cl["form"] == "cig":
                # the record ends `kN`, `9M`, [the B array,] the tag: without the array these are its last 12 bytes
                assert len(f["ops"]) == 280 and f["ops"][-2][1] == lc.N and len(r) - (f["cig_off"] + 4 * 278) == (320 if cl["b_array"] else 12)
        elif cl["kind"] == "covers":
            a = H + lc.SEG * cl["seg"]
            assert o < a and o + len(r) == cl["end"] and a + lc.SEG - 15 <= cl["end"] < a + lc.SEG and (cl["decoy_at"] - a) % 16 == 0
            assert data[cl["decoy_at"]:cl["decoy_at"] + len(lc.DECOY)] == lc.DECOY and cl["decoy_at"] + len(lc.DECOY) < cl["end"]
            assert set(data[a:cl["decoy_at"] - 8]) <= {0x11, 0xff}                # sequence and quality bytes: no block_size among them
        elif cl["kind"] == "seg_count":
            counts = lc.seg_counts([r for o, r in recs])
            assert counts == cl["counts"] and counts[cl["seg"]] % 8 == cl["mod8"] and counts[cl["seg"]] >= 435 and sum(len(r) == 37 for o, r in recs) >= 1990
        elif cl["kind"] == "stream_end":
            assert cl["index"] == len(recs) - 1 and len(data) - H == cl["stream_bytes"] == o + len(r) - H
    kinds = {cl["kind"] for cl in case.claims}
    n_seg = (len(data) - H + lc.SEG - 1) // lc.SEG
    if name.startswith(("B_start_phase", "B_align_", "B_sparse")):
        assert sorted(cl["d"] for cl in case.claims) == list(range(41)) and sum(cl["room_edge"] for cl in case.claims) == 15 and 40 <= n_seg <= 60
    if name.startswith("B_align_"):
        assert H % 16 == int(name[8:])
    if name.startswith("B_win_end_"):
        assert H % 16 == 0                     # (so that the staged window ends exactly at w1)
        assert [cl["e"] for cl in case.claims] == 2 * list(lc.WIN_END_E[name[10:]]) and {cl["form"] for cl in case.claims} == {name[10:]} and 40 <= n_seg <= 60
    if name == "B_room_edge":
        ph = [cl for cl in case.claims if cl["kind"] == "start_phase"]
        assert sorted(cl["d"] for cl in ph) == list(range(1, 16)) and all(cl["room"] == 15 for cl in ph) and 40 <= n_seg <= 60
    if name in ("B_start_phase", "B_room_edge") or name.startswith(("B_end_", "B_align_", "B_full_", "B_win_end_")):
        assert (len(data) - H) / len(recs) <= lc.SPARSE_MEAN           # the staged decode runs
    if name == "B_sparse":
        assert (len(data) - H) / len(recs) > lc.SPARSE_MEAN > lc.first_members_mean(case) > 0
    if name.startswith("B_end_"):
        total = len(data) - H
        want = {"exact": 0, "plus1": 1, "minus1": lc.SEG - 1}.get(name[6:])
        if want is not None:
            assert total % lc.SEG == want
        else:
            assert 0 < H + total // lc.SEG * lc.SEG - case.claims[0]["offset"] <= 40
    assert kinds or case.reads


def rows_of(bed):
    return [l.split(b"\t") for l in bed.splitlines()]


@pytest.mark.parametrize("name", lc.NAMES)
def test_oracle_has_the_reference_digest(layout_dir, name):
    case = lc.build(name, layout_dir)
    for args in case.arglists:
        key = " ".join(args)
        rc, out, err = run_oracle(case.argv(args))
        gold = GOLD[name]["runs"][key]
        print(name, key, "rows", out.count(b"\n"), "planted", case.planted[key], "reference rows", gold["rows"])
        assert rc == gold["rc"] == 0, err
        assert out.count(b"\n") == gold["rows"] and hashlib.sha256(out).hexdigest() == gold["sha256"], (name, key)
        assert gold["rows"] >= case.planted[key] > 0


def test_threshold_reads_give_the_same_rows_up_to_the_shift(layout_dir):
    """16 operations (the serial emitter), the same with 0H behind it and with 5H in front of it (17: the wave-per-read emitter)"""
    case = lc.build("A_directed", layout_dir)
    rds = {rd["name"]: rd for rd in case.reads if rd["name"].startswith("thr")}
    assert len({rd["tid"] for rd in rds.values()}) == 3 or len(rds) == 3
    for args in case.arglists:
        rows = rows_of(run_oracle(case.argv(args))[1])
        got = {}
        for n_, rd in rds.items():
            chrom = lc.CONTIGS[rd["tid"]][0].encode()
            mine = [r for r in rows if r[0] == chrom and rd["pos"] <= int(r[1]) <= rd["pos"] + rd["span"]]
            # the flag (and so the strand under RF) and the tag are the read's own: everything else, shifted
            got[n_] = [(int(r[1]) - rd["pos"], int(r[2]) - rd["pos"], r[4], r[9], r[10], r[11]) for r in mine]
        assert got["thr16"] == got["thr17_0H_behind"] == got["thr17_5H_front"] and len(got["thr16"]) == 2, (args, got)


def test_motif_reads_get_the_planted_verdicts(layout_dir):
    case = lc.build("A_motif", layout_dir)
    for args in case.arglists:
        rows = rows_of(run_oracle(case.argv(args))[1])
        for rd in case.reads:
            mine = sorted((int(r[1]), r[5].decode()) for r in rows if rd["pos"] <= int(r[1]) <= rd["pos"] + rd["span"])
            want = rd["verdicts"] if rd["tag"] == " " else rd["verdicts"].replace("?", rd["tag"])
            assert "".join(s for p, s in mine) == want, (args, rd["name"])


class Cand(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("thick_start", C.c_uint32), ("thick_end", C.c_uint32)]


@pytest.mark.parametrize("name", ["A_directed", "A_generated", "A_motif", "A_grid_8193"])
def test_three_cigar_walks_agree_on_family_a(built, layout_dir, name):
    emu = C.CDLL(os.path.join(ROOT, "tests", "hostemu", "libhostemu.so"))
    orc = C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    emu.emu_cigar_walk.argtypes = [C.c_int32, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(Cand), C.c_int]
    orc.orc_cigar_walk.argtypes = [C.c_int32, C.POINTER(C.c_uint32), C.c_int, C.POINTER(Cand), C.c_int]
    case = lc.build(name, layout_dir)
    a, b = (Cand * 256)(), (Cand * 256)()
    for rd in case.reads:
        ops = rd["ops"]
        arr = (C.c_uint32 * len(ops))(*[(l << 4) | o for l, o in ops])
        na = emu.emu_cigar_walk(rd["pos"], arr, len(ops), a, 256)
        nb = orc.orc_cigar_walk(rd["pos"], arr, len(ops), b, 256)
        mine = lc.walk(rd["pos"], ops)
        assert na == nb == len(mine) <= 256, rd["name"]
        for i in range(na):
            assert (a[i].start, a[i].end, a[i].thick_start, a[i].thick_end) == (b[i].start, b[i].end, b[i].thick_start, b[i].thick_end) == mine[i], (rd["name"], i)
