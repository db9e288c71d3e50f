"""The decode rule (bam_core.h record_row, compiled for the host by tests/hostemu as emu_record_row) against a plain restatement of what the
reference does with one record, written from its functions (file:line relative to the reference tree, as in bam_core.h):

  src/utils/htslib/hts.c:1950-1960   hts_itr_next: the first record with another tid or with pos >= end finishes the iteration; a record is
                                     returned when end > iter->beg and iter->end > beg
  src/utils/htslib/sam.c:544-554     bam_readrec: beg = pos, end = bam_endpos
  src/utils/htslib/sam.c:336-342     bam_endpos
  src/utils/htslib/sam.c:1233-1266   skip_aux / bam_aux_get: a field of a type aux_type2size (:344-360) does not know abort()s the process
  src/utils/htslib/sam.c:1301-1307   bam_aux2A
  src/junctions/junctions_extractor.cc:377-497  parse_alignment_into_junctions: n_cigar <= 1 returns; the barcode tag (-b) is asked for
                                     first (:393-395), then every junction the CIGAR walk closes asks for its strand (:415 / :447 / :467 / :490)
                                     in front of junction_qc (:160-170, reached through add_junction)
  src/junctions/junctions_extractor.cc:283-322  set_junction_strand_XS / set_junction_strand_flag

No GPU needed.  Records come from bamio; hypothesis drives the inputs and a directed list names the rule's edges, each of which asserts in the
restatement that it reaches its branch."""
import ctypes as C
import os
import struct

import pytest
from hypothesis import given, settings, strategies as st

import bamio
from conftest import run_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HCC = os.path.join(ROOT, "tests", "golden", "test_hcc1395.bam")


class Cfg(C.Structure):
    _fields_ = [("n_ref", C.c_int32), ("strandness", C.c_int32), ("tag0", C.c_uint8), ("tag1", C.c_uint8), ("bc0", C.c_uint8), ("bc1", C.c_uint8),
                ("min_intron", C.c_uint32), ("max_intron", C.c_uint32), ("region_tid", C.c_int32), ("region_beg", C.c_int32), ("region_end", C.c_int32),
                ("long_threshold", C.c_uint32), ("stop_index", C.c_uint32), ("stop_on", C.c_int32), ("abort_on", C.c_int32), ("odd_on", C.c_int32)]


class Row(C.Structure):
    _fields_ = [("in_region", C.c_int32), ("stop_candidate", C.c_int32), ("is_long", C.c_int32), ("abort_read", C.c_int32), ("odd_read", C.c_int32),
                ("strand", C.c_int32), ("nev", C.c_uint32)]


ROW_FIELDS = [f for f, _ in Row._fields_]


@pytest.fixture(scope="module")
def emu(built):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostemu", "libhostemu.so"))
    lib.emu_record_row.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.POINTER(Cfg), C.POINTER(Row)]
    return lib


def cfg(**kw):
    """the tool's defaults (-s XS, -m 70, -M 500000, whole file, no -b, long_threshold 16), changed by kw"""
    d = dict(n_ref=3, strandness=0, tag=b"XS", bc=None, min_intron=70, max_intron=500000, region_tid=-2, region_beg=0, region_end=0x7fffffff,
             long_threshold=16, stop_index=0xffffffff, stop_on=False, abort_on=False, odd_on=False)
    assert set(kw) <= set(d), kw
    d.update(kw)
    return d


def emu_row(lib, rec, i, c):
    bc = c["bc"] or b"\0\0"
    cc = Cfg(c["n_ref"], c["strandness"], c["tag"][0], c["tag"][1], bc[0], bc[1], c["min_intron"], c["max_intron"], c["region_tid"], c["region_beg"],
             c["region_end"], c["long_threshold"], c["stop_index"], int(c["stop_on"]), int(c["abort_on"]), int(c["odd_on"]))
    out = Row()
    assert lib.emu_record_row(rec, len(rec), i, C.byref(cc), C.byref(out)) == 0
    return {f: getattr(out, f) for f in ROW_FIELDS}


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
AUX_SIZE = {ord(t): n for ts, n in (("AcC", 1), ("sS", 2), ("iIf", 4), ("d", 8)) for t in ts}     # sam.c:344-360 (Z, H, B: by their own rule)
REF_OPS = (0, 2, 3, 7, 8)                                                                          # M D N = X consume the reference


def aux_get(aux, tag):
    """bam_aux_get: ("found", offset of the type byte) / ("none",) / ("abort",)"""
    s = 0
    while s < len(aux):
        name = aux[s:s + 2]
        s += 2
        if name == tag:
            return ("found", s)
        t = aux[s]
        s += 1
        if t in b"ZH":
            while aux[s]:
                s += 1
            s += 1
        elif t == ord("B"):
            n = struct.unpack_from("<I", aux, s + 1)[0]
            s += 5 + AUX_SIZE.get(aux[s], 0) * n
        elif t in AUX_SIZE:
            s += AUX_SIZE[t]
        else:
            return ("abort",)
    return ("none",)


def restate(rec, i, c, reached=None):
    """One record of the file, the i-th: what the reference's loop does with it, in the row's terms.  `reached` collects the branches taken."""
    reached = set() if reached is None else reached
    block_len, tid, pos, x2, x3, l_seq = struct.unpack_from("<iiiIIi", rec, 0)
    l_qname, n_cigar, flag = x2 & 0xff, x3 & 0xffff, x3 >> 16
    cigar = [(w & 15, w >> 4) for w in struct.unpack_from("<%dI" % n_cigar, rec, 36 + l_qname)]
    aux = rec[36 + l_qname + 4 * n_cigar + (l_seq + 1) // 2 + l_seq:]
    row = dict(in_region=1, stop_candidate=0, is_long=0, abort_read=0, odd_read=0, strand=ord("?"), nev=0)
    # the iterator
    if c["region_tid"] != -2:
        past = tid != c["region_tid"] or pos >= c["region_end"]
        returned = not past
        if c["stop_on"]:
            if i >= c["stop_index"]:
                reached.add("behind_stop")
                returned = False                          # the iteration has finished in front of this record
            elif past:
                reached.add("stop_candidate")
                row["stop_candidate"] = 1
        if returned:
            if not (flag & 4) and n_cigar > 0:
                reached.add("endpos_cigar")
                end = pos + sum(l for o, l in cigar if o in REF_OPS)
            else:
                reached.add("endpos_plus_one")
                end = pos + 1
            returned = end > c["region_beg"]
            reached.add("overlaps" if returned else "ends_in_front")
        elif past:
            reached.add("past_region")
        row["in_region"] = int(returned)
    if not row["in_region"]:
        return row
    # parse_alignment_into_junctions
    if n_cigar <= 1:
        reached.add("one_op")
        return row
    if not 0 <= tid < c["n_ref"]:
        reached.add("no_contig")                          # (target_name[tid] does not exist: such a read gives no junction)
        return row
    aborts = False
    if c["bc"] and c["abort_on"]:
        got = aux_get(aux, c["bc"])
        reached.add("bc_" + got[0])
        aborts = got[0] == "abort"
    n_lens = [l for o, l in cigar if o == 3]
    row["nev"] = sum(1 for l in n_lens if not (l < c["min_intron"] or l > c["max_intron"]))
    # every N operation closes a junction that asks for its strand, junction_qc comes behind.  The row of a read without an event is read by nobody:
    # it carries what the tag walk said where one was made for the abort's or the count's sake, '?' otherwise.
    if row["nev"] or (n_lens and c["strandness"] == 0 and (c["abort_on"] or c["odd_on"])):
        if not row["nev"]:
            reached.add("asked_without_event")
        if c["strandness"] == 0:
            got = aux_get(aux, c["tag"])
            reached.add("tag_" + got[0])
            if got[0] == "found" and aux[got[1]] == ord("A") and aux[got[1] + 1] != 0:
                row["strand"] = aux[got[1] + 1]
            if got[0] == "abort":
                aborts = aborts or bool(c["abort_on"])
                if c["odd_on"]:
                    row["odd_read"] = 1
                    row["strand"] |= 0x80
        else:
            rev, mrev, r1, r2 = (flag >> 4) & 1, (flag >> 5) & 1, (flag >> 6) & 1, (flag >> 7) & 1
            nb = int(not (c["strandness"] - 1))
            first, second = nb ^ r1 ^ rev, nb ^ r2 ^ mrev
            row["strand"] = ord("?") if first != second else ord("+") if first else ord("-")
            reached.add("flag_rule")
        if row["nev"] and n_cigar > c["long_threshold"]:
            reached.add("long")
            row["is_long"] = 1
    row["abort_read"] = int(aborts)
    return row


# ---- directed cases ------------------------------------------------------------------------------------------------------------------------
ODD = b"ZZq\x01\x02\x03"                                   # tag ZZ, type 'q': no such type
B_ARRAY = b"YBBS" + struct.pack("<I", 3) + b"\1\0\2\0\3\0"
XS = bamio.tagA("XS", "-")
CB = bamio.tagZ("CB", "ACGT")
SPLICED = "20M100N20M"


def rec(tid=0, pos=1000, cigar=SPLICED, flag=0, aux=XS, **kw):
    return bamio.record(tid, pos, cigar, flag=flag, aux=aux, **kw)


def directed_cases():
    """(name, record, row index, cfg, branches the restatement must reach, fields the row must have)"""
    out = []

    def add(name, r, c, reach, expect, i=5):
        out.append(pytest.param(r, i, c, reach, expect, id=name))

    # tid of -1, n_ref - 1, n_ref
    add("tid_minus_one", rec(tid=-1), cfg(), {"no_contig"}, dict(nev=0, in_region=1))
    add("tid_last", rec(tid=2), cfg(), {"tag_found"}, dict(nev=1, strand=ord("-")))
    add("tid_n_ref", rec(tid=3), cfg(), {"no_contig"}, dict(nev=0))
    # one CIGAR operation against two
    add("one_op", rec(cigar="100N"), cfg(), {"one_op"}, dict(nev=0))
    add("two_ops", rec(cigar="100N20M"), cfg(), {"tag_found"}, dict(nev=1))
    # an N at the intron limits
    for ln, nev in ((69, 0), (70, 1), (500000, 1), (500001, 0)):
        add("intron_%d" % ln, rec(cigar="20M%dN20M" % ln), cfg(), {"tag_found"} if nev else set(), dict(nev=nev))
    # endpos against region_beg; pos against region_end (the read covers [1000, 1140))
    add("endpos_eq_beg", rec(), cfg(region_tid=0, region_beg=1140, region_end=5000), {"endpos_cigar", "ends_in_front"}, dict(in_region=0, nev=0))
    add("endpos_eq_beg_plus_1", rec(), cfg(region_tid=0, region_beg=1139, region_end=5000), {"endpos_cigar", "overlaps"}, dict(in_region=1, nev=1))
    add("pos_eq_end_minus_1", rec(), cfg(region_tid=0, region_beg=0, region_end=1001), {"overlaps"}, dict(in_region=1, nev=1))
    add("pos_eq_end", rec(), cfg(region_tid=0, region_beg=0, region_end=1000), {"past_region"}, dict(in_region=0, nev=0, stop_candidate=0))
    add("pos_eq_end_stop_on", rec(), cfg(region_tid=0, region_beg=0, region_end=1000, stop_on=True), {"stop_candidate"}, dict(in_region=0, stop_candidate=1))
    add("other_tid_stop_on", rec(tid=1), cfg(region_tid=0, region_beg=0, region_end=5000, stop_on=True), {"stop_candidate"}, dict(in_region=0, stop_candidate=1))
    # an unmapped-flagged read with a CIGAR: its end is pos + 1
    add("unmapped_in_front", rec(flag=4), cfg(region_tid=0, region_beg=1001, region_end=5000), {"endpos_plus_one", "ends_in_front"}, dict(in_region=0))
    add("unmapped_inside", rec(flag=4), cfg(region_tid=0, region_beg=1000, region_end=5000), {"endpos_plus_one", "overlaps"}, dict(in_region=1, nev=1))
    # the row index against stop_index
    add("index_stop_minus_1", rec(), cfg(region_tid=0, region_beg=0, region_end=5000, stop_on=True, stop_index=6), {"overlaps"}, dict(in_region=1, nev=1))
    add("index_eq_stop", rec(), cfg(region_tid=0, region_beg=0, region_end=5000, stop_on=True, stop_index=5), {"behind_stop"}, dict(in_region=0, nev=0, stop_candidate=0))
    add("index_eq_stop_past", rec(tid=1), cfg(region_tid=0, region_beg=0, region_end=5000, stop_on=True, stop_index=5), {"behind_stop"}, dict(in_region=0, stop_candidate=0))
    # n_cigar against long_threshold
    add("n_cigar_eq_threshold", rec(cigar="20M100N20M"), cfg(long_threshold=3), {"tag_found"}, dict(nev=1, is_long=0))
    add("n_cigar_threshold_plus_1", rec(cigar="20M100N10M5S"), cfg(long_threshold=3), {"long"}, dict(nev=1, is_long=1))
    add("long_without_event", rec(cigar="20M10N10M1I10M"), cfg(long_threshold=3, abort_on=True), {"asked_without_event"}, dict(nev=0, is_long=0))
    # an aux field of unknown type in front of the strand tag, behind it, without one; the same for the barcode tag
    for where, aux, walk in (("front", ODD + XS, "abort"), ("behind", XS + ODD, "found"), ("alone", ODD, "abort"), ("b_array", B_ARRAY + XS, "found"), ("none", b"", "none")):
        for abort_on in (False, True):
            for odd_on in (False, True):
                strand = ord("-") if walk == "found" else ord("?") | (0x80 if walk == "abort" and odd_on else 0)
                add("strand_tag_%s_abort%d_odd%d" % (where, abort_on, odd_on), rec(aux=aux), cfg(abort_on=abort_on, odd_on=odd_on), {"tag_" + walk},
                    dict(nev=1, abort_read=int(walk == "abort" and abort_on), odd_read=int(walk == "abort" and odd_on), strand=strand))
    for where, aux, walk in (("front", ODD + CB + XS, "abort"), ("behind", CB + XS + ODD, "found"), ("alone", XS + ODD, "abort"), ("b_array", B_ARRAY + CB + XS, "found"), ("none", XS, "none")):
        for abort_on in (False, True):
            # (XS in front of the odd field: only the barcode walk meets it; behind it, the strand walk does too)
            add("barcode_tag_%s_abort%d" % (where, abort_on), rec(aux=aux), cfg(bc=b"CB", abort_on=abort_on), {"bc_" + walk} if abort_on else set(),
                dict(nev=1, abort_read=int(walk == "abort" and abort_on)))
    add("barcode_asked_without_n", rec(cigar="20M5D20M", aux=ODD + CB), cfg(bc=b"CB", abort_on=True), {"bc_abort"}, dict(nev=0, abort_read=1))
    add("barcode_not_asked_one_op", rec(cigar="40M", aux=ODD + CB), cfg(bc=b"CB", abort_on=True), {"one_op"}, dict(nev=0, abort_read=0))
    # an N, no event inside -m / -M, -s XS with abort_out on: the tag is still asked for
    add("n_without_event_abort_on", rec(cigar="20M10N20M", aux=ODD + XS), cfg(abort_on=True), {"asked_without_event", "tag_abort"}, dict(nev=0, abort_read=1))
    add("n_without_event_abort_off", rec(cigar="20M10N20M", aux=ODD + XS), cfg(), set(), dict(nev=0, abort_read=0, strand=ord("?")))
    add("n_without_event_odd_on", rec(cigar="20M10N20M", aux=ODD + XS), cfg(odd_on=True), {"asked_without_event", "tag_abort"}, dict(nev=0, odd_read=1, strand=ord("?") | 0x80))
    add("n_without_event_rf", rec(cigar="20M10N20M", aux=ODD + XS), cfg(strandness=1, abort_on=True), set(), dict(nev=0, abort_read=0))
    # strandness 1, 2, 3: the flag rule, the odd field is never met
    for s, strand in ((1, "+"), (2, "-"), (3, "-")):
        add("strandness_%d" % s, rec(flag=0x50 | 0x1, aux=ODD + XS), cfg(strandness=s, abort_on=True, odd_on=True), {"flag_rule"},
            dict(nev=1, abort_read=0, odd_read=0, strand=ord(strand)))
    add("strandness_1_disagree", rec(flag=0x40 | 0x1, aux=XS), cfg(strandness=1), {"flag_rule"}, dict(nev=1, strand=ord("?")))
    return out


@pytest.mark.parametrize("r,i,c,reach,expect", directed_cases())
def test_directed_case_reaches_its_branch_and_equals_the_restatement(emu, r, i, c, reach, expect):
    reached = set()
    want = restate(r, i, c, reached)
    assert reach <= reached, (reach, reached)
    for k, v in expect.items():
        assert want[k] == v, (k, want)
    assert emu_row(emu, r, i, c) == want


# ---- generated cases -------------------------------------------------------------------------------------------------------------------------
aux_field = st.one_of(
    st.sampled_from([XS, bamio.tagA("XS", "+"), b"XSA\0", b"XSi\1\0\0\0", bamio.tagZ("XS", "+"), CB, b"CBA!", bamio.tagZ("CB", ""), ODD, B_ARRAY,
                     b"YAB?" + struct.pack("<I", 9), b"NHC\1", b"ASs\1\0", b"XDd" + b"\0" * 8, bamio.tagZ("MD", "20"), b"HHH1F\0"]))
cigar_op = st.tuples(st.one_of(st.integers(0, 400), st.sampled_from([69, 70, 71, 499999, 500000, 500001])), st.sampled_from([0, 0, 3, 3, 1, 2, 4, 5, 7, 8]))


@settings(max_examples=3000, deadline=None)
@given(tid=st.integers(-1, 3), pos=st.integers(0, 3000), ops=st.lists(cigar_op, min_size=0, max_size=24), flag=st.integers(0, 0xfff),
       aux=st.lists(aux_field, max_size=4), i=st.integers(0, 12), strandness=st.integers(0, 3), bc=st.sampled_from([None, b"CB"]),
       region=st.one_of(st.none(), st.tuples(st.integers(0, 2), st.integers(0, 3500), st.integers(0, 3500))),
       stop=st.one_of(st.none(), st.integers(0, 12)), abort_on=st.booleans(), odd_on=st.booleans(), long_threshold=st.integers(0, 24),
       limits=st.sampled_from([(70, 500000), (0, 0xffffffff), (200, 300), (300, 200)]))
def test_generated_records_equal_the_restatement(emu, tid, pos, ops, flag, aux, i, strandness, bc, region, stop, abort_on, odd_on, long_threshold, limits):
    r = bamio.record(tid, pos, ops, flag=flag, aux=b"".join(aux), l_seq=7)
    c = cfg(strandness=strandness, bc=bc, abort_on=abort_on, odd_on=odd_on, long_threshold=long_threshold, min_intron=limits[0], max_intron=limits[1])
    if region is not None:
        c.update(region_tid=region[0], region_beg=region[1], region_end=region[2])
        if stop is not None:
            c.update(stop_on=True, stop_index=stop)
    assert emu_row(emu, r, i, c) == restate(r, i, c)


# ---- one whole file ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts,events,rows", [(["-s", "XS", "-a", "0"], 15085, 25), (["-s", "XS", "-a", "0", "-m", "200", "-M", "3000"], 15, 2)])
def test_events_of_a_whole_file_equal_the_oracles_scores(emu, opts, events, rows):
    """Sum of nev over every record of the file == sum of the BED12 score column (supporting reads of every junction) the oracle prints with -a 0."""
    contigs, recs = bamio.split_records(bamio.inflate_all(HCC))
    assert len(recs) == 31678
    c = cfg(n_ref=len(contigs))
    if "-m" in opts:
        c.update(min_intron=int(opts[opts.index("-m") + 1]), max_intron=int(opts[opts.index("-M") + 1]))
    got = sum(emu_row(emu, r, i, c)["nev"] for i, r in enumerate(recs))
    rc, bed, _ = run_oracle(opts + [HCC])
    assert rc == 0
    lines = bed.decode().splitlines()
    assert len(lines) == rows
    assert got == sum(int(l.split("\t")[4]) for l in lines) == events
