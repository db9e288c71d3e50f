"""No GPU: the cases of tests/cse_edge_cases.py are what they claim to be, and the references the GPU tests compare the kernels with
(tests/cse_ref.py) stand on three legs before a device is asked:
  * the product's own cores (cse_core.h junction_scan / variant_scan over GtfModel's tables, tests/hostemu emu_junction_scan / emu_variant_scan) give
    the same raw lists, item for item, on every annotation case in both index forms (the direct (contig, bin) index and the binary search);
  * the oracle's `junctions annotate` / `variants annotate` on the same files print the columns the references imply (anchor, the three skipped
    counts, the transcript list; transcripts, distances, annotations);
  * the reference binary printed the same columns for the same files (tests/golden/cse_edges/ref.json, made by make_golden_cse_edges.py), and the
    files are still the ones it read (a digest of every case's inputs).
The claims a builder makes -- candidate totals per junction, the index of the first flag-setting candidate, the level a transcript is filed at, the
candidate count of a window -- are re-derived here with arithmetic that shares nothing with the builder or the reference.

J_geometry (junctions at coordinates above 2^29, with distinct bins at the levels 1 to 6) has NO file-level check: `junctions annotate` reads the
splice site from a FASTA, and a FASTA of 600 Mb contigs is no fixture.  Its legs are the hostemu twin and the fact that its bin walk is the walk of
the variant case, whose seven-level transcripts the oracle and the reference binary do see (V_edges needs no FASTA)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import cse_edge_cases as ec
import cse_edge_common as cm
import cse_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "cse_edges", "ref.json")))
ORACLE = os.path.join(ROOT, "oracle", "oracle_cli")
JUNCTION_NAMES = sorted(ec.JUNCTION_CASES)


@pytest.fixture(scope="module")
def edge_dir(built, tmp_path_factory):
    return tmp_path_factory.mktemp("cse_edges")


_emu = None


def emu():
    global _emu
    if _emu is None:
        E = C.CDLL(os.path.join(ROOT, "tests", "hostemu", "libhostemu.so"))
        V = C.c_void_p
        E.emu_gtf_open.restype = V
        E.emu_gtf_open.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
        E.emu_gtf_close.argtypes = [V]
        E.emu_gtf_bin_index.argtypes = [V]
        E.emu_gtf_n_tx.argtypes = [V]
        E.emu_gtf_n_tx.restype = C.c_uint32
        E.emu_gtf_tx_id.argtypes = [V, C.c_uint32]
        E.emu_gtf_tx_id.restype = C.c_char_p
        E.emu_gtf_tx_bin.argtypes = [V, C.c_uint32]
        E.emu_gtf_tx_bin.restype = C.c_uint32
        E.emu_gtf_chrom_of.argtypes = [V, C.c_char_p]
        E.emu_gtf_chrom_of.restype = C.c_int32
        E.emu_junction_scan.restype = C.c_long
        E.emu_junction_scan.argtypes = [V, C.c_uint32, V, V, V, C.c_char_p, C.c_int, V, V, V, C.c_size_t, V, V, V]
        E.emu_variant_scan.restype = C.c_long
        E.emu_variant_scan.argtypes = [V, C.c_uint32, V, V, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, V, V, V, V, C.c_size_t, V, V, V]
        _emu = E
    return _emu


_models = {}


def model(case):
    if case.gtf not in _models:
        err = C.create_string_buffer(512)
        h = emu().emu_gtf_open(case.gtf.encode(), err, 512)
        assert h, err.value
        _models[case.gtf] = h
    return _models[case.gtf]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def emu_junctions(case, keep_single):
    n, cap = len(case.j_contig), 1 << 17
    u = lambda k: np.zeros(k, dtype=np.uint32)
    fl, vi, off = u(n), u(n), u(n + 1)
    while True:
        kind, a, b = u(cap), u(cap), u(cap)
        total = emu().emu_junction_scan(model(case), n, _p(case.j_contig), _p(case.j_start), _p(case.j_end1), case.j_strand.encode(), int(keep_single),
                                        _p(fl), _p(vi), _p(off), cap, _p(kind), _p(a), _p(b))
        assert total >= 0
        if total <= cap:
            return dict(flags=fl, visits=vi, off=off, kind=kind[:total], a=a[:total], b=b[:total])
        cap = total


def emu_variants(case, contig, o):
    n, cap = len(contig), 1 << 16
    u = lambda k: np.zeros(k, dtype=np.uint32)
    ces, cee, vi, off, tx, ann, dist = u(n), u(n), u(n), u(n + 1), u(cap), u(cap), u(cap)
    total = emu().emu_variant_scan(model(case), n, _p(contig), _p(case.v_pos0), o["intronic_min"], o["exonic_min"], o["all_intronic"], o["all_exonic"],
                                   o["skip_single"], _p(ces), _p(cee), _p(vi), _p(off), cap, _p(tx), _p(ann), _p(dist))
    assert 0 <= total <= cap
    return dict(ces=ces, cee=cee, visits=vi, off=off, tx=tx[:total], ann=ann[:total], dist=dist[:total])


def same(got, exp, what):
    for k in exp:
        assert np.array_equal(got[k], exp[k]), (what, k, first_difference(got[k], exp[k]))


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.asarray(a[:n]) != np.asarray(b[:n]))[0]
    return "lengths %d / %d, first difference at %s" % (len(a), len(b), ("%d: %d / %d" % (d[0], a[d[0]], b[d[0]])) if len(d) else "none")


# ---- the claims, with arithmetic of this file's own -----------------------------------------------------------------------------------------------
LEVEL_FIRST = [37359, 4681, 585, 73, 9, 1, 0]                # first bin id of the levels 0 (16 KiB) to 6 (the whole 32-bit range)


def filed_at(t):
    """(level, index at that level) of a transcript: of the exon that is first in strand order its start, of the last one its end, shifted until equal"""
    ex = sorted(t["exons"], reverse=t["strand"] == "-")
    lo, hi = ex[0][0] // 16384, (ex[-1][1] - 1) // 16384
    lvl = 0
    while lo != hi:
        lo, hi, lvl = lo // 8, hi // 8, lvl + 1
    return lvl, lo


def candidates(case, j):
    """the transcripts junction j is dealt, in visiting order"""
    c, js, je = int(case.j_contig[j]), int(case.j_start[j]), int(case.j_end1[j])
    out = []
    for t in case.transcripts:
        lvl, at = filed_at(t)
        if case.contigs.index(t["contig"]) == c and (js // 16384) // 8 ** lvl <= at <= ((je - 1) // 16384) // 8 ** lvl:
            out.append((lvl, at, t["id"].encode(), t))
    return [x[3] for x in sorted(out, key=lambda x: x[:3])]


@pytest.mark.parametrize("layout", ec.LAYOUTS)
@pytest.mark.parametrize("name", JUNCTION_NAMES + ["V_edges"])
def test_annotation_builders_build_what_they_claim(edge_dir, name, layout):
    case = ec.build(name, edge_dir, layout)
    assert len(case.contigs) == (3 if layout == "direct" else 230) and case.gtf_lines < 4000
    assert emu().emu_gtf_bin_index(model(case)) == (1 if layout == "direct" else 0)
    # ids in byte order are the transcript numbers; the product's model files every transcript where this file's arithmetic does
    ids = sorted(t["id"].encode() for t in case.transcripts)
    assert emu().emu_gtf_n_tx(model(case)) == len(ids)
    by_id = {t["id"]: t for t in case.transcripts}
    for k, i in enumerate(ids):
        assert emu().emu_gtf_tx_id(model(case), k) == i
        lvl, at = filed_at(by_id[i.decode()])
        assert emu().emu_gtf_tx_bin(model(case), k) == LEVEL_FIRST[lvl] + at, i
    for i, c in enumerate(case.contigs):
        assert emu().emu_gtf_chrom_of(model(case), c.encode()) == i
    for tid, lvl in case.claims["levels"].items():
        assert filed_at(by_id[tid])[0] == lvl, tid
    for j, total in case.claims["totals"].items():
        assert len(candidates(case, j)) == total, (name, j)
    for j, at in case.claims["setter"].items():
        js, je, sd = int(case.j_start[j]), int(case.j_end1[j]), case.j_strand[j]
        sets = [t["strand"] == sd and len(t["exons"]) > 1 and any(e == js or s == je for s, e in t["exons"]) for t in candidates(case, j)]
        assert sets.index(True) == at and sum(sets) == 1, (name, j)
    if name == "J_totals":
        assert sorted(set(case.claims["totals"].values())) == [0, 1, 63, 64, 65, 127, 128, 129, 200]
        # some lanes of every turn are idle: candidates of the other strand among the junction's
        for j in case.claims["totals"]:
            n_other = sum(t["strand"] != case.j_strand[j] for t in candidates(case, j))
            assert n_other > 0 or case.claims["totals"][j] < 2
    if name.startswith("J_setter"):
        assert sorted(set(case.claims["setter"].values())) == ec.SETTER_AT and len(case.claims["setter"]) == 2 * len(ec.SETTER_AT)
    if name in ("J_geometry", "V_edges"):
        assert {filed_at(t)[0] for t in case.transcripts} == set(range(7))
    if name == "J_geometry":
        spans = sorted({(int(e) - 1) // 16384 - int(s) // 16384 + 1 for s, e in zip(case.j_start, case.j_end1)})
        assert 2 in spans and 9 in spans
        assert any(int(s) % 16384 == 0 for s in case.j_start)
        assert {(int(e) - 1) % 16384 for e in case.j_end1} >= {16383, 0, 1}
        assert len(set(case.j_contig.tolist())) == 3
    if name == "J_items":
        assert len(case.j_contig) == 129 and "?" in case.j_strand[:4] and -1 in case.j_contig[:4].tolist()


def test_window_builders_build_what_they_claim():
    def n_candidates(c, w):
        span = int((c.rend.astype(np.int64) - c.rpos.astype(np.int64)).max())
        t, beg, end = int(c.w_tid[w]), int(c.w_beg[w]), int(c.w_end[w])
        return int(((c.tid.astype(np.int64) == t) & (c.rpos.astype(np.int64) >= max(beg - span, 0)) & (c.rpos.astype(np.int64) < end)).sum())
    for name in ec.WINDOW_CASES:
        c = ec.build(name, None)
        key = c.tid.astype(np.int64) << 32 | c.rpos.astype(np.int64)
        assert np.all(key[1:] >= key[:-1]), name                    # file order
        for w, n in c.claims.get("candidates", {}).items():
            assert n_candidates(c, w) == n, (name, w)
    c = ec.build("W_sizes", None)
    assert sorted(c.claims["candidates"].values()) == ec.WINDOW_CANDIDATES and {4095, 4096, 4097, 8197} <= set(ec.WINDOW_CANDIDATES)
    ev, win, counts = cse_ref.window_pairs(c.tid, c.rpos, c.rend, c.w_tid, c.w_beg, c.w_end)
    big = [w for w, n in c.claims["candidates"].items() if n > 4000]
    for w in big:                                                   # about half of a large window's candidates end in front of it
        assert 0.4 < counts[w] / c.claims["candidates"][w] < 0.6
    assert counts[0] == 0 and max(counts) > 1000                    # an empty window first; a window larger than the batch of 1000
    assert [cse_ref.pair_batches(counts, b or 1 << 26, len(c.tid)) for b in ec.PAIR_BATCHES][0] == 1
    assert 1 < cse_ref.pair_batches(counts, 5000, len(c.tid)) < cse_ref.pair_batches(counts, 1000, len(c.tid)) < len(counts)
    # a batch of 1: every window that holds a pair is alone but for empty windows behind it
    assert cse_ref.pair_batches(counts, 1000, len(c.tid)) < cse_ref.pair_batches(counts, 1, len(c.tid)) >= sum(n > 0 for n in counts)
    c = ec.build("W_300", None)
    assert len(c.w_tid) == 300 and c.claims["big"] == [0, 255, 256, 299]
    assert [w for w in range(300) if n_candidates(c, w) > 4096] == c.claims["big"] and max(c.claims["big"]) >= 256
    c = ec.build("W_span", None)
    assert len(c.tid) > 262_144 and c.claims["longest"] > 262_144
    assert int(np.argmax(c.rend.astype(np.int64) - c.rpos)) == c.claims["longest"]
    ev, win, counts = cse_ref.window_pairs(c.tid, c.rpos, c.rend, c.w_tid, c.w_beg, c.w_end)
    for w in c.claims["only_longest"]:
        assert ev[win == w].tolist() == [c.claims["longest"]]
    assert n_candidates(c, 0) > 4096


def test_assoc_builder_builds_what_it_claims():
    for n in (1, 1000):
        c = ec.build("A_%d" % n, None)
        assert len(c.w_contig) == n and np.diff(c.contig_off.astype(np.int64)).tolist() == ec.BUCKETS
        pj, pw = cse_ref.assoc_pairs(c.w_contig, c.w_ces, c.w_cee, c.contig_off, c.j_start, c.j_end)
        assert len(pj) > 0
    assert -1 in c.w_contig.tolist() and np.any(c.w_ces > c.w_cee)
    kept = {w: set(pj[pw == w].tolist()) for w in range(19)}
    j = int(c.contig_off[5]) + 64
    assert all(j in kept[w] for w in (0, 3, 6, 7, 8, 9)) and not any(j in kept[w] for w in (1, 2, 4, 5, 10))
    assert int(c.contig_off[2]) not in kept[15] and all(int(c.contig_off[2]) in kept[w] for w in (16, 17)) and int(c.contig_off[2]) not in kept[18]
    assert kept[11] == set() and kept[12] == set() and len(kept[13]) == 1 and len(kept[14]) == 129


# ---- the references against the product's cores on the host ------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_single", [False, True])
@pytest.mark.parametrize("layout", ec.LAYOUTS)
@pytest.mark.parametrize("name", JUNCTION_NAMES)
def test_junction_reference_equals_the_core(edge_dir, name, layout, keep_single):
    case = ec.build(name, edge_dir, layout)
    ann = cse_ref.Annotation(case.transcripts, case.contigs)
    exp = cse_ref.junction_scan(ann, case.j_contig, case.j_start, case.j_end1, case.j_strand, keep_single)
    same(emu_junctions(case, keep_single), exp, (name, layout, keep_single))
    assert len(exp["kind"]) > 0
    if name == "J_items":
        # items straddle the turns: some junction has a transcript whose items begin in one stretch of 64 candidates' items and end in the next --
        # and keep_single changes what is listed (the single exon at candidate 10 sets a flag)
        assert int(np.diff(exp["off"].astype(np.int64)).max()) > 132
        other = cse_ref.junction_scan(ann, case.j_contig, case.j_start, case.j_end1, case.j_strand, not keep_single)
        assert not np.array_equal(other["flags"], exp["flags"])


@pytest.mark.parametrize("layout", ec.LAYOUTS)
@pytest.mark.parametrize("k", range(len(ec.VARIANT_OPTS)))
def test_variant_reference_equals_the_core(edge_dir, layout, k):
    case = ec.build("V_edges", edge_dir, layout)
    o = ec.VARIANT_OPTS[k]
    ann = cse_ref.Annotation(case.transcripts, case.contigs)
    contig = np.array([ann.contig_index.get(c, -1) for c in case.v_contig], dtype=np.int32)
    exp = cse_ref.variant_scan(ann, contig, case.v_pos0, **o)
    same(emu_variants(case, contig, o), exp, (layout, o))
    per = np.diff(exp["off"].astype(np.int64))
    assert per.min() == 0 and (per == 1).any() and len(case.v_pos0) >= 129
    if o["intronic_min"] == 2 and o["exonic_min"] == 3 and not o["all_intronic"] and not o["all_exonic"]:
        assert per.max() == 70                                       # more than a wave's worth of hits
    if o["all_exonic"]:
        # the position below intronic_min: W_low holds it and is not walked once the subtraction wraps, W_six (level 6) is
        low = [i for i, (c, p) in enumerate(zip(case.v_contig, case.v_pos0)) if int(p) == 0]
        hit = [[ann.ids[t] for t in exp["tx"][exp["off"][i]:exp["off"][i + 1]]] for i in low]
        assert hit == ([["W_low"], ["W_six"]] if o["intronic_min"] == 0 else [[], ["W_six"]])


# ---- the references against the oracle and the reference binary, through files -----------------------------------------------------------------------
def test_fixture_names():
    assert sorted(GOLD) == sorted("%s/%s" % (n, l) for n in cm.FILE_JUNCTION_CASES + ["V_edges"] for l in ec.LAYOUTS)


@pytest.mark.parametrize("layout", ec.LAYOUTS)
@pytest.mark.parametrize("name", cm.FILE_JUNCTION_CASES)
def test_junction_reference_equals_the_oracle_and_the_reference_binary(edge_dir, name, layout):
    case = ec.build(name, edge_dir, layout)
    gold = GOLD["%s/%s" % (name, layout)]
    assert case.digest == gold["inputs_sha256"], "the builder drifted: regenerate tests/golden/cse_edges/ref.json"
    ann = cse_ref.Annotation(case.transcripts, case.contigs)
    for args in cm.JUNCTION_RUNS:
        out = os.path.join(str(edge_dir), "%s_%s.ja" % (name, layout))
        r = subprocess.run([ORACLE, "junctions-annotate"] + args + ["-o", out, case.bed, case.fasta, case.gtf], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        g = gold["runs"][" ".join(args)]
        assert r.returncode == g["rc"] == 0, r.stderr
        rows = cm.junction_columns(open(out, "rb").read())
        assert len(rows) == g["rows"] and cm.digest(rows) == g["sha256"], (name, layout, args)
        ref = cse_ref.junction_scan(ann, case.j_contig, case.j_start, case.j_end1, case.j_strand, "-S" in args)
        exp = []
        for i in range(len(case.j_contig)):
            if case.j_contig[i] < 0:
                continue                                              # (no BED line)
            n_acc, n_exo, n_don, txs = cse_ref.unique_counts(ref, i)
            exp.append(("J%05d" % i, n_acc, n_exo, n_don, cm.anchor_of(int(ref["flags"][i])), ",".join(ann.ids[t] for t in txs) or "NA"))
        assert rows == exp, (name, layout, args, next((a, b) for a, b in zip(rows, exp) if a != b))


@pytest.mark.parametrize("layout", ec.LAYOUTS)
def test_variant_reference_equals_the_oracle_and_the_reference_binary(edge_dir, layout):
    case = ec.build("V_edges", edge_dir, layout)
    gold = GOLD["V_edges/%s" % layout]
    assert case.digest == gold["inputs_sha256"], "the builder drifted: regenerate tests/golden/cse_edges/ref.json"
    ann = cse_ref.Annotation(case.transcripts, case.contigs)
    contig = np.array([ann.contig_index.get(c, -1) for c in case.v_contig], dtype=np.int32)
    names = ["non_splice_region", "exonic", "intronic", "splicing_exonic", "splicing_intronic"]
    for o, args in zip(ec.VARIANT_OPTS, cm.VARIANT_RUNS):
        out = os.path.join(str(edge_dir), "V_%s.vcf" % layout)
        r = subprocess.run([ORACLE, "variants-annotate"] + args + ["-o", out, case.vcf, case.gtf], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        g = gold["runs"][" ".join(args)]
        assert r.returncode == g["rc"] == 0, r.stderr
        rows = cm.variant_columns(open(out, "rb").read())
        assert len(rows) == g["rows"] and cm.digest(rows) == g["sha256"], (layout, args)
        ref = cse_ref.variant_scan(ann, contig, case.v_pos0, **o)
        exp = []
        for i in range(len(contig)):
            k = slice(int(ref["off"][i]), int(ref["off"][i + 1]))
            lists = [",".join(ann.ids[t] for t in ref["tx"][k]), ",".join(str(d) for d in ref["dist"][k]), ",".join(names[a] for a in ref["ann"][k])]
            exp.append((case.v_contig[i], int(case.v_pos0[i]) + 1) + tuple(x or "NA" for x in lists))
        assert rows == exp, (layout, args, next((a, b) for a, b in zip(rows, exp) if a != b))
