"""The stretch between the DEFLATE launch and the group-by -- k_seg_walk / k_seg_verify, k_decode_seg<true>, k_decode_sparse, k_long_fill, k_emit_short,
k_emit_long -- on files aimed at its edges (tests/layout_cases.py), through the public path: JunctionsExtractor on a real BAM, BED12 bytes compared with
the oracle's, their SHA-256 and row count with what the reference binary printed (tests/golden/layout/layout_ref.json), and the row count with the number
of junctions the builder planted and the filters keep.  Every read has its own locus: a wrong event is a wrong row, and the assertion names the first one.
tests/test_layout_cases_host.py checks without a GPU that the files are what they claim to be.  Run with `-m gpu` on an MI355X.

That these tests can fail was shown once, on scratch builds with one-line faults, this file run once per build:
  * k_emit_long, `ts_carry = s_R[wave][lastb]` (not lastb + 1): test_emit_long_tile_edges[A_directed, A_generated, A_motif] fail (first wrong row: a left
    anchor that starts at the N of the tile before, not behind it).  The grid files have no read of more than one tile and pass.
  * k_emit_long, the pending junction's strand from `strand`, not `my_strand`: test_emit_long_tile_edges[A_motif] fails (the '-' pending at
    operation 63 comes out '?'); nothing else can see it.
  * k_emit_long, `nx_i = nn_i` skipped on a wave's second trip: NOT a fault that only changes values.  Its one run was killed at the time limit in
    test_emit_long_grid_stride_and_prefetch[A_grid_16385], the first file with a third trip, after A_grid_8192 and A_grid_8193 had passed: the third
    trip emits the second trip's read again, its own read's event slots are never written, and the group-by is handed whatever lay there.
    Run instead with only `nx_pos` left one stride stale (every read emitted once, into its own slots): A_grid_16385 and A_grid_24580 fail,
    A_grid_8192 and A_grid_8193 pass (a second trip's row was fetched during the first).
  * k_decode_seg, `in_win = STAGED && rec_end <= w1 + 16`: test_record_layout_against_segments_and_window[B_win_end_seq] fails (the tag walk meets bytes
    that were never staged and the call ends like the reference at an aux field of unknown type); the other B files pass.  A first version of that
    file, under a header with H % 16 = 12, passed: the window is staged in 16-byte pieces from a 16-aligned start, which had brought the four bytes
    behind w1 into the LDS.  The window-end files now have H % 16 = 0.  This fault was not run on B_win_end_cig and the A files: a CIGAR word read from
    unstaged LDS makes the decode's event count and the emitter's disagree, which leaves event slots unwritten like the fault above.
  * k_seg_walk, the `room` mask `(1u << (room - 1)) - 1u`: no output differs anywhere (the verify sweep repairs the segment);
    test_record_layout_against_segments_and_window[B_room_edge] fails on framing_sweeps, 2 for 1.  The start-phase files cannot see it: with 16 KiB
    segments `room < 16` is reached only behind a candidate whose chain ended, which is what B_room_edge plants.  framing_sweeps depends on the
    file's bytes alone (1 in every run of the unchanged code).
"""
import hashlib
import json
import os

import pytest

import layout_cases as lc
from conftest import run_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "layout", "layout_ref.json")))


@pytest.fixture(scope="module")
def layout_dir(built, tmp_path_factory):
    return tmp_path_factory.mktemp("layout")


def gpu_extract(ctx, argv):
    """(rc, bed12 bytes, extractor) the way `regtools junctions extract <argv>` would produce them"""
    import regtools_amd
    je = regtools_amd.JunctionsExtractor(ctx=ctx)
    try:
        je.parse_options(list(argv))
        je.identify_junctions_from_BAM()
    except regtools_amd.RegtoolsError as e:
        return (0 if e.code == 0 else 1), b"", je
    return 0, je.bed12(), je


def first_difference(got, exp):
    g, e = got.splitlines(), exp.splitlines()
    for k in range(max(len(g), len(e))):
        a, b = g[k] if k < len(g) else b"<no row>", e[k] if k < len(e) else b"<no row>"
        if a != b:
            return "row %d of %d / %d\n  device: %s\n  oracle: %s" % (k, len(g), len(e), a.decode(), b.decode())
    return "equal"


def check(gpu_ctx, case):
    for args in case.arglists:
        key = " ".join(args)
        rc, out, je = gpu_extract(gpu_ctx, case.argv(args))
        orc, exp, err = run_oracle(case.argv(args))
        gold = GOLD[case.name]["runs"][key]
        print("%s [%s]: device rows %d, oracle rows %d, reference rows %d, planted %d, records %s, framing sweeps %s" % (
            case.name, key, out.count(b"\n"), exp.count(b"\n"), gold["rows"], case.planted[key], je.stats.get("n_records") if rc == 0 else None,
            je.stats.get("framing_sweeps") if rc == 0 else None))
        assert rc == orc == gold["rc"] == 0, err
        assert out == exp, "%s [%s]: %s" % (case.name, key, first_difference(out, exp))
        assert hashlib.sha256(out).hexdigest() == gold["sha256"] and out.count(b"\n") == gold["rows"], (case.name, key)
        assert out.count(b"\n") >= case.planted[key] > 0
        assert je.stats["n_records"] == case.n_records
        assert je.stats["n_events"] >= case.planted[key]
        if case.name == "B_room_edge":
            # every guess of the framing is right in this file, the true starts in a segment's last bytes included: a second sweep means one was not found
            assert je.stats["framing_sweeps"] == 1
    return je


A_SMALL = ["A_directed", "A_generated", "A_motif"]
A_GRID = ["A_grid_%d" % n for n in lc.GRID_SIZES]
B_NAMES = [n for n in lc.NAMES if n.startswith("B_")]
assert sorted(A_SMALL + A_GRID + B_NAMES) == lc.NAMES


@pytest.mark.parametrize("name", A_SMALL)
def test_emit_long_tile_edges(gpu_ctx, layout_dir, name):
    """Reads of 17 to 200 operations: an N on either side of a tile edge, right anchors that run through a tile or to the read's end, every closer of a
    pending N, left anchors carried from the tile before, pending junctions that -m / -M drop, zero-length operations, the motif chain over an edge;
    400 generated reads of every operation code."""
    check(gpu_ctx, lc.build(name, layout_dir))


@pytest.mark.parametrize("name", A_GRID)
def test_emit_long_grid_stride_and_prefetch(gpu_ctx, layout_dir, name):
    """8,192 long reads fill k_emit_long's grid once; from 8,193 on a wave makes a second trip (24,580: a fourth) with the row it fetched ahead."""
    check(gpu_ctx, lc.build(name, layout_dir))


@pytest.mark.parametrize("name", B_NAMES)
def test_record_layout_against_segments_and_window(gpu_ctx, layout_dir, name):
    """Record starts 0 to 40 bytes in front of a segment's end (under every alignment of the segment's start, and between records of kilobytes, where the
    lane-per-segment decode runs), record ends around the end of the staged window, segments full of 37-byte records, streams that end on a segment's end."""
    case = lc.build(name, layout_dir)
    je = check(gpu_ctx, case)
    assert je.stats["inflated_bytes"] >= case.header_len + 37 * case.n_records
