"""The front of the overlapped upload (rgx_extract_mem on host bytes): the chunk copies and their arrival flags, the member list fetched into HBM by a
kernel, the helper thread that enqueues the copies.  As in tests/test_gpu_gate.py a child process lowers
the thresholds (REGTOOLS_AMD_OVERLAP, REGTOOLS_AMD_INFLATE=coop) so that files of a few hundred members take the arrival-gated launch; one child runs all
the calls, every table is compared byte for byte with the oracle's BED12 of the same file."""
import json
import os
import struct
import subprocess
import sys
import zlib

import pytest

import bamio
from conftest import ROOT, run_oracle

pytestmark = pytest.mark.gpu

CHUNKS = 8

CHILD = r"""
import json, sys
import regtools_amd
F = json.load(open(sys.argv[1]))
data = {k: (open(p, "rb").read(), open(p + ".bai", "rb").read()) for k, p in F.items()}
pins = {k: regtools_amd.PinnedBuffer(v[0]) for k, v in data.items()}

def pinned(ctx, k, **kw):
    je = regtools_amd.JunctionsExtractor(ctx=ctx, strandness=0, **kw)
    je.identify_junctions_from_BAM(bai_bytes=data[k][1], host_ptr=pins[k].ptr, host_len=len(data[k][0]))
    return je.bed12().decode("latin1")

def pageable(ctx, k):
    je = regtools_amd.JunctionsExtractor(ctx=ctx, strandness=0)
    je.identify_junctions_from_BAM(bam_bytes=data[k][0], bai_bytes=data[k][1])
    return je.bed12().decode("latin1")

out = {}
if sys.argv[3] == "pipeline":
    # a process of its own: the two contexts' eight streams are then all the process has, the layout the pipeline is built for (its gated waves and
    # the kernels that release them must not share a hardware queue, pipeline.cpp)
    order = ["small", "large", "boundary", "small"]
    ctx = regtools_amd.Context(0)
    out["sequential"] = [pinned(ctx, k) for k in order]
    ctx.close()
    pl = regtools_amd.Pipeline(0, 2)
    got = []
    for rnd in range(2):
        tickets = [pl.submit(bai_bytes=data[k][1], host_ptr=pins[k].ptr, host_len=len(data[k][0]), strandness=0) for k in order]
        got.append([pl.wait(t).bed12().decode("latin1") for t in tickets])
    pl.close()
    out["pipeline"] = got
    json.dump(out, open(sys.argv[2], "w"))
    sys.exit(0)
ctx = regtools_amd.Context(0)
out["boundary"] = [pinned(ctx, "boundary") for _ in range(2)]
ctx.close()
print("-- boundary done --", file=sys.stderr, flush=True)
# two sizes on one context: the larger file behind the smaller one grows the member list's block in HBM; the flag epochs go on
ctx = regtools_amd.Context(0)
out["two_sizes"] = [pinned(ctx, "small"), pinned(ctx, "large"), pinned(ctx, "small")]
ctx.close()
fresh = []
for k in ("small", "large"):
    ctx = regtools_amd.Context(0)
    fresh.append(pinned(ctx, k))
    ctx.close()
out["fresh"] = fresh
# a plain bytes object (hipMemcpyAsync blocks: the helper thread's reason to be) between two page-locked calls
ctx = regtools_amd.Context(0)
out["pageable"] = [pinned(ctx, "small"), pageable(ctx, "large"), pinned(ctx, "small"), pageable(ctx, "small")]
# three shards of one scan on one device: each sends the header's members and its own range
print("-- sharded --", file=sys.stderr, flush=True)
m = regtools_amd.extract_multi([0, 0, 0], bai_bytes=data["shard"][1], host_ptr=pins["shard"].ptr, host_len=len(data["shard"][0]), strandness=0)
out["sharded"] = [m.bed12().decode("latin1")]
print("-- one shard --", file=sys.stderr, flush=True)
out["sharded"].append(pinned(ctx, "shard"))
print("-- end --", file=sys.stderr, flush=True)
ctx.close()
json.dump(out, open(sys.argv[2], "w"))
"""


def _chunk_bytes(length, chunks=CHUNKS):
    """api_front.cpp stage_upload: the file goes up in `chunks` equal chunks of whole 4 KiB pages"""
    return ((length + chunks - 1) // chunks + 4095) & ~4095


def _stored_member(data, want):
    """the first bytes of `data` as a BGZF member of exactly `want` bytes (stored DEFLATE blocks: the compressed size follows the payload's); returns
    (member, bytes of data used)"""
    n = want - 31
    for _ in range(8):
        m = bamio.bgzf_member(data[:n], level=0)
        if len(m) == want:
            return m, n
        n -= len(m) - want
    raise AssertionError("no stored member of %d bytes" % want)


def _boundary_file(src, path):
    """`src` (a regtools_amd.synth file) with the same inflated stream and three member boundaries moved: one ON the end of an upload chunk, one a byte in
    front of a chunk's end, one a byte behind.  The member in front of such a boundary is cut in two -- a stored first half of the length that lands on the
    target, the rest deflated as before -- so the file's length moves by a few dozen bytes; the chunk size the finished file gets is checked at the end."""
    members = [(off, payload, isize) for off, payload, isize in bamio.bgzf_members(src)]
    raw = open(src, "rb").read()
    ends = [off for off, _, _ in members[1:]] + [len(raw)]
    for G in (_chunk_bytes(len(raw)), _chunk_bytes(len(raw)) + 4096):
        targets = [2 * G, 4 * G - 1, 6 * G + 1]
        out, cur = [], 0
        for (off, payload, isize), end in zip(members, ends):
            whole = raw[off:end]
            if targets and isize > 8192 and cur + 31 + 64 <= targets[0] and cur + len(whole) + 200 > targets[0]:
                data = zlib.decompress(payload, -15)
                first, used = _stored_member(data, targets[0] - cur)
                assert 0 < used < len(data)
                out += [first, bamio.bgzf_member(data[used:])]
                cur += len(first) + len(out[-1])
                targets.pop(0)
            else:
                out.append(whole); cur += len(whole)
        blob = b"".join(out)
        if not targets and _chunk_bytes(len(blob)) == G:
            open(path, "wb").write(blob)
            bounds = set(off for off, _, _ in bamio.bgzf_members(blob))
            assert 2 * G in bounds and 4 * G - 1 in bounds and 6 * G + 1 in bounds            # (what the test is about)
            assert bamio.inflate_all(blob) == bamio.inflate_all(raw)
            return G
    raise AssertionError("no chunk size fits the rebuilt file")


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    from regtools_amd import synth
    td = tmp_path_factory.mktemp("upload_front")
    files = {}
    # ("shard": rgx_extract_multi scans the members once for its shards from 8 MiB on, whatever REGTOOLS_AMD_OVERLAP says)
    for name, n, seed in (("small", 120_000, 21), ("large", 500_000, 22), ("plain", 200_000, 23), ("shard", 720_000, 24)):
        files[name] = str(td / (name + ".bam"))
        synth.write(files[name], n, shape="short", seed=seed)
    files["boundary"] = str(td / "boundary.bam")
    _boundary_file(files.pop("plain"), files["boundary"])
    synth.index(files["boundary"])
    assert os.path.getsize(files["shard"]) >= 8 << 20
    jf, of = str(td / "files.json"), str(td / "out.json")
    json.dump(files, open(jf, "w"))
    env = dict(os.environ, REGTOOLS_AMD_OVERLAP="0,%d" % CHUNKS, REGTOOLS_AMD_INFLATE="coop", REGTOOLS_AMD_EARLY_TAIL="0", REGTOOLS_AMD_TRACE="1", PYTHONPATH=ROOT)
    out, trace = {}, {}
    for mode in ("calls", "pipeline"):
        r = subprocess.run([sys.executable, "-c", CHILD, jf, of, mode], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        out.update(json.load(open(of)))
        trace[mode] = r.stderr.decode()
    want = {}
    for k, p in files.items():
        rc, bed, _ = run_oracle(["-s", "XS", p])
        assert rc == 0 and bed
        want[k] = bed.decode("latin1")
    return dict(out=out, want=want, trace=trace["calls"], trace_pipeline=trace["pipeline"], sizes={k: os.path.getsize(p) for k, p in files.items()})


def test_member_boundaries_at_a_chunk_end(child):
    """A wave is released by the flag of the chunk that holds the last byte it reads, 24 bytes behind its last member's payload: members that end on a
    chunk's end, a byte in front of it and a byte behind it read across it."""
    mine = child["trace"].split("-- boundary done --")[0]
    assert mine.count("launch inflate (gated)") == 2, mine[-2000:]                 # (the host scan vouched for the rebuilt file, both calls)
    assert "verdict not clean" not in child["trace"] and "upload failed" not in child["trace"]
    assert child["out"]["boundary"] == [child["want"]["boundary"]] * 2


def test_two_sizes_on_one_context(child):
    w = child["want"]
    assert child["out"]["fresh"] == [w["small"], w["large"]]
    assert child["out"]["two_sizes"] == [w["small"], w["large"], w["small"]]


def test_pageable_input_between_page_locked_calls(child):
    w = child["want"]
    assert child["out"]["pageable"] == [w["small"], w["large"], w["small"], w["small"]]


def test_sharded_input_sends_a_range(child):
    import re
    merged, one = child["out"]["sharded"]
    assert one == child["want"]["shard"] and merged == one
    sharded = child["trace"].split("-- sharded --")[1].split("-- one shard --")[0]
    assert sharded.count("launch inflate (gated)") == 3, sharded[-2000:]
    assert "whole-file upload" not in sharded, sharded[-2000:]
    size = child["sizes"]["shard"]
    went = {int(m.group(1)): tuple(int(x) for x in m.groups()[1:]) for m in
            re.finditer(r"shard (\d) of 3: bytes \[(\d+), (\d+)\) of (\d+) go up behind the header's \[0, (\d+)\)", sharded)}
    assert sorted(went) == [0, 1, 2], sharded[-2000:]
    assert went[0][0] == 0 and went[0][1] < size                                     # the first shard: the head of the file, header included
    for g in (1, 2):
        lo, hi, total, hdr = went[g]
        assert total == size and 0 < hdr <= lo < hi and (hi == size) == (g == 2), went
    assert went[0][1] > went[1][0] and went[1][1] > went[2][0]                       # (neighbours overlap by the members a record may run into)


def test_depth_two_pipeline_hands_the_wire_on(child):
    w = child["want"]
    seq = [w["small"], w["large"], w["boundary"], w["small"]]
    assert child["out"]["sequential"] == seq
    assert child["out"]["pipeline"] == [seq, seq]
    assert "launch inflate (gated)" in child["trace_pipeline"]
