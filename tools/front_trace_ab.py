#!/usr/bin/env python3
"""The decisions of an extract call's front, one build of the library against another: python tools/front_trace_ab.py OTHER_TREE [OUT_DIR]
(run from this tree's root on a machine with an MI355X; OTHER_TREE is a built checkout of the commit to compare with).

For each of three environments a fresh process per build runs, on one context, two calls on page-locked host bytes on each of four synthetic files
(short 1.2 M and 3.2 M reads, fuzz 20 k, long 2 k: the files of tests/test_gpu_gate.py) and rgx_extract_multi over three shards of the first, with
REGTOOLS_AMD_TRACE=1 REGTOOLS_AMD_INFLATE=coop.  The [rgx trace] lines are compared with their timing columns stripped: every "early tail: part j:
members < k, segments [a, b) of n", every "shard g of n: bytes [..)", which launches were gated.  A change that only moves code leaves the diff empty.
Writes OUT_DIR/{build}_{environment}.stderr.txt, diff_{environment}.txt and summary.txt; exit status 0 = no difference."""
import difflib
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.getcwd()
ENVS = (("overlap_0_16_1", {"REGTOOLS_AMD_OVERLAP": "0,16,1"}), ("overlap_0_7", {"REGTOOLS_AMD_OVERLAP": "0,7"}),
        ("early_tail_7cuts", {"REGTOOLS_AMD_OVERLAP": "0,16,1", "REGTOOLS_AMD_EARLY_TAIL": "2,4,6,8,10,12,14"}))
FILES = (("short_1200000", "short", 1200000, 3), ("short_3200000", "short", 3200000, 3), ("fuzz_20000", "fuzz", 20000, 4), ("long_2000", "long", 2000, 5))
CHILD = r"""
import json, sys
import regtools_amd
from regtools_amd import _ffi
jobs = json.load(open(sys.argv[1]))
print("-- library %s --" % _ffi.LIB_PATH, file=sys.stderr, flush=True)
ctx = regtools_amd.Context(0)
out = []
for j in jobs:
    bam = open(j["bam"], "rb").read(); bai = open(j["bam"] + ".bai", "rb").read()
    pin = regtools_amd.PinnedBuffer(bam)
    print("-- file %s --" % j["name"], file=sys.stderr, flush=True)
    je = regtools_amd.JunctionsExtractor(ctx=ctx, strandness=0)
    res = []
    for rep in range(2):                       # twice: the gate's flags keep the earlier call's epoch
        print("-- call %d --" % rep, file=sys.stderr, flush=True)
        je.identify_junctions_from_BAM(bai_bytes=bai, host_ptr=pin.ptr, host_len=len(bam))
        res.append(je.bed12().decode("latin1"))
    if j.get("sharded"):
        print("-- sharded --", file=sys.stderr, flush=True)
        m = regtools_amd.extract_multi([0, 0, 0], bai_bytes=bai, host_ptr=pin.ptr, host_len=len(bam), strandness=0)
        res.append(m.bed12().decode("latin1"))
    out.append(res)
    pin.close()
ctx.close()
json.dump(out, open(sys.argv[2], "w"))
"""


def strip(text):
    keep = []
    for l in text.splitlines():
        if not (l.startswith("[rgx trace]") or l.startswith("-- ")) or l.startswith("-- library"):
            continue
        if "first chunk enqueued" in l:          # written by the upload thread: its place among the other lines is a race
            continue
        l = re.sub(r"\+\s*[0-9.]+ ms\s+\(at\s+[0-9.]+\)", "+T", l)
        l = re.sub(r" clock [0-9.]+", "", l)
        l = re.sub(r"\+\s*[0-9.]+ ms$", "+T", l)
        l = re.sub(r"total [0-9.]+ ms; device buffers grown so far: (\d+) allocations, ([0-9.]+) MB, [0-9.]+ ms", r"total T; grown \1 allocations, \2 MB", l)
        l = re.sub(r"member scan [0-9.]+ ms, shards [0-9.]+ ms \(.*", "member scan T", l)
        l = re.sub(r"merge (\S+)\s+[0-9.]+ ms", r"merge \1 T", l)
        keep.append(l)
    # the shards run on threads of their own: what each says is compared, not the order
    head, _, tail = "\n".join(keep).partition("-- sharded --")
    return head.splitlines() + ["-- sharded (lines sorted) --"] + sorted(tail.splitlines())


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    builds = (("other", os.path.abspath(sys.argv[1])), ("this", ROOT))
    out_dir = os.path.abspath(sys.argv[2] if len(sys.argv) > 2 else "front_trace_ab")
    os.makedirs(out_dir, exist_ok=True)
    log = open(os.path.join(out_dir, "summary.txt"), "w")

    def say(*a):
        s = " ".join(str(x) for x in a)
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    sys.path.insert(0, ROOT)
    from regtools_amd import synth
    worst = 0
    with tempfile.TemporaryDirectory(dir="/tmp") as td:
        jobs = []
        for name, shape, n, seed in FILES:
            p = os.path.join(td, name + ".bam")
            synth.write(p, n, shape=shape, seed=seed)
            jobs.append(dict(name=name, bam=p, sharded=(name == FILES[0][0])))
        jf = os.path.join(td, "jobs.json")
        json.dump(jobs, open(jf, "w"))
        for ename, extra in ENVS:
            got = {}
            for bname, broot in builds:
                env = dict(os.environ, REGTOOLS_AMD_TRACE="1", REGTOOLS_AMD_INFLATE="coop", PYTHONPATH=broot, **extra)
                of = os.path.join(td, "out_%s_%s.json" % (bname, ename))
                r = subprocess.run([sys.executable, "-c", CHILD, jf, of], env=env, cwd=td, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
                err = r.stderr.decode("latin1")
                open(os.path.join(out_dir, "%s_%s.stderr.txt" % (bname, ename)), "w").write(err)
                if r.returncode != 0:            # (nothing more is started on the device behind a process that failed)
                    say(ename, bname, "exit status", r.returncode)
                    say(err[-3000:])
                    return 1
                got[bname] = (strip(err), hashlib.sha256(open(of, "rb").read()).hexdigest())
            a, b = got["other"], got["this"]
            d = list(difflib.unified_diff(a[0], b[0], "other", "this", lineterm=""))
            open(os.path.join(out_dir, "diff_%s.txt" % ename), "w").write("\n".join(d) + "\n")
            say(ename, "stripped lines", len(a[0]), len(b[0]), "| diff lines", len(d), "| early-tail part lines", sum("early tail: part" in l for l in b[0]),
                "| shard lines", sum(" go up behind the header" in l for l in b[0]), "| gated launches", sum("launch inflate (gated)" in l for l in b[0]),
                "| outputs equal", a[1] == b[1])
            worst = max(worst, len(d) + (a[1] != b[1]))
    say("RESULT:", "no difference" if worst == 0 else "DIFFERENCES")
    return 0 if worst == 0 else 2


if __name__ == "__main__":
    sys.exit(main())
