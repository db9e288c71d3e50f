#!/usr/bin/env python
"""upload_timeline.py DIR -- what the chunked upload of `junctions extract` costs beside the wire's own time, from a rocprofv3 trace.

DIR holds the CSV output of
    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -o tl -- python bench.py --gpus 1 --steps K --warmup W
(no counters in the same run).  A chunk is a host-to-device copy of 0.3 ms and more; the chunks of one step follow one another within 2 ms.
Per step, for the last `--steps` steps of the trace (the timed ones):
    span      first chunk's start to last chunk's end
    wire      number of chunks x the trace's median chunk duration
    extra     span - wire: what is not transfer (gaps between the copies, copies that share the bus with something else)
    worst     the longest chunk over the median (the bar: 1.10)
    before    from the end of whatever the device did last before the step (the previous step's table copy) to the first chunk's start
and one line of medians over those steps.  --step N also prints step N's copies and kernels of 0.2 ms and more (N counts from the end: 1 = last).
"""
import argparse
import csv
import glob
import os
import statistics


def load(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0][:48], False))
    for f in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            h2d = "HOST_TO_DEVICE" in r.get("Direction", "")
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "COPY " + r.get("Direction", "?")[12:], h2d))
    rows.sort()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--step", type=int, default=0)
    a = ap.parse_args()
    rows = load(a.dir)
    chunks = [r for r in rows if r[3] and r[1] - r[0] >= 300e3]
    if not chunks:
        raise SystemExit("no chunk copies in the trace")
    steps = [[chunks[0]]]
    for c in chunks[1:]:
        if c[0] - steps[-1][-1][1] > 2e6:
            steps.append([c])
        else:
            steps[-1].append(c)
    n_chunks = statistics.mode(len(s) for s in steps)
    steps = [s for s in steps if len(s) == n_chunks][-a.steps:]
    med = statistics.median(c[1] - c[0] for s in steps for c in s)
    print("chunks per step %d, median chunk %.3f ms, steps looked at %d" % (n_chunks, med / 1e6, len(steps)))
    print("%5s %8s %8s %8s %7s %8s %7s" % ("step", "span", "wire", "extra", "worst", "before", "gaps"))
    out = []
    for k, s in enumerate(steps):
        span = s[-1][1] - s[0][0]
        worst = max(c[1] - c[0] for c in s) / med
        gaps = sum(s[i + 1][0] - s[i][1] for i in range(len(s) - 1))
        prev = [r[1] for r in rows if r[1] <= s[0][0]]
        before = s[0][0] - max(prev) if prev else float("nan")
        out.append((span, n_chunks * med, span - n_chunks * med, worst, before, gaps))
        print("%5d %8.3f %8.3f %8.3f %7.2f %8.3f %7.3f" % (k, span / 1e6, n_chunks * med / 1e6, (span - n_chunks * med) / 1e6, worst, before / 1e6, gaps / 1e6))
    m = [statistics.median(o[i] for o in out) for i in range(6)]
    print("%5s %8.3f %8.3f %8.3f %7.2f %8.3f %7.3f" % ("med", m[0] / 1e6, m[1] / 1e6, m[2] / 1e6, m[3], m[4] / 1e6, m[5] / 1e6))
    print("worst chunk of all steps: %.2f x the median" % max(o[3] for o in out))
    if a.step:
        s = steps[-a.step]
        t0 = s[0][0]
        nxt = steps[-a.step + 1][0][0] if a.step > 1 else t0 + 40e6
        for r in rows:
            if t0 - 1e6 <= r[0] < nxt and (r[1] - r[0] > 200e3 or "inflate" in r[2] or "member" in r[2] or r[2].startswith("COPY")):
                print("%9.3f -> %9.3f ms  (%7.3f)  %s" % ((r[0] - t0) / 1e6, (r[1] - t0) / 1e6, (r[1] - r[0]) / 1e6, r[2]))


if __name__ == "__main__":
    main()
