#!/bin/bash
# GPU-box script: the new overlap test, the full gpu suite, then the bench line with a host-side trace of one step.
cd "$(dirname "$0")/.."
O=${1:?usage: tools/run_r2_check.sh OUTDIR}; mkdir -p $O
timeout 600 python -m pytest tests/test_gpu_parity.py -m gpu -x -q -k "overlapped" > $O/pytest_overlap.txt 2>&1; tail -5 $O/pytest_overlap.txt
timeout 900 python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $O/bench.json 2> $O/bench.err; cat $O/bench.json; tail -3 $O/bench.err
REGTOOLS_AMD_TRACE=1 timeout 600 python bench.py --full --steps 1 --warmup 1 --no-cpu-baseline 2>&1 | grep "rgx trace" | tail -60 > $O/trace.txt; head -40 $O/trace.txt
