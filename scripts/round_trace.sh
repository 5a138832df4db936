#!/bin/bash
# The committed-evidence run of a build (one GPU visit): smoke, the GPU
# suite, then the full bench under rocprofv3 --kernel-trace --stats (the
# bench line printed in the same run: scripts/trace_vs_bench.py).
# Output goes to $ZF_OUT (default bench_out/ in the repository root).
set -u
cd "$(dirname "$0")/.."
REPO=$(pwd); OUT=$(realpath -m "${ZF_OUT:-bench_out}"); export ZF_OUT="$OUT"; mkdir -p "$OUT"
export HSA_ENABLE_IPC_MODE_LEGACY=0
rm -rf "$OUT/bench_trace" "$OUT/stages.log"
bash scripts/gpu_check.sh tests || exit $?
grep -q "pytest_gpu rc=0" "$OUT/stages.log" || { echo "GPU suite failed"; exit 1; }
cd /tmp && export TMPDIR=/tmp && cd "$REPO"
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/bench_trace" -o run --output-format csv \
  -- python3 bench.py --steps 20 --warmup 5 --full > "$OUT/bench_trace.log" 2>&1 || exit $?
grep '^{' "$OUT/bench_trace.log" | head -1 | cut -c1-300
