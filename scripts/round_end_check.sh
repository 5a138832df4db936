#!/bin/bash
# Round-end check in one GPU visit: smoke, the GPU suite and the full
# bench (gpu_check.sh), the training-step sweep, and a rocprofv3 kernel
# trace of the K1 spline kernels (bench_rqs at the cfg2 coupling shape).
# Output goes to $ZF_OUT (default bench_out/ in the repository root).
set -u
cd "$(dirname "$0")/.."
REPO=$(pwd); OUT=$(realpath -m "${ZF_OUT:-bench_out}"); export ZF_OUT="$OUT"; mkdir -p "$OUT"
export HSA_ENABLE_IPC_MODE_LEGACY=0
bash scripts/gpu_check.sh all || exit $?
grep -q "rc=0" <(grep "pytest_gpu rc" "$OUT/stages.log") || { echo "GPU suite failed"; exit 1; }
timeout -k 10 300 python scripts/train_bench.py > "$OUT/train_bench.jsonl" 2> "$OUT/train_bench.err" || exit $?
cat "$OUT/train_bench.jsonl"
cd /tmp && export TMPDIR=/tmp && cd "$REPO"
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d "$OUT/k1prof" -o run --output-format csv -- python3 scripts/bench_rqs.py 20 16 > "$OUT/k1prof.log" 2>&1 || exit $?
tail -1 "$OUT/k1prof.log"
