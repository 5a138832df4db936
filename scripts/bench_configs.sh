#!/bin/bash
# Every BASELINE config on one GPU (one GPU visit): one full bench line each
# (with the CPU baseline and parity) into $ZF_OUT/configs.jsonl (default
# bench_out/ in the repository root).  Stops at the first failure.
set -u
cd "$(dirname "$0")/.."
OUT=$(realpath -m "${ZF_OUT:-bench_out}"); export ZF_OUT="$OUT"; mkdir -p "$OUT"
export HSA_ENABLE_IPC_MODE_LEGACY=0
: > "$OUT/configs.jsonl"
for c in ${CONFIGS:-cfg2 cfg3 cfg3s cfg4 cfg5}; do
  timeout -k 10 300 python bench.py --config $c --steps 20 --warmup 5 --full --no-spline-kernel > "$OUT/cfg_$c.log" 2>&1 || { tail -5 "$OUT/cfg_$c.log"; exit 1; }
  grep '^{' "$OUT/cfg_$c.log" >> "$OUT/configs.jsonl"
  python -c "import json,sys; d=json.loads(open('$OUT/cfg_$c.log').read().strip().splitlines()[-1]); print('$c', round(d['value']/1e6,1), 'M/s', round(d['roofline']['frac'],3), d.get('cpu_baseline',{}).get('value'))"
done
