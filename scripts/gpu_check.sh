#!/bin/bash
# One GPU visit: smoke -> GPU tests -> short full bench (+ optional rocprof).
# Logs go to $ZF_OUT (default bench_out/ in the repository root).
# Stops at the first crash / abort / timeout (exit >= 124 or a signal); an
# ordinary test failure (pytest exit 1) still lets the bench run.
set -u
cd "$(dirname "$0")/.."
REPO=$(pwd); OUT=$(realpath -m "${ZF_OUT:-bench_out}"); export ZF_OUT="$OUT"
mkdir -p "$OUT"
export HSA_ENABLE_IPC_MODE_LEGACY=0
stage() {  # stage <name> <timeout> <cmd...>
  local name=$1 tmo=$2; shift 2
  echo "=== $name: $*" | tee -a "$OUT/stages.log"
  timeout -k 10 "$tmo" "$@" > "$OUT/$name.log" 2>&1
  local rc=$?
  echo "=== $name rc=$rc" | tee -a "$OUT/stages.log"
  tail -5 "$OUT/$name.log"
  if [ $rc -ge 124 ] || [ $rc -gt 128 ]; then echo "stopping after $name (rc=$rc)"; exit $rc; fi
  return $rc
}
MODE=${1:-all}
stage smoke 300 python -c "import __graft_entry__ as g; g.smoke()" || [ $? -lt 124 ] || exit 1
if [ "$MODE" = "all" ] || [ "$MODE" = "tests" ]; then
  stage pytest_gpu 1200 python -m pytest tests -m gpu -q -p no:cacheprovider --timeout 300 -ra
fi
if [ "$MODE" = "all" ] || [ "$MODE" = "bench" ]; then
  stage bench 600 python bench.py --steps 20 --warmup 3 --full
fi
if [ "${PROFILE:-0}" = "1" ]; then
  cd /tmp && export TMPDIR=/tmp
  cd "$REPO"
  stage rocprof 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run --output-format csv -- python bench.py --steps 10 --warmup 2 --full --no-cpu-baseline
fi
exit 0
