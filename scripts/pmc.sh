#!/bin/bash
# PMC passes for the flow kernel (each pass its own rocprofv3 run, --kernel-trace only).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
REPO=$(pwd); mkdir -p gpurun_out; export TMPDIR=/tmp
B="python3 bench.py --steps 3 --warmup 1 --full --no-cpu-baseline --no-spline-kernel ${BENCH_ARGS:-}"
i=0
for set in "SQ_INSTS_VALU SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE" \
           "SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_VMEM_RD SQ_VALU_MFMA_COEXEC_CYCLES SQ_INSTS_VALU_TRANS_F32 SQ_INSTS_SALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_ANY" ; do
  i=$((i+1))
  timeout -k 10 300 rocprofv3 --pmc $set --kernel-trace -d "$REPO/gpurun_out/pmc$i" -o run --output-format csv -- $B > gpurun_out/pmc$i.log 2>&1 || exit $?
done
exit 0
