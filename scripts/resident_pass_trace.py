"""Tuning: per-wave stamp trace of the resident flow kernel's passes
(flow_kernel_x3r under -DZF_X3_TRACE=1; never the shipped library).  Build

    python -m zenflow_amd.build --out tune/libx3rtrace.so -DZF_X3_TRACE=1

and run on the GPU as

    ZF_LIB=tune/libx3rtrace.so python scripts/resident_pass_trace.py [cfg2] [rows_log2] > profiles/resident_pass_trace.json

Per block, wave and pass the kernel stores 16 s_memtime stamps (zf_flow_x3_kernel.h,
X3R_STAMP): 0 arrival at the pass's first barrier, 1 exit from it, 2 span DMA issued,
3 exit from the second barrier, 4 the wave's first tile's state ready, 5.. the end of
each of its tiles.  The summary holds, per pass, medians and ranges over blocks of
  tail            spread (max - min over the block's waves) of the arrival at the first barrier;
  span_gap        exit of the first barrier -> exit of the second (median over the block's waves);
  first_tile      exit of the second barrier -> end of the wave's first tile (median over waves);
  middle_tile     end of tile m - 1 -> end of tile m, m the middle of a wave's tile list;
  last_round_tile the same for the last tile of the waves that run the block's last round.
  idle_before_barrier_mean  what a wave waits at the first barrier on average (last arrival - its own).
Ticks are s_memtime's shader-clock ticks, comparable only inside a block; they become time through the
wall time of the launches (the trace build's own), and every figure is also given as a share of the
kernel's length."""
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
os.environ.setdefault("ZF_ALLOW_MISSING_SYMBOLS", "1")
import bench  # noqa: E402
from zenflow_amd import _lib as L  # noqa: E402
from zenflow_amd._lib import DeviceArray  # noqa: E402

NW, PASSES, STAMPS = 12, 4, 16

name = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
N = 1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 20)
D, Cd, K, layers, nL, latent, mode, act = bench.workload(name)
flow, variables, x, c = bench.make_workload(name, N)
prog = flow.bind(variables, D, Cd).program
lib = L.load_library()
MAXB = 1024  # blocks the buffer has room for (one block per CU; the kernel checks its index against the length)
n = MAXB * NW * PASSES * STAMPS
buf = DeviceArray.from_numpy(np.zeros(n, np.uint64))
fn = getattr(lib, f"zf_x3r_trace_set_k{K}")
fn.argtypes = [C.c_void_p, C.c_longlong]
assert fn(buf.ptr, n) == 0
xd = DeviceArray.from_numpy(x)
out = DeviceArray((N,))
for _ in range(3):
    prog.log_prob(xd, None, out=out)
L.synchronize()
reps = 20
t0 = time.perf_counter()
for _ in range(reps):
    prog.log_prob(xd, None, out=out)
L.synchronize()
wall_us = (time.perf_counter() - t0) / reps * 1e6
assert prog.launch_count("resident_frame") > 0, "the launch did not take the resident form's specialised frame"
t = buf.numpy().reshape(MAXB, NW, PASSES, STAMPS).astype(np.int64)
ncu = int((t[:, 0, 0, 0] > 0).sum())  # blocks that ran: 0 .. ncu - 1
assert ncu > 0 and (t[:ncu, 0, 0, 0] > 0).all()
t = t[:ncu]
assert fn(None, 0) == 0

# s_memtime counts shader-clock ticks and is not comparable between blocks (one counter per XCD), so every
# figure is a difference inside one block, and ticks become time through the launch's wall time:
# a block's span, first arrival of pass 0 .. its last tile end, is the kernel's length but for launch overhead.
bspan = t.reshape(ncu, -1).max(axis=1) - t[:, :, 0, 0].min(axis=1)
span = float(np.median(bspan))
TICK_US = wall_us / span


def stat(v):
    v = np.asarray(v, np.float64)
    return {"median_us": round(float(np.median(v)) * TICK_US, 3), "min_us": round(float(v.min()) * TICK_US, 3),
            "max_us": round(float(v.max()) * TICK_US, 3), "median_share_of_kernel": round(float(np.median(v)) / span, 5)}


res = {"config": name, "rows": N, "blocks": ncu, "waves_per_block": NW,
       "wall_us_per_launch_trace_build": round(wall_us, 2), "block_span_ticks_median": span,
       "ticks_per_us": round(span / wall_us, 1),
       "note": "us = ticks x wall time / median block span; share_of_kernel = ticks / median block span", "passes": []}
tot = {"span_gap": 0.0, "tail": 0.0, "idle_before_barrier_mean": 0.0, "first_minus_middle_tile": 0.0,
       "first_tile_state_ready": 0.0}
for p in range(PASSES):
    s = t[:, :, p, :]
    ntile = (s[:, :, 5:] > 0).sum(axis=2)  # tiles of each wave
    tail = s[:, :, 0].max(axis=1) - s[:, :, 0].min(axis=1)
    # what the waves of a block wait at the first barrier on average: the last arrival minus each wave's own
    idle = (s[:, :, 0].max(axis=1, keepdims=True) - s[:, :, 0]).mean(axis=1)
    gap = np.median(s[:, :, 3] - s[:, :, 1], axis=1)
    dma_issue = np.median(s[:, :, 2] - s[:, :, 1], axis=1)
    ready = np.median(s[:, :, 4] - s[:, :, 3], axis=1)
    first = np.median(s[:, :, 5] - s[:, :, 3], axis=1)
    mid_t, last_t = [], []
    for b in range(ncu):
        mids, lasts = [], []
        top = ntile[b].max()
        for w in range(NW):
            k = int(ntile[b, w])
            if k >= 3:
                m = k // 2
                mids.append(s[b, w, 5 + m] - s[b, w, 5 + m - 1])
            if k == top and k >= 2:
                lasts.append(s[b, w, 5 + k - 1] - s[b, w, 5 + k - 2])
        mid_t.append(np.median(mids))
        last_t.append(np.median(lasts))
    pass_len = s.max(axis=(1, 2)) - s[:, :, 0].min(axis=1)
    q = {"pass": p, "tiles_per_wave": [int(ntile.min()), int(ntile.max())],
         "tail": stat(tail), "idle_before_barrier_mean": stat(idle), "span_gap": stat(gap), "dma_issue": stat(dma_issue),
         "first_tile_state_ready": stat(ready), "first_tile": stat(first),
         "middle_tile": stat(mid_t), "last_round_tile": stat(last_t), "pass_length": stat(pass_len)}
    res["passes"].append(q)
    if p > 0:  # pass 0's arrivals are the launch's, not a previous pass's end
        tot["tail"] += q["tail"]["median_share_of_kernel"]
        tot["idle_before_barrier_mean"] += q["idle_before_barrier_mean"]["median_share_of_kernel"]
    tot["span_gap"] += q["span_gap"]["median_share_of_kernel"]
    tot["first_tile_state_ready"] += q["first_tile_state_ready"]["median_share_of_kernel"]
    tot["first_minus_middle_tile"] += q["first_tile"]["median_share_of_kernel"] - q["middle_tile"]["median_share_of_kernel"]
res["share_of_kernel_summed_over_passes"] = {k: round(v, 5) for k, v in tot.items()}
print(json.dumps(res, indent=1))
