"""Cost of the input gradient and of the segment repeat (zenflow_amd.nn,
zf_condnet_backward_input, zf_segment_repeat) at the shape of
examples/deep_set.ipynb: 50,000 x 2 element rows (padded), 1,000 sets with the
notebook's length distribution, Phi = [BatchNorm,] 3 x Dense(128) swish,
Dense(8), Dropout(0.3), sum.  GPU box only; not part of bench.py's contract.

input    ``forward + backward`` against ``forward + backward_input`` of the
         ConditionTrainer, with and without BatchNorm, on device-resident
         inputs by device events, alternated round by round in one process.
         The difference is what d / d x costs: one bn_bwd_kernel launch with
         BatchNorm, one (rows x 128) -> (rows x 2) GEMM without.
train    ``forward + backward + apply_gradient`` (the entries that existed
         before), for an A/B of two libraries: run once per library with
         ``ZF_LIB=...`` (and ``ZF_ALLOW_MISSING_SYMBOLS=1`` for the older one),
         alternating, appending to the same ``--out``; the record carries
         ``--label``.
repeat   zf_segment_repeat alone, 1,000 sets -> 100,000 rows, F = 8 (100
         samples per set, ``DeepSetFlow.sample``): the bytes it must move (c
         and the offsets read, out written) over time as a fraction of the
         6.29 TB/s float4 copy (MI355X_MICROARCH.md).

One JSON line per (leg group, round) is appended to ``--out`` (default
profiles/deepset_bench.jsonl).

    python scripts/deepset_bench.py [--rounds 3] [--only input|train|repeat] [--label NAME]
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from scripts.condnet_bench import COPY_RATE, notebook_sets
from scripts.input_grad_bench import timed


def _trainer(batch_norm):
    import zenflow_amd as zf
    from zenflow_amd import nn
    from zenflow_amd._lib import DeviceArray

    rng = np.random.default_rng(1)
    X, _, off = notebook_sets(rng)
    S, rows = len(off) - 1, len(X)
    net = nn.ConditionNet(8, layers=(128,) * 3, batch_norm=batch_norm, dropout=0.3, pool="sum")
    v = net.init(zf.PRNGKey(0), X, off)
    ct = nn.ConditionTrainer(net, v, 2, rows, sets_max=S)
    Xd, od = DeviceArray.from_numpy(X), DeviceArray.from_numpy(off)
    gcd = DeviceArray.from_numpy(rng.standard_normal((S, 8)).astype(np.float32))
    return ct, Xd, od, gcd, rows, S


def bench_input(args, lines):
    from zenflow_amd import _lib as L
    from zenflow_amd._lib import DeviceArray

    lib, st = L.load_library(), L.stream()
    for bn in (True, False):
        ct, Xd, od, gcd, rows, S = _trainer(bn)
        cd, gxd = DeviceArray((S, 8)), DeviceArray((rows, 2))
        seed = [0]

        def forward():
            seed[0] += 1
            L.check(lib.zf_condnet_forward(ct.handle, Xd.ptr, rows, od.ptr, S, 1, 1, seed[0], cd.ptr, st), "forward")

        def forward_backward():
            forward()
            L.check(lib.zf_condnet_backward(ct.handle, gcd.ptr, None, st), "backward")

        def forward_backward_input():
            forward()
            L.check(lib.zf_condnet_backward_input(ct.handle, gcd.ptr, None, gxd.ptr, st), "backward_input")

        for rnd in range(args.rounds):
            rec = {"what": "input_gradient", "batch_norm": bn, "rows": rows, "sets": S, "round": rnd}
            for leg, fn in (("forward", forward), ("forward_backward", forward_backward),
                            ("forward_backward_input", forward_backward_input)):
                ms, calls = timed(fn, args.min_seconds)
                rec[leg + "_ms"], rec[leg + "_calls"] = round(ms, 5), calls
            rec["backward_ms"] = round(rec["forward_backward_ms"] - rec["forward_ms"], 5)
            rec["backward_input_ms"] = round(rec["forward_backward_input_ms"] - rec["forward_ms"], 5)
            rec["input_gradient_ms"] = round(rec["forward_backward_input_ms"] - rec["forward_backward_ms"], 5)
            lines.append(rec)
            print(json.dumps(rec), flush=True)
        L.synchronize()


def bench_train(args, lines):
    from zenflow_amd import _lib as L
    from zenflow_amd._lib import DeviceArray

    lib, st = L.load_library(), L.stream()
    ct, Xd, od, gcd, rows, S = _trainer(True)
    cd = DeviceArray((S, 8))
    seed = [0]

    def train_step():
        seed[0] += 1
        L.check(lib.zf_condnet_forward(ct.handle, Xd.ptr, rows, od.ptr, S, 1, 1, seed[0], cd.ptr, st), "forward")
        L.check(lib.zf_condnet_backward(ct.handle, gcd.ptr, None, st), "backward")
        L.check(lib.zf_condnet_apply_gradient(ct.handle, None, st), "apply_gradient")

    for rnd in range(args.rounds):
        ms, calls = timed(train_step, args.min_seconds)
        rec = {"what": "forward_backward_apply", "label": args.label, "lib": os.environ.get("ZF_LIB", ""), "rows": rows,
               "sets": S, "round": rnd, "ms": round(ms, 5), "calls": calls}
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    L.synchronize()


def bench_repeat(args, lines):
    from zenflow_amd import _lib as L
    from zenflow_amd._lib import DeviceArray

    lib = L.load_library()
    S, per, F = 1000, 100, 8
    rows = S * per
    cd = DeviceArray.from_numpy(np.random.default_rng(3).standard_normal((S, F), dtype=np.float32))
    od = DeviceArray.from_numpy(np.arange(0, rows + 1, per, dtype=np.int64))
    out = DeviceArray((rows, F))
    ws = DeviceArray((lib.zf_segment_workspace_bytes(rows, S, F),), np.uint8)

    def run():
        L.check(lib.zf_segment_repeat(cd.ptr, S, F, od.ptr, rows, out.ptr, None, ws.ptr, L.stream()),
                "zf_segment_repeat")

    nbytes = S * F * 4 + (S + 1) * 8 + rows * F * 4
    for rnd in range(args.rounds):
        ms, calls = timed(run, args.min_seconds)
        rec = {"what": "segment_repeat", "sets": S, "rows": rows, "F": F, "bytes_moved": nbytes, "round": rnd,
               "ms": round(ms, 6), "calls": calls, "fraction_of_copy_rate": round(nbytes / (ms * 1e-3) / COPY_RATE, 5)}
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    L.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--only", default="", help="input | train | repeat")
    ap.add_argument("--label", default="this", help="name of the library in the train records")
    ap.add_argument("--out", default=os.path.join("profiles", "deepset_bench.jsonl"))
    args = ap.parse_args()
    lines = []
    if args.only in ("", "input"):
        bench_input(args, lines)
    if args.only in ("", "train"):
        bench_train(args, lines)
    if args.only in ("", "repeat"):
        bench_repeat(args, lines)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
