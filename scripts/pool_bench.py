"""Times of the max pooling of the conditioning network (zenflow_amd.nn,
``ConditionNet(pool="sum" | "max")``) and of the three reductions of
zf_segment_pool (sum, mean, max) in one run, at the shapes of
scripts/condnet_bench.py.  The yardstick is the sum, whose
kernels are untouched: every figure is also given as a ratio to the sum's in
the same round.  GPU box only; not part of bench.py's contract.

notebook    50,000 x 2 element rows (padded), 1,000 sets with the notebook's
            length distribution, Phi = BatchNorm, 3 x Dense(128) swish,
            Dense(8), Dropout(0.3), the pooling: ``forward`` and ``forward +
            backward`` of one ConditionTrainer per pooling on device-resident
            inputs, by device events.
segment     zf_segment_pool alone on 2^24 x 8 floats (537 MB, past the
            Infinity Cache), without dropout: evenly loaded sets of 256 rows,
            and the same bytes with one set holding half the rows; for the max
            also with the tie counts (one more pass over h), which only a
            train-mode forward asks for.

The legs are alternated round by round in one process.  One JSON line per
(leg group, round) goes to ``--out`` (default profiles/pool_bench.jsonl).

    python scripts/pool_bench.py [--rounds 3] [--only notebook|segment]
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from scripts.condnet_bench import notebook_sets
from scripts.input_grad_bench import timed

POOLS = ("sum", "max")  # of the network; the mean is a standalone reduction (bench_segment)


def bench_notebook(args, lines):
    import zenflow_amd as zf
    from zenflow_amd import _lib as L
    from zenflow_amd import nn
    from zenflow_amd._lib import DeviceArray

    rng = np.random.default_rng(1)
    X, _, off = notebook_sets(rng)
    S, rows = len(off) - 1, len(X)
    Xd, od = DeviceArray.from_numpy(X), DeviceArray.from_numpy(off)
    gcd = DeviceArray.from_numpy(rng.standard_normal((S, 8)).astype(np.float32))
    cd = DeviceArray((S, 8))
    lib, st = L.load_library(), L.stream()
    legs = {}
    for pool in POOLS:
        net = nn.ConditionNet(8, layers=(128,) * 3, dropout=0.3, pool=pool)
        ct = nn.ConditionTrainer(net, net.init(zf.PRNGKey(0), X, off), 2, rows, sets_max=S)
        seed = [0]

        def forward(ct=ct, seed=seed):
            seed[0] += 1
            L.check(lib.zf_condnet_forward(ct.handle, Xd.ptr, rows, od.ptr, S, 1, 1, seed[0], cd.ptr, st), "forward")

        def forward_backward(ct=ct, forward=forward):
            forward()
            L.check(lib.zf_condnet_backward(ct.handle, gcd.ptr, None, st), "backward")

        forward_backward()
        legs[pool] = (ct, forward, forward_backward)
    for rnd in range(args.rounds):
        rec = {"what": "notebook", "rows": rows, "sets": S, "round": rnd}
        for pool in POOLS:
            _, forward, forward_backward = legs[pool]
            for leg, fn in (("forward", forward), ("forward_backward", forward_backward)):
                ms, calls = timed(fn, args.min_seconds)
                rec[f"{pool}_{leg}_ms"], rec[f"{pool}_{leg}_calls"] = round(ms, 5), calls
        for pool in POOLS[1:]:
            for leg in ("forward", "forward_backward"):
                rec[f"{pool}_over_sum_{leg}"] = round(rec[f"{pool}_{leg}_ms"] / rec[f"sum_{leg}_ms"], 4)
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    L.synchronize()


def bench_segment(args, lines):
    from zenflow_amd import _lib as L
    from zenflow_amd._lib import DeviceArray

    lib = L.load_library()
    rows, F, per = 1 << 24, 8, 256
    hd = DeviceArray.from_numpy(np.random.default_rng(3).standard_normal((rows, F), dtype=np.float32))
    even = np.arange(0, rows + 1, per, dtype=np.int64)
    skew = np.concatenate([[0], np.arange(rows // 2, rows + 1, per)]).astype(np.int64)
    codes = {"sum": L.ZF_POOL_SUM, "mean": L.ZF_POOL_MEAN, "max": L.ZF_POOL_MAX}
    legs = {}
    for split, off in (("even", even), ("skewed", skew)):
        S = len(off) - 1
        od, out, cnt = DeviceArray.from_numpy(off), DeviceArray((S, F)), DeviceArray((S, F), np.int32)
        ws = DeviceArray((lib.zf_segment_pool_workspace_bytes(rows, S, F, L.ZF_POOL_MAX),), np.uint8)
        for name, pool, count in (("sum", "sum", None), ("mean", "mean", None), ("max", "max", None),
                                  ("max_counts", "max", cnt)):
            def run(od=od, out=out, ws=ws, S=S, code=codes[pool], count=count):
                L.check(lib.zf_segment_pool(hd.ptr, rows, F, od.ptr, S, code, 0.0, 0, out.ptr, None,
                                            None if count is None else count.ptr, ws.ptr, L.stream()),
                        "zf_segment_pool")
            legs[(split, name)] = (run, S)
    nbytes = rows * F * 4
    for rnd in range(args.rounds):
        rec = {"what": "segment_pool", "rows": rows, "F": F, "bytes_read": nbytes, "round": rnd}
        for (split, name), (run, S) in legs.items():
            ms, calls = timed(run, args.min_seconds)
            rec[f"{split}_sets"] = S
            rec[f"{split}_{name}_ms"], rec[f"{split}_{name}_calls"] = round(ms, 5), calls
        for split in ("even", "skewed"):
            for name in ("mean", "max", "max_counts"):
                rec[f"{split}_{name}_over_sum"] = round(rec[f"{split}_{name}_ms"] / rec[f"{split}_sum_ms"], 4)
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    L.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--only", default="", help="notebook | segment")
    ap.add_argument("--out", default=os.path.join("profiles", "pool_bench.jsonl"))
    args = ap.parse_args()
    lines = []
    if args.only in ("", "notebook"):
        bench_notebook(args, lines)
    if args.only in ("", "segment"):
        bench_segment(args, lines)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
