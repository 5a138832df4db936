"""Time of the eval-mode input gradient (``BoundFlow.log_prob_and_grad``)
beside ``Trainer.loss_grad`` and the fused ``log_prob`` at the same shapes.
GPU box only; not part of bench.py's contract.

Device events around batches of calls on device-resident inputs, after a
warm-up; every figure covers at least ``--min-seconds`` of device work.  The
VJP and loss_grad are alternated round by round in one process, so each round
compares them under the same clocks.  One JSON line per (config, rows, round)
goes to ``--out`` (default profiles/input_grad_bench.jsonl).

The VJP does strictly less work than loss_grad (no weight-gradient GEMMs, no
batch reductions), so ``vjp_ms < loss_grad_ms`` is expected in every round;
``vjp_below_loss_grad`` records whether it held.

    python scripts/input_grad_bench.py [--configs cfg2,cfg4] [--rows 1024,65536] [--rounds 3]
    python scripts/input_grad_bench.py --only vjp --configs cfg2 --rows 1024   (for a kernel trace)
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np


def timed(fn, min_seconds):
    """ms per call of fn (launches on the library stream), by device events."""
    from zenflow_amd import _lib as L

    for _ in range(3):
        fn()
    L.synchronize()
    reps, total_ms, calls = 4, 0.0, 0
    while total_ms < min_seconds * 1e3:
        a, b = L.Event(), L.Event()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        total_ms += a.elapsed_ms(b)
        calls += reps
        reps = min(reps * 2, 4096)
    return total_ms / calls, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg4")
    ap.add_argument("--rows", default="1024,65536")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--only", default="", help="vjp | loss_grad | log_prob: time that leg alone")
    ap.add_argument("--out", default=os.path.join("profiles", "input_grad_bench.jsonl"))
    args = ap.parse_args()

    import ctypes as ct

    from tests.flowcases import build_flow, make_case
    from zenflow_amd import _lib as L
    from zenflow_amd._lib import DeviceArray
    from zenflow_amd.train import Trainer

    lib = L.load_library()
    lines = []
    for name in args.configs.split(","):
        for N in [int(r) for r in args.rows.split(",")]:
            case = make_case(name, N=N, seed=5)
            cfg = case["cfg"]
            flow = build_flow(cfg)
            flow.latent._dim = cfg["D"]
            bf = flow.bind(case["variables"], cfg["D"], cfg["C"])
            tr = Trainer(flow, case["variables"], cfg["D"], cfg["C"], N)
            xd = DeviceArray.from_numpy(np.ascontiguousarray(case["x"]))
            cd = None if case["c"] is None else DeviceArray.from_numpy(np.ascontiguousarray(case["c"]))
            cptr = None if cd is None else cd.ptr
            # preallocated outputs and raw entry points: the device work, not Python's allocations
            h = bf.program.vjp_handle(N)
            lp, dx = DeviceArray((N,)), DeviceArray((N, cfg["D"]))
            dc = DeviceArray((N, cfg["C"])) if cfg["C"] else None
            g, loss = DeviceArray((tr.program.blob.size,)), DeviceArray((1,), np.float64)
            st = L.stream()

            def vjp():
                L.check(lib.zf_trainer_log_prob_vjp(h.handle, xd.ptr, cptr, None, lp.ptr, dx.ptr,
                                                    None if dc is None else dc.ptr, N, st), "vjp")

            def loss_grad():
                L.check(lib.zf_trainer_loss_grad_shard(tr.handle, xd.ptr, cptr, N, N, 0, loss.ptr, g.ptr, st),
                        "loss_grad")

            def log_prob():
                bf.log_prob(xd, cd, out=lp)

            legs = {"vjp": vjp, "loss_grad": loss_grad, "log_prob": log_prob}
            if args.only:
                ms, calls = timed(legs[args.only], args.min_seconds)
                lines.append({"config": name, "rows": N, args.only + "_ms": round(ms, 5), "calls": calls})
                print(json.dumps(lines[-1]), flush=True)
                continue
            for rnd in range(args.rounds):
                rec = {"config": name, "rows": N, "round": rnd, "variant": bf.program.kernel_variant}
                for leg in ("vjp", "loss_grad", "log_prob"):
                    ms, calls = timed(legs[leg], args.min_seconds)
                    rec[leg + "_ms"] = round(ms, 5)
                    rec[leg + "_calls"] = calls
                rec["vjp_below_loss_grad"] = rec["vjp_ms"] < rec["loss_grad_ms"]
                lines.append(rec)
                print(json.dumps(rec), flush=True)
            del tr, h
    if not args.only:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
