"""Time of a pass through sampling — ``zf_trainer_sample_forward`` +
``zf_trainer_sample_backward`` — beside the eval-mode custom-loss pass
``zf_trainer_forward(train = 0)`` + ``zf_trainer_backward`` of the same
trainer, at the same shapes.  GPU box only; not part of bench.py's contract.

The two legs run the same conditioner GEMMs, weight-gradient GEMMs, BatchNorm
sums and gradient cast; they differ in the spline kernels (the inverse with
its log-det and the reverse of the root formula against the forward spline
and its reverse) and in a few row kernels.  The eval custom-loss leg is the
yardstick: profiles/custom_loss_bench.jsonl holds its figures on the parent.

Device events around batches of calls on device-resident inputs, after a
warm-up; every figure covers at least ``--min-seconds`` of device work.  The
legs are alternated round by round in one process, so each round compares
them under the same clocks.  The cotangents are resident on the device (gx
standard normal, glq = 1/N): the user's own loss is not in the figures.  One
JSON line per (config, rows, round) goes to ``--out`` (default
profiles/sample_grad_bench.jsonl).

    python scripts/sample_grad_bench.py [--configs cfg2,cfg4] [--rows 1024,65536] [--rounds 3]
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from scripts.input_grad_bench import timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg4")
    ap.add_argument("--rows", default="1024,65536")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join("profiles", "sample_grad_bench.jsonl"))
    args = ap.parse_args()

    from tests.flowcases import build_flow, make_case
    from tests.sample_grad_oracle import make_inputs
    from zenflow_amd import _lib as L
    from zenflow_amd._lib import DeviceArray
    from zenflow_amd.train import Trainer

    lib = L.load_library()
    lines = []
    for name in args.configs.split(","):
        for N in [int(r) for r in args.rows.split(",")]:
            case = make_case(name, N=N, seed=5)
            cfg = case["cfg"]
            D, C = cfg["D"], cfg["C"]
            flow = build_flow(cfg)
            flow.latent._dim = D
            tr_sample = Trainer(flow, case["variables"], D, C, N)
            tr_eval = Trainer(flow, case["variables"], D, C, N)
            z, gx, _ = make_inputs(case, N, 5)
            xd = DeviceArray.from_numpy(np.ascontiguousarray(case["x"]))
            zd, gxd = DeviceArray.from_numpy(z), DeviceArray.from_numpy(gx)
            cd = None if case["c"] is None else DeviceArray.from_numpy(np.ascontiguousarray(case["c"]))
            cptr = None if cd is None else cd.ptr
            cot = DeviceArray.from_numpy(np.full(N, -1.0 / N, np.float32))
            glq = DeviceArray.from_numpy(np.full(N, 1.0 / N, np.float32))
            lp, xo, lq = DeviceArray((N,)), DeviceArray((N, D)), DeviceArray((N,))
            gc = DeviceArray((N, C)) if C else None
            gcptr = None if gc is None else gc.ptr
            st = L.stream()

            def sample():
                L.check(lib.zf_trainer_sample_forward(tr_sample.handle, zd.ptr, cptr, N, N, xo.ptr, lq.ptr, st),
                        "sample_forward")
                L.check(lib.zf_trainer_sample_backward(tr_sample.handle, gxd.ptr, glq.ptr, None, None, gcptr, st),
                        "sample_backward")

            def custom_eval():
                L.check(lib.zf_trainer_forward(tr_eval.handle, xd.ptr, cptr, N, N, 0, 0, lp.ptr, st), "forward")
                L.check(lib.zf_trainer_backward(tr_eval.handle, cot.ptr, None, gcptr, st), "backward")

            legs = {"sample": sample, "custom_eval": custom_eval}
            for rnd in range(args.rounds):
                rec = {"config": name, "rows": N, "round": rnd}
                for leg, fn in legs.items():
                    ms, calls = timed(fn, args.min_seconds)
                    rec[leg + "_ms"] = round(ms, 5)
                    rec[leg + "_calls"] = calls
                rec["sample_over_eval"] = round(rec["sample_ms"] / rec["custom_eval_ms"], 4)
                lines.append(rec)
                print(json.dumps(rec), flush=True)
            del tr_sample, tr_eval
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
