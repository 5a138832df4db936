"""Time of a custom-loss step — ``zf_trainer_forward`` + ``zf_trainer_backward``
+ ``zf_trainer_apply_gradient`` — beside what it is built from, at the same
shapes.  GPU box only; not part of bench.py's contract.

* train mode against the eager ``step`` (ZF_TRAIN_GRAPH=0): the same kernels
  plus the loss reduction, minus one latent launch;
* eval mode against ``log_prob_vjp``, which runs the same forward and input
  reverse without the weight-gradient GEMMs, the BatchNorm sums, the gradient
  cast and the optimiser.

Device events around batches of calls on device-resident inputs, after a
warm-up; every figure covers at least ``--min-seconds`` of device work.  The
legs are alternated round by round in one process, so each round compares
them under the same clocks.  The cotangent is -1/N (the NLL's), resident on
the device: the user's own loss is not in the figures.  One JSON line per
(config, rows, round) goes to ``--out`` (default profiles/custom_loss_bench.jsonl).

    python scripts/custom_loss_bench.py [--configs cfg2,cfg4] [--rows 1024,65536] [--rounds 3]
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
    ap.add_argument("--out", default=os.path.join("profiles", "custom_loss_bench.jsonl"))
    args = ap.parse_args()

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
            D, C = cfg["D"], cfg["C"]
            flow = build_flow(cfg)
            flow.latent._dim = D

            def trainer():
                return Trainer(flow, case["variables"], D, C, N)

            tr_train, tr_eval, tr_vjp = trainer(), trainer(), trainer()
            os.environ["ZF_TRAIN_GRAPH"] = "0"  # read at zf_trainer_create: this trainer steps eagerly
            tr_step = trainer()
            del os.environ["ZF_TRAIN_GRAPH"]
            xd = DeviceArray.from_numpy(np.ascontiguousarray(case["x"]))
            cd = None if case["c"] is None else DeviceArray.from_numpy(np.ascontiguousarray(case["c"]))
            cptr = None if cd is None else cd.ptr
            cot = DeviceArray.from_numpy(np.full(N, -1.0 / N, np.float32))
            lp, dx = DeviceArray((N,)), DeviceArray((N, D))
            gc = DeviceArray((N, C)) if C else None
            gcptr = None if gc is None else gc.ptr
            loss = DeviceArray((1,), np.float64)
            st = L.stream()

            def custom(tr, train):
                def run():
                    L.check(lib.zf_trainer_forward(tr.handle, xd.ptr, cptr, N, N, train, train, lp.ptr, st), "forward")
                    L.check(lib.zf_trainer_backward(tr.handle, cot.ptr, None, gcptr, st), "backward")
                    L.check(lib.zf_trainer_apply_gradient(tr.handle, None, st), "apply_gradient")
                return run

            def step():
                L.check(lib.zf_trainer_step_cond_shard(tr_step.handle, xd.ptr, cptr, N, N, loss.ptr, gcptr, st), "step")

            def vjp():
                L.check(lib.zf_trainer_log_prob_vjp(tr_vjp.handle, xd.ptr, cptr, cot.ptr, lp.ptr, dx.ptr, gcptr, N, st),
                        "vjp")

            legs = {"custom_train": custom(tr_train, 1), "step_eager": step, "custom_eval": custom(tr_eval, 0),
                    "vjp": vjp}
            for rnd in range(args.rounds):
                rec = {"config": name, "rows": N, "round": rnd}
                for leg, fn in legs.items():
                    ms, calls = timed(fn, args.min_seconds)
                    rec[leg + "_ms"] = round(ms, 5)
                    rec[leg + "_calls"] = calls
                rec["train_over_step"] = round(rec["custom_train_ms"] / rec["step_eager_ms"], 4)
                rec["eval_over_vjp"] = round(rec["custom_eval_ms"] / rec["vjp_ms"], 4)
                lines.append(rec)
                print(json.dumps(rec), flush=True)
            del tr_train, tr_eval, tr_vjp, tr_step
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
