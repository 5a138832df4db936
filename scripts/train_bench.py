"""Training-step throughput: samples/s of
``Trainer.step`` (train-mode forward + reverse pass + nadamw update) for a
few batch sizes on the BASELINE configs.  GPU box only; not part of bench.py's
contract (the headline metric is the eval-mode log_prob).

    python scripts/train_bench.py [--configs cfg1,cfg2,cfg5] [--batches 1024,16384,65536]
                                  [--optimizer legacy|chain|clip] [--reps R]

``--optimizer``: ``legacy`` the trainer's own nadamw (adam_kernel), ``chain``
the same update as ``optim.nadamw`` (prologue + chain_update_kernel), ``clip``
``optim.chain(optim.clip_by_global_norm(1.0), optim.nadamw(...))`` (one launch
more: the sum of squares).  ``--reps``: timed repetitions per row (the
run-to-run spread on the box).
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg1,cfg2,cfg5")
    ap.add_argument("--batches", default="1024,16384,65536")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--optimizer", choices=("legacy", "chain", "clip"), default="legacy")
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--tag", default="")
    ap.add_argument("--weighted", action="store_true", help="the weighted loss: Trainer.step(w=...)")
    args = ap.parse_args()

    from tests.flowcases import build_flow, make_case
    from zenflow_amd import _lib as L
    from zenflow_amd._lib import DeviceArray
    from zenflow_amd.train import Trainer

    def optimizer():
        if args.optimizer == "legacy":
            return None
        import zenflow_amd.optim as optim

        nadamw = optim.nadamw(1e-3)
        return nadamw if args.optimizer == "chain" else optim.chain(optim.clip_by_global_norm(1.0), nadamw)

    for name in args.configs.split(","):
        for B in [int(b) for b in args.batches.split(",")]:
            case = make_case(name, N=B, seed=5)
            cfg = case["cfg"]
            flow = build_flow(cfg)
            flow.latent._dim = cfg["D"]
            tr = Trainer(flow, case["variables"], cfg["D"], cfg["C"], B, optimizer=optimizer())
            xd = DeviceArray.from_numpy(np.ascontiguousarray(case["x"]))
            cd = None if case["c"] is None else DeviceArray.from_numpy(np.ascontiguousarray(case["c"]))
            wd = None
            if args.weighted:  # exponential weights, an eighth of them zero, a sixteenth negative
                rng = np.random.default_rng(1005)
                w = rng.exponential(1.0, B).astype(np.float32)
                w[rng.choice(B, B // 8, replace=False)] = 0.0
                w[rng.choice(B, B // 16, replace=False)] = -0.25
                wd = DeviceArray.from_numpy(w)
            for _ in range(3):
                tr.step(xd, cd, w=wd)
            for rep in range(args.reps):
                L.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    tr.step(xd, cd, w=wd)
                L.synchronize()
                dt = (time.perf_counter() - t0) / args.steps
                rec = {"config": name, "batch": B, "optimizer": args.optimizer, "weighted": bool(args.weighted),
                       "ms_per_step": round(dt * 1e3, 4), "samples_per_s": round(B / dt), "loss": tr.last_loss()}
                if args.tag:
                    rec["tag"] = args.tag
                if args.reps > 1:
                    rec["rep"] = rep
                print(json.dumps(rec), flush=True)
            del tr


if __name__ == "__main__":
    main()
