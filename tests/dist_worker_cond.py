"""Rank program for tests/test_gpu_input_grad.py::test_two_ranks_gc_matches_one_device:
one rank of a data-parallel ``Trainer.loss_grad(..., cond_grad=True)`` on its
shard of the batch (ranks share one GPU through dist.HostAllgather, as
tests/dist_worker.py's ``train_dp``); writes this rank's d loss / d c rows,
the loss and the gradient to <outdir>/rank<r>.npz.

    python tests/dist_worker_cond.py <outdir>      (ZF_TEST_CASE=name:N:seed)"""

import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main(outdir):
    from tests.flowcases import build_flow, make_case
    from zenflow_amd.dist import HostAllgather, shard_rows
    from zenflow_amd.launch import FileRendezvous
    from zenflow_amd.train import Trainer

    rdzv = FileRendezvous.from_env(timeout=120)
    name, N, seed = os.environ["ZF_TEST_CASE"].split(":")
    N, seed = int(N), int(seed)
    case = make_case(name, N=N, seed=seed)
    cfg = case["cfg"]
    flow = build_flow(cfg)
    flow.latent._dim = cfg["D"]
    a, b = shard_rows(N, rdzv.rank, rdzv.world)
    tr = Trainer(flow, case["variables"], cfg["D"], cfg["C"], b - a, comm=HostAllgather(rdzv))
    loss, g, gc = tr.loss_grad(case["x"][a:b], case["c"][a:b], global_rows=N, cond_grad=True)
    np.savez(Path(outdir, f"rank{rdzv.rank}.npz"), gc=gc, grad=g, loss=np.float64(loss), lo=a, hi=b)
    rdzv.close()


if __name__ == "__main__":
    main(sys.argv[1])
