"""Rank program for tests/test_gpu_custom_loss.py: one rank of a data-parallel
``Trainer.forward / backward / apply_gradient`` (ranks share one GPU through
dist.HostAllgather, as tests/dist_worker_weighted.py).

This rank's shard of the rows and of the cotangent goes through ``forward``
(ZF_TEST_MODE train | eval), ``backward`` and ``apply_gradient``; its lp, the
gradient and the blob after the update go to <outdir>/rank<r>.npz.

    python tests/dist_worker_custom.py <outdir>   (ZF_TEST_CASE=name:N:seed)"""

import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main(outdir):
    from tests.custom_loss_oracle import make_cot
    from tests.flowcases import _blob, build_flow, make_case
    from zenflow_amd.dist import HostAllgather, shard_rows
    from zenflow_amd.launch import FileRendezvous
    from zenflow_amd.train import Trainer

    rdzv = FileRendezvous.from_env(timeout=120)
    name, N, seed = os.environ["ZF_TEST_CASE"].split(":")
    N, seed = int(N), int(seed)
    train = os.environ["ZF_TEST_MODE"] == "train"
    case = make_case(name, N=N, seed=seed)
    cfg = case["cfg"]
    flow = build_flow(cfg)
    flow.latent._dim = cfg["D"]
    a, b = shard_rows(N, rdzv.rank, rdzv.world)
    x = case["x"][a:b]
    c = None if case["c"] is None else case["c"][a:b]
    cot = make_cot(N, seed).astype(np.float32)[a:b]
    tr = Trainer(flow, case["variables"], cfg["D"], cfg["C"], b - a, comm=HostAllgather(rdzv))
    lp = tr.forward(x, c, train=train, global_rows=N)
    g = tr.backward(cot)
    tr.apply_gradient(g)
    np.savez(Path(outdir, f"rank{rdzv.rank}.npz"), lp=lp, grad=g, blob=_blob(tr))
    rdzv.close()


if __name__ == "__main__":
    main(sys.argv[1])
