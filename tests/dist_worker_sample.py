"""Rank program for tests/test_gpu_sample_grad.py: one rank of a data-parallel
``Trainer.sample_forward / sample_backward`` (ranks share one GPU through
dist.HostAllgather, as tests/dist_worker_custom.py).

This rank's shard of the latent rows, the conditions and the cotangents goes
through ``sample_forward`` and ``sample_backward``; its x, log_q and the
gradient go to <outdir>/rank<r>.npz.

    python tests/dist_worker_sample.py <outdir>   (ZF_TEST_CASE=name:N:seed)"""

import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main(outdir):
    from tests.flowcases import build_flow, make_case
    from tests.sample_grad_oracle import make_inputs
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
    z, gx, glq = make_inputs(case, N, seed)
    a, b = shard_rows(N, rdzv.rank, rdzv.world)
    tr = Trainer(flow, case["variables"], cfg["D"], cfg["C"], b - a, comm=HostAllgather(rdzv))
    x, lq = tr.sample_forward(case["c"][a:b] if cfg["C"] else b - a, z=z[a:b], global_rows=N)
    g = tr.sample_backward(gx[a:b], glq[a:b])
    np.savez(Path(outdir, f"rank{rdzv.rank}.npz"), x=x, lq=lq, grad=g)
    rdzv.close()


if __name__ == "__main__":
    main(sys.argv[1])
