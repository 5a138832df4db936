"""Rank program for tests/test_gpu_optim_dp.py: one rank of data-parallel
training with an optimiser chain (ranks share one GPU through
dist.HostAllgather, as tests/dist_worker.py's ``train_dp``).  ZF_TEST_STEPS
steps of chain(clip_by_global_norm(ZF_TEST_MAX_NORM), nadamw(cosine decay))
on this rank's shard; the final blob and, per step, the gradient norm and the
learning rate the step used go to <outdir>/rank<r>.npz.

    python tests/dist_worker_optim.py <outdir>      (ZF_TEST_CASE=name:N:seed)"""

import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def make_chain(max_norm, steps):
    import zenflow_amd.optim as optim

    return optim.chain(optim.clip_by_global_norm(max_norm), optim.nadamw(optim.cosine_decay_schedule(3e-3, steps)))


def run(tr, x, c, steps, global_rows=None):
    """``steps`` steps; (blob, grad_norm per step, learning_rate per step)."""
    from zenflow_amd import _lib as L

    norms, lrs = [], []
    for _ in range(steps):
        tr.step(x, c, global_rows=global_rows)
        st = tr.opt_state()
        norms.append(st["grad_norm"])
        lrs.append(st["learning_rate"])
    blob = np.empty_like(tr.program.blob)
    L.check(L.load_library().zf_trainer_get_blob(tr.handle, blob.ctypes.data), "get_blob")
    return blob, np.asarray(norms, np.float64), np.asarray(lrs, np.float64)


def main(outdir):
    from tests.flowcases import build_flow, make_case
    from zenflow_amd.dist import HostAllgather, shard_rows
    from zenflow_amd.launch import FileRendezvous
    from zenflow_amd.train import Trainer

    rdzv = FileRendezvous.from_env(timeout=120)
    name, N, seed = os.environ["ZF_TEST_CASE"].split(":")
    N, seed = int(N), int(seed)
    steps = int(os.environ.get("ZF_TEST_STEPS", "3"))
    case = make_case(name, N=N, seed=seed)
    cfg = case["cfg"]
    flow = build_flow(cfg)
    flow.latent._dim = cfg["D"]
    a, b = shard_rows(N, rdzv.rank, rdzv.world)
    chain = make_chain(float.fromhex(os.environ["ZF_TEST_MAX_NORM"]), steps)
    tr = Trainer(flow, case["variables"], cfg["D"], cfg["C"], b - a, optimizer=chain, comm=HostAllgather(rdzv))
    blob, norms, lrs = run(tr, case["x"][a:b], None if case["c"] is None else case["c"][a:b], steps, N)
    np.savez(Path(outdir, f"rank{rdzv.rank}.npz"), blob=blob, norms=norms, lrs=lrs)
    rdzv.close()


if __name__ == "__main__":
    main(sys.argv[1])
