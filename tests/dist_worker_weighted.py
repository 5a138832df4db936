"""Rank program for tests/test_gpu_train_weighted.py: one rank of a
data-parallel weighted training run (ranks share one GPU through
dist.HostAllgather, as tests/dist_worker.py's ``train_dp``).

``dp``: ``Trainer.loss_grad(..., w=)`` on this rank's shard of the rows and
weights, then ZF_TEST_STEPS weighted steps; loss, gradient and the final blob
go to <outdir>/rank<r>.npz.  ``train_fn``: ``train(..., W_train=, W_test=,
comm=)`` on every rank with the same data and seed.

    python tests/dist_worker_weighted.py <mode> <outdir>   (dp: ZF_TEST_CASE=name:N:seed)"""

import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def train_fn_weights():
    """(W_train, W_test) of the ``train_fn`` mode: the tests' weights recipe
    on the 2400 training and 600 test rows of dist_worker.two_moons_data."""
    from tests.weighted_grad_oracle import make_weights

    return make_weights(2400, 7), make_weights(600, 8)


def _dp(rdzv, outdir):
    from tests.flowcases import build_flow, make_case
    from tests.weighted_grad_oracle import make_weights
    from zenflow_amd import _lib as L
    from zenflow_amd.dist import HostAllgather, shard_rows
    from zenflow_amd.train import Trainer

    name, N, seed = os.environ["ZF_TEST_CASE"].split(":")
    N, seed = int(N), int(seed)
    steps = int(os.environ.get("ZF_TEST_STEPS", "3"))
    case = make_case(name, N=N, seed=seed)
    cfg = case["cfg"]
    flow = build_flow(cfg)
    flow.latent._dim = cfg["D"]
    a, b = shard_rows(N, rdzv.rank, rdzv.world)
    x = case["x"][a:b]
    c = None if case["c"] is None else case["c"][a:b]
    w = make_weights(N, seed)[a:b]
    tr = Trainer(flow, case["variables"], cfg["D"], cfg["C"], b - a, comm=HostAllgather(rdzv))
    loss, g = tr.loss_grad(x, c, global_rows=N, w=w)
    for _ in range(steps):
        tr.step(x, c, global_rows=N, w=w)
    blob = np.empty_like(tr.program.blob)
    L.check(L.load_library().zf_trainer_get_blob(tr.handle, blob.ctypes.data), "get_blob")
    np.savez(Path(outdir, f"rank{rdzv.rank}.npz"), grad=g, loss=np.float64(loss), blob=blob,
             last_loss=np.float64(tr.last_loss()))


def _train_fn(rdzv, outdir):
    import zenflow_amd as zf
    from tests.dist_worker import two_moons_data, two_moons_flow
    from zenflow_amd.dist import HostAllgather
    from zenflow_amd.io import flatten_variables

    X = two_moons_data()
    Wtr, Wte = train_fn_weights()
    best, best_epoch, lt, ls = zf.train(two_moons_flow(), X[:2400], X[2400:],
                                        epochs=int(os.environ.get("ZF_TEST_EPOCHS", "20")), batch_size=512,
                                        progress=False, comm=HostAllgather(rdzv), W_train=Wtr, W_test=Wte)
    np.savez(Path(outdir, f"rank{rdzv.rank}.npz"), best_epoch=best_epoch, lt=np.asarray(lt), ls=np.asarray(ls),
             **{"v:" + k: v for k, v in flatten_variables(best).items()})


def main(mode, outdir):
    from zenflow_amd.launch import FileRendezvous

    rdzv = FileRendezvous.from_env(timeout=120)
    if mode == "dp":
        _dp(rdzv, outdir)
    elif mode == "train_fn":
        _train_fn(rdzv, outdir)
    else:
        raise SystemExit(f"unknown mode {mode!r}")
    rdzv.close()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
