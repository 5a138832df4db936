"""Optimiser chains under data parallelism.  After the trainer's gradient
reduction every rank holds the same gradient bits (tree_cols_cast_kernel), so
the global norm of clip_by_global_norm needs no communication: each rank sums
the same squares in the same order.  Two ranks sharing this box's GPU
(tests/dist_worker_optim.py, dist.HostAllgather) take 3 steps of
chain(clip_by_global_norm(0.5 n1), nadamw(cosine_decay_schedule(3e-3, 3))) on
their halves of cfg2 x 1024; both must end with one device's blob, gradient
norms and learning rates — ``array_equal``, not a tolerance."""

import os
from pathlib import Path

import numpy as np
import pytest

from tests.test_gpu_train import _setup

pytestmark = pytest.mark.gpu
WORKER = str(Path(__file__).resolve().parent / "dist_worker_optim.py")


def test_two_ranks_chain_matches_one_device_bitwise(tmp_path):
    from tests.dist_worker_optim import make_chain, run
    from zenflow_amd.launch import spawn

    name, N, seed, steps = "cfg2", 1024, 86, 3
    case, flow, probe = _setup(name, N, seed)
    _, g = probe.loss_grad(case["x"], case["c"])
    n1 = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    del probe
    env = dict(os.environ, ZF_TEST_CASE=f"{name}:{N}:{seed}", ZF_TEST_STEPS=str(steps), ZF_DEVICE="0",
               ZF_TEST_MAX_NORM=(0.5 * n1).hex())
    assert spawn(2, [WORKER, str(tmp_path)], env=env, timeout=240) == 0
    ranks = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]

    _, _, tr = _setup(name, N, seed, optimizer=make_chain(0.5 * n1, steps))  # one device, the whole batch
    blob, norms, lrs = run(tr, case["x"], case["c"], steps)
    assert norms[0] == pytest.approx(n1, rel=1e-12) and norms[0] > 0.5 * n1  # step 1 is clipped
    assert lrs[0] == float(np.float32(3e-3)) and lrs[2] < lrs[1] < lrs[0]
    for k, r in enumerate(ranks):
        assert np.array_equal(r["norms"], norms), f"rank {k}: grad_norm {r['norms']} vs {norms}"
        assert np.array_equal(r["lrs"], lrs), f"rank {k}: learning_rate {r['lrs']} vs {lrs}"
        assert np.array_equal(r["blob"], blob, equal_nan=True), f"rank {k}: {np.sum(r['blob'] != blob)} blob entries"
