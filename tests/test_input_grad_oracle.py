"""Pins the input-gradient oracle (tests/input_grad_oracle.py: the eval-mode
flow restated in torch for autograd with respect to x and c) to the NumPy
oracle: the same float64 eval log_prob (1e-12) on every case the GPU tests
use, and at most 1% of rows with a non-finite log_prob or gradient (the rows
the GPU comparison has to leave out).  CPU only."""

import numpy as np
import pytest

from oracle import zf_oracle as O
from tests import input_grad_oracle as IG
from tests.flowcases import make_case

# the eval cases of tests/test_gpu_input_grad.py (a case added there is added here first)
CASES = [("small", 256, 1), ("cfg2", 256, 2), ("cfg4", 256, 3), ("odd", 300, 4), ("deep", 256, 5),
         ("uniform", 256, 6), ("d7k32c2", 256, 7), ("gelu", 256, 8), ("mixed", 256, 9), ("h384c2", 256, 10),
         ("cfg2", 4096, 11)]


def _job(case):
    job = {"model": case["model"], "variables": case["variables"], "x": case["x"], "mode": "eval"}
    if case["c"] is not None:
        job["c"] = case["c"]
    return job


@pytest.mark.parametrize("name,N,seed", CASES)
def test_eval_restatement_equals_numpy_oracle(name, N, seed):
    import torch

    case = make_case(name, N=N, seed=seed)
    lp, gx, gc = IG.eval_grads(_job(case), torch.float64)
    x = case["x"].astype(np.float64)
    c = None if case["c"] is None else case["c"].astype(np.float64)
    ref, _ = O.flow_log_prob(case["model"], case["variables"], x, c, dtype=np.float64)
    got = O.jnp_nan_to_num(lp, nan=-np.inf)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
    bad = ~np.isfinite(lp) | ~np.isfinite(gx).all(axis=1)
    if gc is not None:
        assert gc.shape == c.shape
        bad |= ~np.isfinite(gc).all(axis=1)
    assert bad.mean() <= 0.01, f"{bad.sum()} of {N} rows unusable"
    assert gx.shape == x.shape and np.abs(gx[~bad]).max() > 0


def test_job_file_round_trip(tmp_path):
    case = make_case("cfg4", N=8, seed=3)
    IG.pack_job(tmp_path / "j.npz", case["model"], case["variables"], case["x"], case["c"], cot=np.arange(8.0))
    job = IG.load_job(tmp_path / "j.npz")
    assert job["mode"] == "eval" and job["model"]["latent"] == case["model"]["latent"]
    np.testing.assert_array_equal(job["x"], case["x"])
    k = case["variables"]["params"]["bijector"]["bijectors_1"]["Dense_0"]["kernel"]
    np.testing.assert_array_equal(job["variables"]["params"]["bijector"]["bijectors_1"]["Dense_0"]["kernel"], k)


def test_train_mode_gc_matches_central_differences():
    """d loss / d c of the train-mode loss vs central differences of the NumPy oracle's fp64 loss."""
    import torch

    case = make_case("cfg4", N=64, seed=12)
    job = _job(case)
    job["mode"] = "train"
    loss, gc, _, _ = IG.train_grads(job, torch.float64)

    def np_loss(c):
        lp, _ = O.flow_log_prob(case["model"], case["variables"], case["x"].astype(np.float64), c, train=True,
                                dtype=np.float64)
        return -lp.mean()

    c0 = case["c"].astype(np.float64)
    assert loss == pytest.approx(np_loss(c0), rel=1e-12, abs=1e-12)
    rng = np.random.default_rng(0)
    for _ in range(6):
        i = (rng.integers(64), rng.integers(2))
        h = 1e-6
        cp, cm = c0.copy(), c0.copy()
        cp[i] += h
        cm[i] -= h
        fd = (np_loss(cp) - np_loss(cm)) / (2 * h)
        assert abs(gc[i] - fd) <= 1e-4 * abs(fd) + 1e-8, (i, gc[i], fd)
