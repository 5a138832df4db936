"""Pins the sample-gradient oracle (tests/sample_grad_oracle.py: the flow's
inverse pass restated in torch for autograd with respect to the parameters, z
and c) to the NumPy oracle: the same float64 x as ``O.flow_inverse`` (1e-12)
on every case the GPU tests use, at most 1% of rows with a non-finite
float64 gradient or log_q, and log_q tied to ``flow_lp`` on x.  CPU only."""

import numpy as np
import pytest

from oracle import zf_oracle as O
from tests import sample_grad_oracle as SG
from tests.flowcases import make_case

# the cases of tests/test_gpu_sample_grad.py (a case added there is added here first)
CASES = [("cfg2", 256, 2), ("cfg4", 256, 3), ("odd", 256, 4), ("k64c1", 256, 5), ("gelu", 256, 8),
         ("bounded", 256, 21), ("cfg4", 3, 88), ("small", 65, 1), ("uniform", 512, 6)]


@pytest.mark.parametrize("name,N,seed", CASES)
def test_inverse_restatement_equals_numpy_oracle(name, N, seed):
    import torch

    from oracle import zf_oracle_torch as OT
    from tests.input_grad_oracle import flow_lp

    case = make_case(name, N=N, seed=seed)
    z, gx, glq = SG.make_inputs(case, N, seed)
    assert z.shape == (N, case["cfg"]["D"]) and z.dtype == np.float32
    x, lq, ok, g, gz, gc = SG.sample_grads(case["model"], case["variables"], z, case["c"], gx, glq, torch.float64)
    c = None if case["c"] is None else case["c"].astype(np.float64)
    ref = O.flow_inverse(case["model"], case["variables"], z.astype(np.float64), c, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(x))
    np.testing.assert_allclose(x[fin], ref[fin], rtol=1e-12, atol=1e-12)
    bad = ~ok | ~np.isfinite(gz).all(axis=1)
    if gc is not None:
        assert gc.shape == c.shape
        bad |= ~np.isfinite(gc).all(axis=1)
    assert bad.mean() <= 0.01, f"{bad.sum()} of {N} rows unusable"
    assert np.abs(gz[~bad]).max() > 0
    leaves = [v for _, v in SG._flat(g)]
    assert max(np.abs(v).max() for v in leaves) > 0
    # log_q is flow_lp on the samples, up to the forward spline's epsilons (den + 1e-5
    # and the clamp move forward(inverse(z)) off z by ~1e-5 of a bin, and with it
    # the next op's log-det and the latent's log_prob, whose slope is up to 50 per dim)
    params = OT._tree(case["variables"]["params"]["bijector"], torch.float64, False)
    stats = case["variables"].get("batch_stats", {}).get("bijector", {})
    lp = flow_lp(OT, case["model"], params, stats, torch.tensor(np.where(fin, x, 0.5)),
                 None if c is None else torch.tensor(c), train=False).numpy()
    both = ok & np.isfinite(lp)
    assert both.mean() >= 0.99
    assert np.abs(lp[both] - lq[both]).max() <= 1e-2


def test_gradient_matches_central_differences():
    """d / d z of sum(gx . x + glq log_q) vs central differences of the float64 restatement."""
    import torch

    name, N, seed = "cfg4", 16, 3
    case = make_case(name, N=N, seed=seed)
    z, gx, glq = SG.make_inputs(case, N, seed)
    z = z.astype(np.float64)

    def total(zz):
        x, lq, ok, _, _, _ = SG.sample_grads(case["model"], case["variables"], zz, case["c"], gx, glq, torch.float64)
        assert ok.all()
        return float((gx * x).sum() + (glq * lq).sum())

    _, _, _, _, gz, _ = SG.sample_grads(case["model"], case["variables"], z, case["c"], gx, glq, torch.float64)
    rng = np.random.default_rng(0)
    for _ in range(6):
        i = (rng.integers(N), rng.integers(2))
        h = 1e-7
        zp, zm = z.copy(), z.copy()
        zp[i] += h
        zm[i] -= h
        fd = (total(zp) - total(zm)) / (2 * h)
        assert abs(gz[i] - fd) <= 1e-4 * abs(fd) + 1e-6, (i, gz[i], fd)
