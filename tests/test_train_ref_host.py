"""tests/train_ref.py on the host: the tolerance the GPU trajectory test
(tests/test_gpu_train_trajectory.py) holds adam_kernel to is wide enough for
a correct fp32 evaluation of the update and narrow enough to catch a wrong
one.

The fp32 side is ``adam_kernel_f32``, the kernel's arithmetic operation by
operation in NumPy float32; the float64 side is ``adam_reference``, teacher
forced as in the GPU test: every step starts from the fp32 parameters, the
float64 moments are carried from the same gradients."""

import numpy as np
import pytest

from tests import train_ref as R

STEPS = 16
N = 4096


def _problem(seed=5):
    """Parameters on the scale of a conditioner's weights, and STEPS gradients
    per element: magnitudes 1e-12 .. 10, a quarter of the elements with
    alternating sign (m cancels), a quarter with random signs, one in sixteen
    exactly zero throughout (dead units), some zero on single steps."""
    rng = np.random.default_rng(seed)
    theta = (0.3 * rng.standard_normal(N)).astype(np.float32)
    theta[:8] = 0.0
    mag = 10.0 ** rng.uniform(-12, 1, N)
    g = mag[None, :] * (1 + 0.3 * rng.standard_normal((STEPS, N)))
    kind = rng.integers(0, 4, N)
    alt = (-1.0) ** np.arange(STEPS)[:, None]
    g = np.where(kind[None, :] == 1, np.abs(g) * alt, g)
    g = np.where(kind[None, :] == 2, g * rng.choice([-1.0, 1.0], (STEPS, N)), g)
    g[:, rng.uniform(size=N) < 1 / 16] = 0.0
    g[rng.uniform(size=(STEPS, N)) < 0.02] = 0.0
    mask = rng.uniform(size=N) < 0.9
    return theta, g.astype(np.float32), mask


def _ratios(opt, fault=None):
    """Per step: |fp32 - reference| / tolerance over the masked-in elements."""
    theta, g, mask = _problem()
    state = R.adam_state(mask)
    m = v = np.zeros(N, np.float32)
    out = []
    for t in range(1, STEPS + 1):
        nxt, m, v = R.adam_kernel_f32(theta, g[t - 1], m, v, t, opt, fault=fault)
        ref, state = R.adam_reference(theta, g[t - 1], state, t, opt)
        tol = R.adam_tolerance(ref, theta, g[t - 1], state, t, opt)
        assert np.all(ref[~mask] == theta[~mask]) and np.all(tol[mask] > 0)
        out.append(np.abs(nxt.astype(np.float64) - ref)[mask] / tol[mask])
        theta = nxt
    return out


@pytest.mark.parametrize("nesterov", [True, False])
def test_fp32_update_within_tolerance(nesterov):
    ratios = _ratios(R.Opt(nesterov=nesterov))
    worst = [float(r.max()) for r in ratios]
    print("worst error / tolerance per step:", [f"{w:.3f}" for w in worst])
    assert max(worst) <= 1.0, worst
    # the bound is not slack by orders of magnitude either
    assert max(worst) > 0.02, worst


# the nesterov term only exists with nesterov=True
@pytest.mark.parametrize("fault,nesterov", [(f, n) for f in R.FAULTS for n in (True, False)
                                            if n or f != "nesterov_b1t"])
def test_faulty_update_exceeds_tolerance(fault, nesterov):
    ratios = _ratios(R.Opt(nesterov=nesterov), fault=fault)
    share = [float((r > 1.0).mean()) for r in ratios]
    print(f"{fault}: share of elements over the tolerance per step:", [f"{s:.3f}" for s in share])
    assert min(share[1:]) >= 0.01, share  # from step 2 on (at t = 1, m_0 = 0 hides a lost m)


def test_reference_matches_direct_formula():
    """Two steps of adam_reference against the update written out by hand."""
    opt = R.Opt(nesterov=True)
    th0, g1, g2 = np.array([0.5, -2.0]), np.array([0.1, -3.0]), np.array([-0.2, 1.0])
    st = R.adam_state(np.ones(2, bool))
    th1, st = R.adam_reference(th0, g1, st, 1, opt)
    th2, st = R.adam_reference(th1, g2, st, 2, opt)
    b1, b2, lr, wd, eps = opt.b1, opt.b2, opt.learning_rate, opt.weight_decay, opt.eps
    m1, v1 = (1 - b1) * g1, (1 - b2) * g1**2
    mh = b1 * m1 / (1 - b1**2) + (1 - b1) * g1 / (1 - b1)
    e1 = th0 - lr * (mh / (np.sqrt(v1 / (1 - b2)) + eps) + wd * th0)
    m2, v2 = b1 * m1 + (1 - b1) * g2, b2 * v1 + (1 - b2) * g2**2
    mh = b1 * m2 / (1 - b1**3) + (1 - b1) * g2 / (1 - b1**2)
    e2 = e1 - lr * (mh / (np.sqrt(v2 / (1 - b2**2)) + eps) + wd * e1)
    np.testing.assert_allclose(th1, e1, rtol=1e-15)
    np.testing.assert_allclose(th2, e2, rtol=1e-15)
    np.testing.assert_allclose(st["A"], b1 * (1 - b1) * np.abs(g1) + (1 - b1) * np.abs(g2), rtol=1e-15)


def test_trajectory_batches_and_reset():
    from tests.flowcases import make_case

    b = R.trajectory_batches()
    assert len(b) == R.TRAJ_STEPS and {hi - lo for lo, hi in b} == {128, 99}
    assert all(0 <= lo < hi <= R.TRAJ_ROWS for lo, hi in b) and len({lo for lo, _ in b}) == len(b)
    case = make_case("bounded", N=64, seed=1)
    v = R.reset_shift_bounds(case["variables"])
    sb = v["batch_stats"]["bijector"]["bijectors_0"]
    assert sorted(sb) == ["xmax_0", "xmax_1", "xmin_0", "xmin_1"]
    assert all(np.all(sb[k] == (np.inf if "min" in k else -np.inf)) for k in sb)
    assert np.isfinite(case["variables"]["batch_stats"]["bijector"]["bijectors_0"]["xmin_0"]).all()
