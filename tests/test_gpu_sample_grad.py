"""Gradients through sampling on the GPU: ``Trainer.sample_forward`` (the
samples x = bijector.inverse(z, c) and their log-density log_q) and
``sample_backward(gx, glog_q)`` (the gradient of ``sum(gx . x + glog_q log_q)``
with respect to the parameters, z and c).

With the reference ``flow.apply(vars, c_or_n, method="sample")`` (flow.py:50-78)
is a differentiable JAX function; here the user's ``d loss / d x`` and
``d loss / d log_q`` go into the device trainer's reverse of the inverse pass.
The float64 reference is tests/sample_grad_oracle.py, with z drawn from the
case's latent and standard-normal cotangents.

The parameter-gradient criterion is ``tests.test_gpu_custom_loss.check_params``,
the d / d z and d / d c criterion ``tests.test_gpu_input_grad.check_columns``:
|g - g64| <= 1e-5 max|g64| + 2 max(|g32 - g64|, |g64' - g64|), at most 2% of
rows left out."""

import functools
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest
from numpy.testing import assert_allclose

from tests.flowcases import _blob, _trainer, build_flow, make_case
from tests.sample_grad_oracle import make_inputs

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
WORKER = str(Path(__file__).resolve().parent / "dist_worker_sample.py")
F32 = np.float32

# cfg2: compiled K = 16; cfg4: conditional, Beta; odd: runtime K = 7, three layers,
# truncated normal, C = 3; k64c1: the K limit; gelu; bounded: one-sided ShiftBounds
# (the exp forms); cfg4 at 3 rows and small at 65: a partial last block, rpb not
# dividing the rows
CASES = [("cfg2", 256, 2), ("cfg4", 256, 3), ("odd", 256, 4), ("k64c1", 256, 5), ("gelu", 256, 8),
         ("bounded", 256, 21), ("cfg4", 3, 88), ("small", 65, 1)]


@functools.lru_cache(maxsize=None)
def oracle(name, N, seed, mode):
    """The oracle's .npz of one case (a CPU-only child process), once per session."""
    with tempfile.TemporaryDirectory() as d:
        out = Path(d) / "o.npz"
        subprocess.run([sys.executable, "-m", "tests.sample_grad_oracle", name, str(N), str(seed), mode, str(out)],
                       cwd=ROOT, check=True, timeout=600)
        return dict(np.load(out))


def _record(rec):
    from tests.test_gpu_flow import _append_record

    _append_record("grad_parity.jsonl", rec)


def _cond(case, n=None):
    """``sample_forward``'s first argument: the conditions, or the row count."""
    return case["c"] if case["cfg"]["C"] else (case["x"].shape[0] if n is None else n)


def _run(case, z, gx, glq, N=None, **kw):
    tr = _trainer(case, z.shape[0] if N is None else N)
    x, lq = tr.sample_forward(_cond(case, z.shape[0]), z=z)
    out = tr.sample_backward(gx, glq, **kw)
    return tr, x, lq, out


# ---- 1. the parameter gradient, gz, gc ---------------------------------------------
@pytest.mark.parametrize("mode", ["glq", "noglq"])
@pytest.mark.parametrize("name,N,seed", CASES)
def test_sample_gradient_per_parameter(name, N, seed, mode):
    """sample_forward + sample_backward with standard-normal cotangents (glog_q
    standard normal or None): every parameter tensor by ``check_params``, the
    statistics entries exactly 0, d / d z and d / d c by ``check_columns``."""
    from tests.test_gpu_custom_loss import check_params
    from tests.test_gpu_input_grad import check_columns

    case = make_case(name, N=N, seed=seed)
    ref = oracle(name, N, seed, mode)
    assert ref["dropped"].mean() <= 0.02
    C = case["cfg"]["C"]
    z = ref["z"].astype(F32)
    gx = ref["cgx"].astype(F32)
    gx[ref["dropped"]] = 0.0
    glq = None
    if mode == "glq":
        glq = ref["cglq"].astype(F32)
        glq[ref["dropped"]] = 0.0
    tr, x, lq, out = _run(case, z, gx, glq, cond_grad=C > 0, latent_grad=True)
    g, gz = out[0], out[-1]
    assert x.shape == (N, case["cfg"]["D"]) and x.dtype == F32 and lq.shape == (N,) and lq.dtype == F32
    assert g.shape == tr.program.blob.shape and g.dtype == F32
    assert np.all(g[tr.program.param_mask == 0] == 0), "statistics entries of the gradient must be exactly 0"
    tag = f"{name}/N={N}/sample/{mode}"
    check_params(tag, tr.grad_tree(g), ref, N, f"sample parameter gradient ({mode})")
    rec = {"case": tag, "rows": N, "what": f"sample d / d z, d / d c ({mode})"}
    try:
        assert gz.shape == z.shape and gz.dtype == F32
        check_columns(tag, "gz", gz, ref, rec)
        if C:
            gc = out[1]
            assert gc.shape == case["c"].shape and gc.dtype == F32
            check_columns(tag, "gc", gc, ref, rec)
    finally:
        _record(rec)


# ---- 2. values ---------------------------------------------------------------------------
def _inverse_parity(x, ref):
    """tests/test_gpu_flow.py::test_inverse_parity's rule."""
    from tests.test_gpu_flow import REL

    fin = np.isfinite(ref)
    assert np.mean(fin != np.isfinite(x)) <= 1e-3
    both = fin & np.isfinite(x)
    assert_allclose(x[both], ref[both], rtol=REL, atol=REL * np.abs(ref[both]).max())


@pytest.mark.parametrize("name,N,seed", [c for c in CASES if c[1] > 3])
def test_values(name, N, seed):
    """x against ``O.flow_inverse`` by the inverse-parity rule; log_q against
    the float64 oracle's by REL on the rows finite in both.

    k64c1 apart: at 64 knots a bin is 1/64 wide, half an ulp of z moves log_q
    by 6e-6, and the float32 evaluation of the restated reference itself is
    1.7e-5 off float64 there (the GPU: 2.1e-5), so plain REL is not a bound a
    float32 log_q can hold at the knot limit.  That case is held to
    ``check_columns``' rule instead, REL max(1, |lq64|) + 2 max(|lq32 - lq64|,
    |lq64' - lq64|) per row."""
    from oracle import zf_oracle as O
    from tests.test_gpu_flow import REL

    case = make_case(name, N=N, seed=seed)
    ref = oracle(name, N, seed, "glq")
    z = ref["z"].astype(F32)
    tr = _trainer(case, N)
    x, lq = tr.sample_forward(_cond(case), z=z)
    _inverse_parity(x, O.flow_inverse(case["model"], case["variables"], z, case["c"]))
    lq64 = ref["lq64"]
    both = np.isfinite(lq64) & np.isfinite(lq)
    assert both.mean() >= 0.98
    scale = np.maximum(1.0, np.abs(lq64[both]))
    e = np.abs(lq[both].astype(np.float64) - lq64[both])
    e32 = np.max([np.abs(ref[f"lq32_{r}"] - lq64)[both] for r in range(3)], axis=0)
    cond = np.max([np.abs(ref[f"lq64p_{r}"] - lq64)[both] for r in range(2)], axis=0)
    print(f"{name}/N={N}: log_q max rel err {(e / scale).max():.3g} on {both.sum()} of {N} rows "
          f"(fp32 restatement {(e32 / scale).max():.3g}, conditioning {(cond / scale).max():.3g})")
    if name == "k64c1":
        assert np.isfinite(e32).all() and np.isfinite(cond).all()
        assert (e <= REL * scale + 2 * np.maximum(e32, cond)).all()
    else:
        assert (e / scale).max() <= REL


@pytest.mark.parametrize("name,N,seed", [("cfg2", 300, 2), ("cfg4", 300, 3)])
def test_seeded_draw(name, N, seed):
    """``sample_forward(n, seed=s)`` has the bits of ``sample_forward(z=flow.latent.sample(n,
    PRNGKey(s)))``, and its x agrees with ``Flow.sample(n, seed=s)`` (another
    kernel: the inverse-parity rule, not bits)."""
    from zenflow_amd._lib import DeviceArray
    from zenflow_amd.random import PRNGKey

    case = make_case(name, N=N, seed=seed)
    tr = _trainer(case, N)
    first = _cond(case)
    x, lq = tr.sample_forward(first, seed=7)
    z = tr.flow.latent.sample(N, PRNGKey(7))
    assert z.shape == (N, case["cfg"]["D"])
    x2, lq2 = tr.sample_forward(first, z=z)
    assert np.array_equal(x.view(np.uint32), x2.view(np.uint32))
    assert np.array_equal(lq.view(np.uint32), lq2.view(np.uint32))
    xs = build_flow(case["cfg"])
    xs.latent._dim = case["cfg"]["D"]
    _inverse_parity(x, xs.apply(case["variables"], first, seed=7, method="sample"))
    # device in, device out
    xd, lqd = tr.sample_forward(first, z=DeviceArray.from_numpy(z))
    assert isinstance(xd, DeviceArray) and isinstance(lqd, DeviceArray)
    assert np.array_equal(xd.numpy().view(np.uint32), x.view(np.uint32))
    g = tr.sample_backward(DeviceArray.from_numpy(np.ones_like(z)))
    assert isinstance(g, DeviceArray) and np.isfinite(g.numpy()).all()


# ---- 3. masking ------------------------------------------------------------------------------
def test_identity_columns():
    """cfg2 (a Normal latent: its support is the line).  Rows with one z
    column outside [0, 1): that column is the identity in every coupling, the
    gradient stays finite.  Rows with every column outside: every spline is
    the identity, so no conditioner takes part and the cotangent passes
    through the couplings unchanged — gz is gx through ShiftBounds.inverse
    alone, gx (xmax - xmin), to the bit."""
    name, N, seed = "cfg2", 256, 2
    case = make_case(name, N=N, seed=seed)
    z, gx, _ = make_inputs(case, N, seed)
    rows, cols = np.array([3, 77, 130, 255]), np.array([0, 1, 2, 3])
    z[rows, cols] = np.array([-0.25, 1.0, 1.5, -1e-3], F32)
    allout = [10, 200]
    z[allout] = np.array([[-0.25, 1.0, 1.5, -1e-3], [1.0, 2.0, -3.0, 1.0 + 2.0**-20]], F32)
    tr, x, lq, (g, gz) = _run(case, z, gx, None, latent_grad=True)
    assert np.isfinite(x).all() and np.isfinite(lq).all()
    assert np.isfinite(g).all() and np.abs(g).max() > 0 and np.isfinite(gz).all()
    st = case["variables"]["batch_stats"]["bijector"]["bijectors_0"]
    w = np.array([F32(st[f"xmax_{i}"].reshape(-1)[0]) - F32(st[f"xmin_{i}"].reshape(-1)[0]) for i in range(4)], F32)
    # Roll.inverse, D - 1 times: x[:, i] is z[:, (i + D - 1) % D]
    assert np.array_equal(gz[allout], np.roll(gx[allout] * w, 3, axis=1))
    # without those rows' cotangents the parameter gradient is the same: they carry none
    gx0 = gx.copy()
    gx0[allout] = 0.0
    _, _, _, (g0, _) = _run(case, z, gx0, None, latent_grad=True)
    assert np.array_equal(g.view(np.uint32), g0.view(np.uint32))


def test_rows_outside_the_latents_support():
    """cfg4 (Beta latent): rows with a latent value outside [0, 1] have a
    log_q that is not finite, all-zero gz / gc rows, and the gradient has the
    bits of the run with those rows' cotangents at zero."""
    name, N, seed = "cfg4", 256, 3
    case = make_case(name, N=N, seed=seed)
    z, gx, glq = make_inputs(case, N, seed)
    rows = [5, 100, 255]
    z[rows, 0] = np.array([1.25, -0.5, 1.0 + 2.0**-20], F32)
    tr, x, lq, (g, gc, gz) = _run(case, z, gx, glq, cond_grad=True, latent_grad=True)
    keep = np.ones(N, bool)
    keep[rows] = False
    assert not np.isfinite(lq[rows]).any() and np.isfinite(lq[keep]).all()
    assert np.isfinite(x).all()
    assert np.all(gz[rows] == 0) and np.all(gc[rows] == 0)
    assert np.abs(gz[keep]).max() > 0 and np.abs(gc[keep]).max() > 0
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    gx0, glq0 = gx.copy(), glq.copy()
    gx0[rows] = 0.0
    glq0[rows] = 0.0
    _, _, _, (g0, gc0, gz0) = _run(case, z, gx0, glq0, cond_grad=True, latent_grad=True)
    for u, v in ((g, g0), (gc, gc0), (gz, gz0)):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))


# ---- 4. the state machine --------------------------------------------------------------------
def test_state_machine():
    from zenflow_amd import _lib as L
    from zenflow_amd._lib import DeviceArray

    N = 128
    case = make_case("cfg4", N=N, seed=3)
    x, c = case["x"], case["c"]
    z, gx, glq = make_inputs(case, N, 3)
    tr = _trainer(case, N)
    with pytest.raises(ValueError, match="pending sample_forward"):
        tr.sample_backward(gx)
    tr.sample_forward(c, z=z)
    g = tr.sample_backward(gx, glq)
    with pytest.raises(ValueError, match="pending sample_forward"):  # one backward per forward
        tr.sample_backward(gx)
    xd, cd = DeviceArray.from_numpy(x), DeviceArray.from_numpy(c)
    for between in (lambda: tr.step(x, c), lambda: tr.loss_grad(x, c), lambda: tr.log_prob_vjp(xd, cd),
                    lambda: tr.apply_gradient(g), lambda: tr.forward(x, c)):
        tr.sample_forward(c, z=z)
        between()
        with pytest.raises(ValueError, match="pending sample_forward"):
            tr.sample_backward(gx)
    # a sampling pass is not a forward, and a forward is not a sampling pass
    tr.sample_forward(c, z=z)
    with pytest.raises(ValueError, match="pending forward"):
        tr.backward(np.ones(N, F32))
    lib = L.load_library()
    cot = DeviceArray.from_numpy(np.ones(N, F32))
    gxd = DeviceArray.from_numpy(gx)
    assert lib.zf_trainer_backward(tr.handle, cot.ptr, None, None, L.stream()) == -1
    assert "no forward pending" in lib.zf_last_error().decode()
    tr.sample_backward(gx)  # the refused call enqueued nothing and left the pass pending
    tr.forward(x, c, train=False)
    assert lib.zf_trainer_sample_backward(tr.handle, gxd.ptr, None, None, None, None, L.stream()) == -1
    assert "no forward pending" in lib.zf_last_error().decode()
    tr.backward(np.ones(N, F32))
    assert lib.zf_trainer_sample_backward(tr.handle, gxd.ptr, None, None, None, None, L.stream()) == -1
    # argument checks, before any device call
    with pytest.raises(ValueError, match="batch_max"):
        _trainer(case, 64).sample_forward(c, z=z)
    with pytest.raises(ValueError, match="conditional"):
        tr.sample_forward(N, z=z)
    with pytest.raises(ValueError, match="z must hold"):
        tr.sample_forward(c, z=z[:, :1])
    tr.sample_forward(c, z=z)
    with pytest.raises(ValueError, match="shape"):
        tr.sample_backward(gx[:-1])
    bad = gx.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        tr.sample_backward(bad)
    with pytest.raises(ValueError, match="non-finite"):
        tr.sample_backward(gx, np.full(N, np.inf, F32))
    tr.sample_backward(gx, glq)  # the refused calls left the pass pending
    # ShiftBounds' stored bounds still at the initial +-inf
    fresh = dict(case, variables={"params": case["variables"]["params"], "batch_stats": {"bijector": dict(
        case["variables"]["batch_stats"]["bijector"],
        bijectors_0={k: np.full_like(v, np.inf if k.startswith("xmin") else -np.inf)
                     for k, v in case["variables"]["batch_stats"]["bijector"]["bijectors_0"].items()})}})
    tf = _trainer(fresh, N)
    with pytest.raises(ValueError, match="initial"):
        tf.sample_forward(c, z=z)
    tf.step(x, c)  # a train-mode pass sets them
    xs, _ = tf.sample_forward(c, z=z)
    assert np.isfinite(xs).all()
    # and the trainer still steps
    before = _blob(tr)
    tr.step(x, c)
    assert np.isfinite(tr.last_loss()) and not np.array_equal(_blob(tr), before)


# ---- 5. linearity, accumulation, determinism -----------------------------------------------
def test_accumulation_and_determinism():
    """cfg4, 256 rows: the gradient of the whole batch against the sum of two
    128-row halves with ``global_rows=256`` (1e-6 max|g|, the bound
    tests/test_gpu_input_grad.py holds chunked against whole to); the same
    call twice gives the same bits."""
    name, N, seed = "cfg4", 256, 3
    case = make_case(name, N=N, seed=seed)
    z, gx, glq = make_inputs(case, N, seed)
    outs = []
    for _ in range(2):
        _, x, lq, (g, gc, gz) = _run(case, z, gx, glq, cond_grad=True, latent_grad=True)
        outs.append((x, lq, g, gc, gz))
    for u, v in zip(*outs):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    g = outs[0][2]
    tr = _trainer(case, 128)
    parts = []
    for lo in (0, 128):
        tr.sample_forward(case["c"][lo:lo + 128], z=z[lo:lo + 128], global_rows=N)
        parts.append(tr.sample_backward(gx[lo:lo + 128], glq[lo:lo + 128]))
    err = np.abs(parts[0].astype(np.float64) + parts[1] - g).max()
    print(f"halves vs whole: {err / np.abs(g).max():.3g} of max|g|")
    assert err <= 1e-6 * np.abs(g).max()
    before = _blob(tr)
    tr.apply_gradient(parts[0] + parts[1])
    assert not np.array_equal(_blob(tr), before) and tr.opt_state()["count"] == 1


# ---- 6. two ranks -------------------------------------------------------------------------------
def test_two_ranks_match_one_device_bitwise(tmp_path):
    """cfg4, 128 rows as 2 x 64 (dist.HostAllgather): x and log_q
    (concatenated) and the gradient are one device's, bit for bit, on both
    ranks — the eval custom-loss path's property, which this reverse pass
    inherits (the same leaf trees over the global batch)."""
    from zenflow_amd.launch import spawn

    name, N, seed = "cfg4", 128, 3
    env = dict(os.environ, ZF_TEST_CASE=f"{name}:{N}:{seed}", ZF_DEVICE="0")
    assert spawn(2, [WORKER, str(tmp_path)], env=env, timeout=240) == 0
    ranks = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]
    case = make_case(name, N=N, seed=seed)
    z, gx, glq = make_inputs(case, N, seed)
    _, x, lq, g = _run(case, z, gx, glq)
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    assert np.array_equal(ranks[0]["grad"].view(np.uint32), ranks[1]["grad"].view(np.uint32))
    x2 = np.concatenate([ranks[0]["x"], ranks[1]["x"]])
    lq2 = np.concatenate([ranks[0]["lq"], ranks[1]["lq"]])
    assert np.array_equal(x2.view(np.uint32), x.view(np.uint32))
    assert np.array_equal(lq2.view(np.uint32), lq.view(np.uint32))
    for k, r in enumerate(ranks):
        assert np.array_equal(r["grad"].view(np.uint32), g.view(np.uint32)), \
            f"rank {k}: {np.sum(r['grad'] != g)} gradient entries differ"


# ---- 7. end to end: reverse KL ------------------------------------------------------------------
def test_reverse_kl_trains():
    """The ``uniform`` case (D = 2, K = 4, one hidden layer of 32; ShiftBounds
    on [0, 1]) fitted to a product of Beta(2, 5) densities by reverse KL,
    E_z[log q(x(z)) - log p(x(z))]: batch 512, 60 ``adam(1e-2)`` steps of
    sample_forward -> host loss -> sample_backward -> apply_gradient.  The KL
    estimate on one fixed held-out z batch is finite at every step and ends
    below its start (a sanity condition: the gradient tests carry the
    precision)."""
    from zenflow_amd import optim

    case = make_case("uniform", N=512, seed=6)
    st = case["variables"]["batch_stats"]["bijector"]["bijectors_0"]
    for k in st:
        st[k] = np.full_like(st[k], 0.0 if k.startswith("xmin") else 1.0)
    tr = _trainer(case, 512, optimizer=optim.adam(1e-2))
    zt = np.random.default_rng(99).uniform(size=(512, 2)).astype(F32)

    def log_p(x):
        return np.sum(np.log(30.0) + np.log(x) + 4.0 * np.log1p(-x), axis=1)

    def held_out():
        x, lq = tr.sample_forward(512, z=zt)
        ok = np.isfinite(lq) & np.isfinite(x).all(axis=1)
        assert ok.mean() >= 0.99
        x, lq = x[ok].astype(np.float64), lq[ok].astype(np.float64)
        return float(np.mean(lq - log_p(x)))

    kl = [held_out()]
    for step in range(60):
        x, lq = tr.sample_forward(512, seed=step)
        ok = np.isfinite(lq) & np.isfinite(x).all(axis=1)
        xs = np.where(ok[:, None], x, 0.5).astype(np.float64)
        gx = -(1.0 / xs - 4.0 / (1.0 - xs)) / 512
        gx[~ok] = 0.0
        tr.sample_backward(gx.astype(F32), np.full(512, 1.0 / 512, F32))
        tr.apply_gradient()
        kl.append(held_out())
    print(f"reverse KL, held out: start {kl[0]:.6g}, end {kl[-1]:.6g}, min {min(kl):.6g}")
    assert np.isfinite(kl).all()
    assert kl[-1] < kl[0]
