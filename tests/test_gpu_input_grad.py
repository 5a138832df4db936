"""Gradients of log_prob with respect to the samples and the conditions
(the reference's Flow is a differentiable JAX function, flow.py:22-48;
examples/deep_set.ipynb's DeepSetFlow / loss_fn_2 cells train phi through
c = phi(x) with jax.grad).

* eval mode: ``log_prob_and_grad`` = (log_prob, cot . d lp / d x, cot . d lp / d c)
  vs float64 autograd of the restated flow (tests/input_grad_oracle.py);
* train mode: ``Trainer.loss_grad / step(cond_grad=True)``'s d loss / d c vs
  float64 autograd of the train-mode loss (train.py:64-72), with loss,
  gradient and stepped parameters bit-identical to the calls without it.

The tolerance is tests/test_gpu_train.py::test_train_gradient_per_parameter's,
per output column: |g_gpu - g64| <= 1e-5 max|g64| + 2 max(|g32 - g64|,
|g64' - g64|), maxima over the column's usable rows, g32 the float32
autograd over three row orders and g64' the float64 gradient at inputs and
parameters jittered by 2^-22 relative.  Rows whose float64 log_prob is not
finite must be exactly zero on the GPU (the `where` gradient of flow.py:47's
nan_to_num).  Rows with a finite log_prob whose autograd gradient is NaN, or
that a float32 or jittered evaluation loses, are left out of the comparison
(at most 2% of a case, tests/test_input_grad_oracle.py holds the float64
share to 1%); the GPU gradient there must still be finite."""

import functools
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

from tests.flowcases import bounded_case as _bounded_case
from tests.flowcases import _blob, _trainer, build_flow, make_case
from tests.input_grad_oracle import pack_job

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
F32 = np.float32


def run_oracle(model, variables, x, c=None, mode="eval", **extra):
    """The oracle's .npz for one job (a CPU-only child process)."""
    with tempfile.TemporaryDirectory() as d:
        job, out = Path(d) / "job.npz", Path(d) / "out.npz"
        pack_job(job, model, variables, x, c, mode=mode, **extra)
        subprocess.run([sys.executable, "-m", "tests.input_grad_oracle", str(job), str(out)], cwd=ROOT, check=True,
                       timeout=600)
        return dict(np.load(out))


@functools.lru_cache(maxsize=None)
def case_oracle(name, N, seed, mode="eval", stride=1):
    """(case, oracle results) of a tests/flowcases case, computed once per session."""
    case = make_case(name, N=N, seed=seed)
    extra = {"rows": np.arange(0, N, stride)} if stride > 1 else {}
    return case, run_oracle(case["model"], case["variables"], case["x"], case["c"], mode=mode, **extra)


def check_columns(tag, key, got, ref, record=None, zero_rows=True):
    """The module docstring's rule for one output (``gx``, ``gc``, ``gk``) over its columns."""
    g64 = ref[key + "64"]
    got = np.asarray(got, np.float64).reshape(g64.shape)
    others = [ref[f"{key}32_{r}"] for r in range(3)] + [ref[f"{key}64p_{r}"] for r in range(2)]
    if g64.ndim == 1:
        g64, got, others = g64[:, None], got[:, None], [o[:, None] for o in others]
    # rows whose log_prob is not finite: zero on the GPU (the interface's rule)
    bad = ~np.isfinite(ref["lp64"]) if "lp64" in ref else np.zeros(g64.shape[0], bool)
    # rows autograd itself loses: a finite log_prob whose gradient is NaN (a
    # sample clipped onto the spline's end runs the interior formula on the
    # fill-mode NaN knots in the unselected `where` branch, and 0 * NaN
    # reaches x), or a float32 / jittered evaluation that is not finite
    lost = ~np.isfinite(g64).all(axis=1)
    for k in ("gx64", "gc64"):
        if k in ref and "lp64" in ref:
            lost |= ~np.isfinite(ref[k]).all(axis=1)
    for o in others:
        lost |= ~np.isfinite(o).all(axis=1)
    use = ~bad & ~lost
    assert use.mean() >= 0.98, f"{tag}: only {use.sum()} of {use.size} rows usable"
    if zero_rows and bad.any():
        assert np.all(got[bad] == 0), f"{tag}/{key}: non-finite rows must have zero gradient"
    assert np.isfinite(got[~bad]).all(), f"{tag}/{key}: non-finite gradient on a row with a finite log_prob"
    worst = 0.0
    over = []
    for j in range(g64.shape[1]):
        r = g64[use, j]
        scale = max(np.abs(r).max(), 1e-30)
        e32 = max(np.abs(o[use, j] - r).max() for o in others[:3])
        cond = max(np.abs(o[use, j] - r).max() for o in others[3:])
        e = np.abs(got[use, j] - r)
        worst = max(worst, float(e.max() / scale))
        print(f"{tag}/{key}[{j}]: gpu {e.max() / scale:.3g} fp32 autograd {e32 / scale:.3g} conditioning "
              f"{cond / scale:.3g} (of max |g64| {scale:.3g})")
        if not (e <= 1e-5 * scale + 2 * max(e32, cond)).all():
            over.append(f"{key}[{j}]: max rel {e.max() / scale:.3g} (fp32 autograd {e32 / scale:.3g}, "
                        f"conditioning {cond / scale:.3g})")
    if record is not None:
        record[f"{key}_max_rel_err_vs_fp64"] = worst
        record.setdefault("over", []).extend(over)
    assert not over, f"{tag}: {over}"
    return use, bad


def _record(rec):
    from tests.test_gpu_flow import _append_record

    _append_record("grad_parity.jsonl", rec)


def gpu_vjp(case, cot=None, **kw):
    flow = build_flow(case["cfg"])
    return flow.apply(case["variables"], case["x"], case["c"], method="log_prob_and_grad", cotangent=cot, **kw)


def check_eval(tag, case, ref, lp, dx, dc, rows=None):
    from tests.test_gpu_flow import check_lp

    N, D, C = case["x"].shape[0], case["cfg"]["D"], case["cfg"]["C"]
    assert lp.shape == (N,) and lp.dtype == F32 and dx.shape == (N, D) and dx.dtype == F32
    check_lp(lp, case, tag)
    sel = slice(None) if rows is None else rows
    rec = {"case": tag, "rows": N, "what": "input gradient (eval)"}
    try:
        check_columns(tag, "gx", dx[sel], ref, rec)
        if C:
            assert dc.shape == (N, C) and dc.dtype == F32
            check_columns(tag, "gc", dc[sel], ref, rec)
        else:
            assert dc is None
    finally:
        _record(rec)


EVAL_CASES = [("small", 256, 1), ("cfg2", 256, 2), ("cfg4", 256, 3), ("odd", 300, 4), ("deep", 256, 5),
              ("uniform", 256, 6), ("d7k32c2", 256, 7), ("gelu", 256, 8), ("mixed", 256, 9), ("h384c2", 256, 10)]


@pytest.mark.parametrize("name,N,seed", EVAL_CASES)
def test_eval_vjp_parity(name, N, seed):
    case, ref = case_oracle(name, N, seed)
    check_eval(f"{name}/N={N}", case, ref, *gpu_vjp(case))


def test_bounded_shift_bounds():
    case = _bounded_case()
    ref = run_oracle(case["model"], case["variables"], case["x"], case["c"])
    lp, dx, dc = gpu_vjp(case)
    check_eval("bounded", case, ref, lp, dx, dc)
    # a clipped one-sided dim passes nothing through z: only log_det's -t term, -dt/dx, is left
    st = case["variables"]["batch_stats"]["bijector"]["bijectors_0"]
    x = case["x"].astype(np.float64)
    fin = np.isfinite(ref["lp64"])
    clipped = 0
    for i, t, dtdx in ((0, np.log(x[:, 0]), 1 / x[:, 0]), (1, np.log(2 - x[:, 1]), -1 / (2 - x[:, 1]))):
        lo, hi = float(st[f"xmin_{i}"].reshape(-1)[0]), float(st[f"xmax_{i}"].reshape(-1)[0])
        m = ((t < lo - 1e-3) | (t > hi + 1e-3)) & fin
        clipped += m.sum()
        np.testing.assert_allclose(dx[m, i], -dtdx[m], rtol=1e-6)
    assert clipped > 0, "no row clips: the case does not cover the clamp"


def test_cotangent():
    case = make_case("cfg4", N=300, seed=3)
    cot = np.random.default_rng(31).uniform(-2, 2, 300).astype(F32)
    ref = run_oracle(case["model"], case["variables"], case["x"], case["c"], cot=cot)
    lp, dx, dc = gpu_vjp(case, cot)
    check_eval("cfg4/cot", case, ref, lp, dx, dc)
    lp1, _, _ = gpu_vjp(case)
    assert np.array_equal(lp, lp1)  # log_prob does not depend on the cotangent


def test_non_finite_rows():
    case = make_case("cfg4", N=256, seed=3)
    rows = [5, 100, 255]
    case["x"] = case["x"].copy()
    case["x"][rows] = 100.0
    ref = run_oracle(case["model"], case["variables"], case["x"], case["c"])
    assert not np.isfinite(ref["lp64"][rows]).any()
    lp, dx, dc = gpu_vjp(case)
    assert np.all(lp[rows] == np.finfo(F32).min)
    assert np.all(dx[rows] == 0) and np.all(dc[rows] == 0)
    check_eval("cfg4/nonfinite", case, ref, lp, dx, dc)


def test_row_independence_and_chunking():
    case, ref = case_oracle("odd", 300, 4)
    lp, dx, dc = gpu_vjp(case)
    p = np.random.default_rng(41).permutation(300)
    pc = dict(case, x=case["x"][p], c=case["c"][p])
    lpp, dxp, dcp = gpu_vjp(pc)
    inv = np.argsort(p)
    assert np.array_equal(lpp[inv], lp) and np.array_equal(dxp[inv], dx) and np.array_equal(dcp[inv], dc)
    lpk, dxk, dck = gpu_vjp(case, chunk_rows=128)
    assert np.abs(dxk - dx).max() <= 1e-6 * np.abs(dx).max()
    assert np.abs(dck - dc).max() <= 1e-6 * np.abs(dc).max()
    assert np.abs(lpk - lp).max() <= 1e-6 * np.abs(lp).max()
    one = dict(case, x=case["x"][:1], c=case["c"][:1])
    lp1, dx1, dc1 = gpu_vjp(one)
    assert lp1.shape == (1,) and dx1.shape == (1, 5) and dc1.shape == (1, 3)
    assert np.abs(dx1 - dx[:1]).max() <= 1e-6 * np.abs(dx).max()


def test_large_batch():
    """65536 rows: the forward GEMMs run the split-MFMA kernel; the oracle takes every 16th row."""
    case, ref = case_oracle("cfg2", 65536, 11, "eval", 16)
    lp, dx, dc = gpu_vjp(case)
    N = 65536
    assert lp.shape == (N,) and dx.shape == (N, 4) and dc is None
    rows = np.arange(0, N, 16)
    sub = dict(case, x=case["x"][rows])
    from tests.test_gpu_flow import check_lp

    check_lp(lp[rows], sub, "cfg2/N=65536")
    rec = {"case": "cfg2/N=65536", "rows": N, "what": "input gradient (eval), every 16th row"}
    try:
        check_columns("cfg2/N=65536", "gx", dx[rows], ref, rec)
    finally:
        _record(rec)


# ---- train mode: d loss / d c ----------------------------------------------------
@pytest.mark.parametrize("bn_small", ["1", "0"])
@pytest.mark.parametrize("name,N,seed", [("cfg4", 128, 12), ("odd", 300, 13), ("deep", 256, 14)])
def test_train_gc(name, N, seed, bn_small, monkeypatch):
    monkeypatch.setenv("ZF_TRAIN_BN_SMALL", bn_small)
    case, ref = case_oracle(name, N, seed, "train")
    x, c = case["x"], case["c"]
    tr = _trainer(case, N)
    loss0, g0 = tr.loss_grad(x, c)
    loss, g, gc = tr.loss_grad(x, c, cond_grad=True)
    assert loss == loss0 and np.array_equal(g, g0)
    assert gc.shape == c.shape and gc.dtype == F32
    assert loss == pytest.approx(float(ref["loss64"]), rel=2e-5, abs=2e-5)
    rec = {"case": f"{name}/bn_small={bn_small}", "rows": N, "what": "d loss / d c (train)"}
    try:
        check_columns(f"{name}/train", "gc", gc, ref, rec)
    finally:
        _record(rec)
    plain, cond = _trainer(case, N), _trainer(case, N)
    for _ in range(3):
        plain.step(x, c)
        gcs = cond.step(x, c, cond_grad=True)
    assert gcs.shape == c.shape and np.isfinite(gcs).all()
    assert plain.last_loss() == cond.last_loss()
    assert np.array_equal(_blob(plain), _blob(cond), equal_nan=True)


def test_deep_set_chain_rule():
    """c = phi(xin) = tanh(xin @ kernel + bias) (tests/flowcases.make_deep_set_module's phi):
    d loss / d phi's weights from the GPU's gc by the chain rule on the host
    vs autograd of the composite; then thirty joint steps lower the loss."""
    N = 256
    rng = np.random.default_rng(51)
    case = make_case("cfg4", N=N, seed=15)
    xin = rng.standard_normal((N, 3)).astype(F32)
    kern = (0.5 * rng.standard_normal((3, 2))).astype(F32)
    bias = np.zeros(2, F32)
    # y depends on xin, so that phi has something to learn
    y = (case["x"] + 0.8 * np.tanh(xin[:, :2])).astype(F32)
    ref = run_oracle(case["model"], case["variables"], y, None, mode="train", xin=xin, phi_kernel=kern,
                     phi_bias=bias)

    def phi(k, b):
        return np.tanh(xin @ k + b).astype(F32)

    tr = _trainer(case, N)
    c = phi(kern, bias)
    loss, _, gc = tr.loss_grad(y, c, cond_grad=True)
    assert loss == pytest.approx(float(ref["loss64"]), rel=2e-5, abs=2e-5)
    gpre = gc.astype(np.float64) * (1 - c.astype(np.float64) ** 2)
    gk, gb = xin.astype(np.float64).T @ gpre, gpre.sum(axis=0)
    rec = {"case": "cfg4/deep_set", "rows": N, "what": "d loss / d phi (train, chain rule from gc)"}
    try:
        check_columns("deep_set", "gk", gk, ref, rec, zero_rows=False)
        check_columns("deep_set", "gb", gb, ref, rec, zero_rows=False)
    finally:
        _record(rec)
    # joint training: the flow by its optimiser, phi by plain SGD on the chain rule
    losses = []
    k, b = kern.copy(), bias.copy()
    for _ in range(30):
        c = phi(k, b)
        gc = tr.step(y, c, cond_grad=True)
        losses.append(tr.last_loss())
        gpre = gc * (1 - c * c)
        k -= 0.05 * (xin.T @ gpre)
        b -= 0.05 * gpre.sum(axis=0)
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


def test_two_ranks_gc_matches_one_device(tmp_path):
    from zenflow_amd.launch import spawn

    name, N, seed = "cfg4", 2048, 16
    worker = str(Path(__file__).resolve().parent / "dist_worker_cond.py")
    env = dict(os.environ, ZF_TEST_CASE=f"{name}:{N}:{seed}", ZF_DEVICE="0")
    assert spawn(2, [worker, str(tmp_path)], env=env, timeout=240) == 0
    ranks = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]
    case = make_case(name, N=N, seed=seed)
    loss, g, gc = _trainer(case, N).loss_grad(case["x"], case["c"], cond_grad=True)
    assert [int(r["lo"]) for r in ranks] == [0, N // 2]
    both = np.concatenate([r["gc"] for r in ranks])
    assert np.array_equal(both, gc), f"{np.sum(both != gc)} of {gc.size} gc entries differ"
    for r in ranks:
        assert float(r["loss"]) == loss and np.array_equal(r["grad"], g)


# ---- through the API ---------------------------------------------------------------
def test_api():
    import zenflow_amd as zf
    from tests.flowcases import make_deep_set_module
    from zenflow_amd import _lib as L
    from zenflow_amd import bijectors as bi

    case = make_case("cfg4", N=200, seed=17)
    flow = build_flow(case["cfg"])
    lp, dx, dc = flow.apply(case["variables"], case["x"], case["c"], method="log_prob_and_grad")
    assert isinstance(lp, np.ndarray) and lp.shape == (200,) and dx.shape == (200, 2) and dc.shape == (200, 2)
    bf =flow.bind(case["variables"], 2, 2)
    xd, cd = L.DeviceArray.from_numpy(case["x"]), L.DeviceArray.from_numpy(case["c"])
    out = bf.log_prob_and_grad(xd, cd)
    assert all(isinstance(o, L.DeviceArray) for o in out)
    for a, b in zip(out, (lp, dx, dc)):
        assert np.array_equal(a.numpy(), b)
    dev = flow.apply(case["variables"], xd, cd, method="log_prob_and_grad")
    assert all(isinstance(o, L.DeviceArray) for o in dev) and np.array_equal(dev[1].numpy(), dx)
    # the handle is kept on the cached program, and re-created when chunk_rows grows
    h = bf.program._vjp
    bf.log_prob_and_grad(xd, cd, chunk_rows=64)
    assert bf.program._vjp is h
    big = make_case("cfg4", N=512, seed=17)
    flow.apply(case["variables"], big["x"], big["c"], method="log_prob_and_grad")
    assert bf.program._vjp is not h and bf.program._vjp.batch_max == 512

    # a user module holding the flow (the deep-set layout)
    Base = make_deep_set_module()

    class DeepSetScore(Base):
        def score(self, x, y):
            return self.flow.log_prob_and_grad(y, self.phi(x))

    m = DeepSetScore(bi.rolling_spline_coupling(2, layers=(64,) * 3))
    rng = np.random.default_rng(5)
    x = rng.standard_normal((100, 3)).astype(F32)
    y = (0.5 + 0.1 * rng.standard_normal((100, 2))).astype(F32)
    v = m.init(zf.PRNGKey(0), x, y)
    _, upd = m.apply(v, x, y, train=True, mutable=["batch_stats"])
    v = {"params": v["params"], "batch_stats": upd["batch_stats"]}
    nlp, ndx, ndc = m.apply(v, x, y, method="score")
    assert nlp.shape == (100,) and ndx.shape == (100, 2) and ndc.shape == (100, 2)
    c = m.apply(v, x, method=lambda mod, x: mod.phi(x))
    sub = {"params": v["params"]["flow"], "batch_stats": v["batch_stats"]["flow"]}
    top = zf.Flow(m.bijectors).apply(sub, y, c, method="log_prob_and_grad")
    for a, b in zip((nlp, ndx, ndc), top):
        assert np.array_equal(a, b, equal_nan=True)

    # unconditional: dc is None
    un = make_case("cfg2", N=64, seed=18)
    ulp, udx, udc = gpu_vjp(un)
    assert udc is None and udx.shape == (64, 4)

    # past the trainer's limits: an error that names the limit, no fallback
    k100 = make_case("k100", N=8, seed=19)
    with pytest.raises(NotImplementedError, match="knots"):
        gpu_vjp(k100)
