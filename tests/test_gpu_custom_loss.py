"""Custom losses on the GPU: ``Trainer.forward`` (per-row log_prob),
``backward(cotangent)`` (the parameter gradient of ``sum(cot * lp)``) and
``apply_gradient`` (the optimiser half of a step).

With the reference the loss is user code around ``flow.apply``
(train.py:64-86, flow.py:22-48) and ``jax.grad`` differentiates it; here the
user's ``d loss / d lp`` goes into the device trainer's reverse pass, in train
mode (batch statistics) and in eval mode (stored statistics).  The float64
reference is tests/custom_loss_oracle.py, with a standard-normal cotangent.

The parameter-gradient criterion is
tests/test_gpu_train.py::test_train_gradient_per_parameter's, the d / d c
criterion tests/test_gpu_input_grad.py::check_columns."""

import functools
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

from tests.custom_loss_oracle import make_cot
from tests.flowcases import CONFIGS, _blob, _trainer, chain_spec, make_case, make_variables

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
WORKER = str(Path(__file__).resolve().parent / "dist_worker_custom.py")
TINY_ROWS = 3
F32 = np.float32

CASES = [("small", 128, 61), ("cfg2", 128, 62), ("cfg4", 128, 63), ("bounded", 256, 89), ("odd", 300, 69),
         ("gelu", 128, 64), ("small", 2, 86), ("cfg4", 3, 88)]


@functools.lru_cache(maxsize=None)
def oracle(name, N, seed, mode):
    """The oracle's .npz of one case and mode (a CPU-only child process), once per session."""
    with tempfile.TemporaryDirectory() as d:
        out = Path(d) / "o.npz"
        subprocess.run([sys.executable, "-m", "tests.custom_loss_oracle", name, str(N), str(seed), mode, str(out)],
                       cwd=ROOT, check=True, timeout=600)
        return dict(np.load(out))


def _get(tree, path):
    for k in path:
        tree = tree[k]
    return np.asarray(tree, np.float64)


def _record(rec):
    from tests.test_gpu_flow import _append_record

    _append_record("grad_parity.jsonl", rec)


def _cot(ref):
    """The oracle's cotangent in fp32, 0 on the rows autograd loses."""
    cot = ref["cot"].astype(F32)
    cot[ref["dropped"]] = 0.0
    return cot


def check_params(tag, gg, ref, N, what):
    """test_train_gradient_per_parameter's rule over every parameter tensor:
    |g - g64| <= 1e-5 max|g64| + 2 max(|g32 - g64|, |g64' - g64|), maxima over
    the tensor; a tensor identically zero in float64 at <= 3 rows is held to
    1e-5 of the largest tensor's scale."""
    keys = sorted(k for k in ref if k.startswith("g64:"))
    assert keys
    for k in ref:  # after the drop every oracle gradient is finite
        if k.startswith(("g64", "g32_", "g64p_")):
            assert np.isfinite(ref[k]).all(), f"{tag}: oracle {k} not finite"
    tiny = N <= TINY_ROWS
    worst, bad = {}, []
    tree_scale = max(np.abs(ref[k]).max() for k in keys)
    for key in keys:
        path = tuple(key[4:].split("/"))
        r64 = ref[key]
        got = _get(gg, path)
        assert got.shape == r64.shape, path
        scale = max(np.abs(r64).max(), 1e-30)
        e = np.abs(got - r64)
        e32 = max(np.abs(ref[f"g32_{k}:" + key[4:]] - r64).max() for k in range(3))
        cond = max(np.abs(ref[f"g64p_{k}:" + key[4:]] - r64).max() for k in range(2))
        ok = e <= 1e-5 * scale + 2 * max(e32, cond)
        if tiny and not r64.any():
            scale = tree_scale
            ok = e <= 1e-5 * tree_scale
        worst["/".join(path)] = (float(e.max() / scale), float(e32 / scale), float(cond / scale))
        print(f"  {tag} {'/'.join(path)}: gpu {e.max() / scale:.3g} fp32 autograd {e32 / scale:.3g} conditioning "
              f"{cond / scale:.3g}")
        if not ok.all():
            bad.append(f"{'/'.join(path)}: {np.sum(~ok)} of {ok.size} over, max rel {e.max() / scale:.3g} "
                       f"(fp32 autograd {e32 / scale:.3g}, conditioning {cond / scale:.3g})")
    _record({"case": tag, "rows": N, "what": what, "leaves": len(worst),
             "gpu_max_rel_err_vs_fp64": max(v[0] for v in worst.values()),
             "torch32_max_rel_err_vs_fp64": max(v[1] for v in worst.values()),
             "conditioning_max_rel": max(v[2] for v in worst.values()), "over": bad})
    assert not bad, bad


# ---- 1. the parameter gradient, both modes ------------------------------------
GRAD_PARAMS = [(n, N, s, mode, "1") for (n, N, s) in CASES for mode in ("train", "eval")] + [("cfg4", 128, 63, "train", "0")]


@pytest.mark.parametrize("name,N,seed,mode,bn_small", GRAD_PARAMS)
def test_custom_gradient_per_parameter(name, N, seed, mode, bn_small, monkeypatch):
    """forward + backward with a standard-normal cotangent: every parameter
    tensor by :func:`check_params`, the statistics entries exactly 0, and
    d / d c by ``check_columns``.  The cases cover the single-block and the
    tree BatchNorm paths (ZF_TRAIN_BN_SMALL), the runtime-K and compiled-K
    spline reverse, one-sided ShiftBounds, gelu, 2 and 3 rows."""
    from tests.test_gpu_input_grad import check_columns

    monkeypatch.setenv("ZF_TRAIN_BN_SMALL", bn_small)
    case = make_case(name, N=N, seed=seed)
    ref = oracle(name, N, seed, mode)
    assert ref["dropped"].mean() <= 0.02 and not (mode == "train" and ref["dropped"].any())
    tr = _trainer(case, N)
    lp = tr.forward(case["x"], case["c"], train=mode == "train", update_stats=False)
    assert lp.shape == (N,) and lp.dtype == F32
    C = case["cfg"]["C"]
    tag = f"{name}/N={N}/{mode}" + ("" if bn_small == "1" else "/bn_small=0")
    if C:
        g, gc = tr.backward(_cot(ref), cond_grad=True)
    else:
        g = tr.backward(_cot(ref))
    assert g.shape == tr.program.blob.shape and g.dtype == F32
    assert np.all(g[tr.program.param_mask == 0] == 0), "statistics entries of the gradient must be exactly 0"
    check_params(tag, tr.grad_tree(g), ref, N, f"custom-loss parameter gradient ({mode})")
    if C:
        assert gc.shape == case["c"].shape and gc.dtype == F32
        rec = {"case": tag, "rows": N, "what": f"custom-loss d / d c ({mode})"}
        try:
            check_columns(tag, "gc", gc, ref, rec)
        finally:
            _record(rec)


# ---- 2. the per-row log_prob -----------------------------------------------------
@pytest.mark.parametrize("name,N,seed", [("cfg4", 128, 63), ("odd", 300, 69), ("bounded", 256, 89)])
def test_forward_log_prob(name, N, seed):
    """Eval: the bits of ``log_prob_vjp``'s lp (the same forward) and
    ``check_lp``.  Train: |lp - lp64| <= 1e-5 max|lp64| + 2 max(|lp32 - lp64|,
    |lp64' - lp64|), and -mean(lp) within rel 2e-5 / abs 2e-5 of the oracle's."""
    from tests.test_gpu_flow import check_lp
    from zenflow_amd._lib import DeviceArray

    case = make_case(name, N=N, seed=seed)
    tr = _trainer(case, N)
    lp = tr.forward(case["x"], case["c"], train=False)
    xd, cd = DeviceArray.from_numpy(case["x"]), DeviceArray.from_numpy(case["c"])
    lpv, _, _ = tr.log_prob_vjp(xd, cd)
    assert np.array_equal(lp.view(np.uint32), lpv.numpy().view(np.uint32))
    check_lp(lp, case, f"{name}/forward(eval)")
    lpd = tr.forward(xd, cd, train=False)  # device in, device out
    assert isinstance(lpd, DeviceArray) and np.array_equal(lpd.numpy().view(np.uint32), lp.view(np.uint32))
    ref = oracle(name, N, seed, "train")
    lp64 = ref["lp64"]
    assert np.isfinite(lp64).all()
    lpt = tr.forward(case["x"], case["c"], train=True, update_stats=False).astype(np.float64)
    e32 = max(np.abs(ref[f"lp32_{r}"] - lp64).max() for r in range(3))
    cond = max(np.abs(ref[f"lp64p_{r}"] - lp64).max() for r in range(2))
    e = np.abs(lpt - lp64)
    scale = np.abs(lp64).max()
    print(f"{name}/forward(train): gpu {e.max() / scale:.3g} fp32 autograd {e32 / scale:.3g} conditioning {cond / scale:.3g}")
    assert (e <= 1e-5 * scale + 2 * max(e32, cond)).all()
    assert -lpt.mean() == pytest.approx(-lp64.mean(), rel=2e-5, abs=2e-5)


# ---- 3. eval gc is the VJP's ---------------------------------------------------------
@pytest.mark.parametrize("name,N,seed", [("cfg4", 128, 63), ("odd", 300, 69)])
def test_eval_gc_is_the_vjps(name, N, seed):
    """``backward(cot, cond_grad=True)`` after ``forward(train=False)``: gc
    has the bits of ``log_prob_vjp``'s dc (the parameter gradients only add
    stores)."""
    from zenflow_amd._lib import DeviceArray

    case = make_case(name, N=N, seed=seed)
    cot = make_cot(N, seed).astype(F32)
    tr = _trainer(case, N)
    tr.forward(case["x"], case["c"], train=False)
    _, gc = tr.backward(cot, cond_grad=True)
    _, _, dc = tr.log_prob_vjp(DeviceArray.from_numpy(case["x"]), DeviceArray.from_numpy(case["c"]),
                               DeviceArray.from_numpy(cot))
    assert np.abs(gc).max() > 0
    assert np.array_equal(gc.view(np.uint32), dc.numpy().view(np.uint32))


# ---- 4. apply_gradient is the step's second half -----------------------------------
def _chain():
    from zenflow_amd import optim

    return optim.chain(optim.clip_by_global_norm(1.0),
                       optim.adamw(optim.warmup_cosine_decay_schedule(0.0, 2e-3, 2, 10)))


def _flat_state(st):
    from zenflow_amd.io import flatten_variables

    out = {"count": np.asarray(st["count"]), "lr": np.asarray(st["learning_rate"]), "gn": np.asarray(st["grad_norm"])}
    for k, tree in enumerate(st["slots"]):
        for name, v in flatten_variables({"params": tree}).items():
            out[f"{k}:{name}"] = np.asarray(v)
    return out


@pytest.mark.parametrize("opt", ["nadamw", "chain"])
def test_apply_gradient_is_the_steps_second_half(opt):
    """Three successive batches: ``step`` on one trainer, ``loss_grad(update_stats=True)``
    + ``apply_gradient(g)`` on another: blob and ``opt_state()`` bit-identical
    after every batch."""
    case = make_case("cfg4", N=3 * 128, seed=63)
    kw = {} if opt == "nadamw" else {"optimizer": _chain()}
    a, b = _trainer(case, 128, **kw), _trainer(case, 128, **({} if opt == "nadamw" else {"optimizer": _chain()}))
    for i in range(3):
        x, c = case["x"][128 * i:128 * (i + 1)], case["c"][128 * i:128 * (i + 1)]
        a.step(x, c)
        _, g = b.loss_grad(x, c, update_stats=True)
        b.apply_gradient(g)
        assert np.array_equal(_blob(a).view(np.uint32), _blob(b).view(np.uint32)), f"batch {i}: blob"
        sa, sb = _flat_state(a.opt_state()), _flat_state(b.opt_state())
        assert sa.keys() == sb.keys() and int(sa["count"]) == i + 1
        for k in sa:
            assert np.array_equal(sa[k], sb[k], equal_nan=True), f"batch {i}: opt_state {k}"
    assert not np.array_equal(_blob(a), _trainer(case, 128).program.blob)


# ---- 5. statistics ----------------------------------------------------------------------
@pytest.mark.parametrize("name,N,seed", [("cfg4", 128, 63), ("bounded", 256, 89)])
def test_statistics(name, N, seed):
    """``forward(train=True, update_stats=True)`` leaves the statistics of
    ``loss_grad(update_stats=True)``; an eval-mode forward + backward leaves
    the whole blob as it was."""
    case = make_case(name, N=N, seed=seed)
    a, b = _trainer(case, N), _trainer(case, N)
    blob0 = _blob(a)
    a.forward(case["x"], case["c"])  # update_stats defaults to train
    a.backward(make_cot(N, seed))
    b.loss_grad(case["x"], case["c"], update_stats=True)
    assert np.array_equal(_blob(a).view(np.uint32), _blob(b).view(np.uint32))
    assert not np.array_equal(_blob(a).view(np.uint32), blob0.view(np.uint32))
    e = _trainer(case, N)
    e.forward(case["x"], case["c"], train=False)
    e.backward(make_cot(N, seed))
    assert np.array_equal(_blob(e).view(np.uint32), blob0.view(np.uint32))
    f = _trainer(case, N)
    f.forward(case["x"], case["c"], train=True, update_stats=False)
    f.backward(make_cot(N, seed))
    assert np.array_equal(_blob(f).view(np.uint32), blob0.view(np.uint32))


# ---- 6. non-finite rows and zero cotangents --------------------------------------------
def _odd_two_sided(N, seed):
    """``odd`` (truncated-normal latent) with dim 0 bounded on both sides,
    (-6, 6).  ShiftBounds maps a two-sided dim linearly without a clamp
    (bijectors.py:186-189), so a row at x_0 = 9 reaches the latent at 1.25,
    outside its support, with every intermediate finite.  With ``odd`` as it
    is no input can: the unbounded dims are clamped to [0, 1] in eval mode and
    covered by the batch min / max in train mode."""
    from oracle import zf_oracle as O

    cfg = dict(CONFIGS["odd"], bounds=((0, -6.0, 6.0),))
    rng = np.random.default_rng(seed)
    spec, variables = make_variables(cfg, rng)
    xs = rng.standard_normal((4096, cfg["D"])).astype(F32)
    _, _, sb = O.shift_bounds_forward(spec["bijectors"][0], {}, xs, train=True)
    variables["batch_stats"]["bijector"]["bijectors_0"] = {k: np.asarray(v, F32) for k, v in sb.items()}
    x = rng.standard_normal((N, cfg["D"])).astype(F32)
    c = rng.standard_normal((N, cfg["C"])).astype(F32)
    assert chain_spec(cfg) == spec
    return {"cfg": cfg, "variables": variables, "x": x, "c": c}


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_non_finite_rows_and_zero_cotangents(mode):
    """Two rows outside the latent's support: their lp is finfo.min, and the
    gradient and gc have the bits of the same call with those rows' cotangent
    at 0.  Eval mode: their gc rows are exactly 0, and what a zero-cotangent
    row holds changes no bit of the gradient."""
    N, rows = 300, [7, 211]
    case = _odd_two_sided(N, 69)
    x, c = case["x"].copy(), case["c"]
    x[rows, 0] = 9.0
    cot = make_cot(N, 69).astype(F32)
    cot0 = cot.copy()
    cot0[rows] = 0.0
    train = mode == "train"

    def run(x, cot):
        tr = _trainer(case, N)
        lp = tr.forward(x, c, train=train, update_stats=False)
        g, gc = tr.backward(cot, cond_grad=True)
        return lp, g, gc

    lp, g, gc = run(x, cot)
    keep = np.ones(N, bool)
    keep[rows] = False
    assert np.all(lp[rows] == np.finfo(F32).min) and np.isfinite(lp[keep]).all() and np.all(lp[keep] > -1e30)
    _, g0, gc0 = run(x, cot0)
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    assert np.array_equal(g.view(np.uint32), g0.view(np.uint32))
    assert np.array_equal(gc.view(np.uint32), gc0.view(np.uint32))
    if not train:
        # (train mode: a zero-cotangent row still has a d / d c through the batch
        # statistics, as zero-weight rows of the weighted loss do)
        assert np.all(gc[rows] == 0)
        # eval rows are independent: what a zero-cotangent row holds changes no bit
        x2 = x.copy()
        x2[rows] = x[[0, 1]]
        _, g2, gc2 = run(x2, cot0)
        assert np.array_equal(g2.view(np.uint32), g.view(np.uint32))
        assert np.array_equal(gc2[keep].view(np.uint32), gc[keep].view(np.uint32)) and np.all(gc2[rows] == 0)


# ---- 7. the state machine -------------------------------------------------------------------
def test_state_machine():
    from zenflow_amd._lib import DeviceArray

    N = 128
    case = make_case("cfg4", N=N, seed=63)
    x, c = case["x"], case["c"]
    cot = make_cot(N, 63)
    tr = _trainer(case, N)
    with pytest.raises(ValueError, match="pending forward"):
        tr.backward(cot)
    tr.forward(x, c)
    g = tr.backward(cot)
    with pytest.raises(ValueError, match="pending forward"):
        tr.backward(cot)
    xd, cd = DeviceArray.from_numpy(x), DeviceArray.from_numpy(c)
    for between in (lambda: tr.step(x, c), lambda: tr.loss_grad(x, c), lambda: tr.log_prob_vjp(xd, cd),
                    lambda: tr.apply_gradient(g)):
        tr.forward(x, c)
        between()
        with pytest.raises(ValueError, match="pending forward"):
            tr.backward(cot)
    with pytest.raises(ValueError, match="update_stats"):
        tr.forward(x, c, train=False, update_stats=True)
    with pytest.raises(ValueError, match="batch_max"):
        _trainer(case, 64).forward(x, c)
    # the C entry's own checks (the Python ones above come first)
    from zenflow_amd import _lib as L

    lib = L.load_library()
    lp = DeviceArray((N,))
    assert lib.zf_trainer_forward(tr.handle, xd.ptr, cd.ptr, N, N, 0, 1, lp.ptr, L.stream()) == -1
    assert lib.zf_trainer_backward(tr.handle, None, None, None, L.stream()) == -1
    assert "no forward pending" in lib.zf_last_error().decode()
    # and the trainer still steps
    before = _blob(tr)
    tr.step(x, c)
    assert np.isfinite(tr.last_loss()) and not np.array_equal(_blob(tr), before)


# ---- 8. determinism ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_determinism(mode):
    N = 300
    case = make_case("odd", N=N, seed=69)
    cot = make_cot(N, 69)
    out = []
    for _ in range(2):
        tr = _trainer(case, N)
        lp = tr.forward(case["x"], case["c"], train=mode == "train")
        g, gc = tr.backward(cot, cond_grad=True)
        out.append((lp, g, gc))
    for u, v in zip(*out):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    if mode == "eval":  # and a second pass over the same trainer's arena (the blob has not changed)
        tr.forward(case["x"], case["c"], train=False)
        assert np.array_equal(tr.backward(cot).view(np.uint32), out[0][1].view(np.uint32))


# ---- 9. gradient accumulation ---------------------------------------------------------------------
def test_gradient_accumulation():
    """Eval mode, cfg2, 128 rows as 2 x 64: g_a + g_b (host) against the
    oracle of the whole batch by the rule of test 1 (the two sums differ in
    order only), and ``apply_gradient(g_a + g_b)`` runs."""
    name, N, seed = "cfg2", 128, 62
    case = make_case(name, N=N, seed=seed)
    ref = oracle(name, N, seed, "eval")
    cot = _cot(ref)
    tr = _trainer(case, 64)
    gs = []
    for lo in (0, 64):
        tr.forward(case["x"][lo:lo + 64], None, train=False)
        gs.append(tr.backward(cot[lo:lo + 64]))
    g = gs[0] + gs[1]
    check_params(f"{name}/N=2x64/eval accumulated", tr.grad_tree(g), ref, N, "custom-loss gradient, accumulated")
    before = _blob(tr)
    tr.apply_gradient(g)
    tree = _trainer(case, 64)
    tree.apply_gradient(tr.grad_tree(g))  # a FLAX tree goes through tree_to_blob
    assert not np.array_equal(_blob(tr), before)
    assert np.array_equal(_blob(tr).view(np.uint32), _blob(tree).view(np.uint32))
    assert tr.opt_state()["count"] == 1


# ---- 10. it trains -----------------------------------------------------------------------------------
F_SIG, BOX = 0.7, ((-1.5, 2.5), (-1.0, 1.5))
BKG = 1.0 / ((BOX[0][1] - BOX[0][0]) * (BOX[1][1] - BOX[1][0]))


def _mixture_sample(n, seed):
    """70% two moons, 30% uniform on BOX."""
    from sklearn.datasets import make_moons

    rng = np.random.default_rng(seed)
    X, _ = make_moons(n, noise=0.05, random_state=seed)
    bkg = rng.uniform(size=n) >= F_SIG
    U = np.stack([rng.uniform(*BOX[0], n), rng.uniform(*BOX[1], n)], axis=1)
    X[bkg] = U[bkg]
    return X.astype(F32)


def _mixture_loss(lp):
    lp = np.asarray(lp, np.float64)
    return float(-np.mean(np.log(F_SIG * np.exp(lp) + (1 - F_SIG) * BKG)))


def _mixture_cot(lp):
    lp = np.asarray(lp, np.float64)
    s = F_SIG * np.exp(lp)
    return (-s / (s + (1 - F_SIG) * BKG) / lp.shape[0]).astype(F32)


def _moons_trainer(X, batch_max):
    from tests.dist_worker import two_moons_flow
    from zenflow_amd.random import PRNGKey
    from zenflow_amd.train import Trainer

    flow = two_moons_flow()
    return Trainer(flow, flow.init(PRNGKey(0), X[:1], None), 2, 0, batch_max)


def test_mixture_likelihood_trains():
    """A two-moons signal next to a uniform background, f = 0.7: 60 steps of
    forward / ``cot = -f e^lp / (f e^lp + (1 - f) bkg) / N`` / backward /
    apply_gradient on 512 rows.  The mixture loss of 512 held-out rows ends
    below its starting value, and below what 60 plain ``step``s on the same
    contaminated rows reach (the parent's capability: the flow then fits the
    signal and the background together).  The held-out loss is a train-mode
    forward without a statistics update: after 60 steps the running
    statistics (momentum 0.99) still hold 55% of their initial values."""
    X, Xt = _mixture_sample(512, 3), _mixture_sample(512, 4)

    def held_out(tr):
        return _mixture_loss(tr.forward(Xt, train=True, update_stats=False))

    mix, plain = _moons_trainer(X, 512), _moons_trainer(X, 512)
    start = held_out(mix)
    assert held_out(plain) == start
    for _ in range(60):
        lp = mix.forward(X)
        mix.backward(_mixture_cot(lp))
        mix.apply_gradient()
        plain.step(X)
    end, ref = held_out(mix), held_out(plain)
    print(f"mixture loss, held out: start {start:.6g}, custom loss {end:.6g}, plain steps {ref:.6g}")
    assert np.isfinite([start, end, ref]).all()
    assert end < start and end < ref


def test_frozen_statistics_fine_tuning():
    """After 40 plain steps on 512 rows: 30 eval-mode steps (forward(train=False),
    cot = -1/64, backward, apply_gradient) on 64 other rows lower their eval-mode
    NLL, and leave every statistic as it was."""
    X = _mixture_sample(512, 3)
    Xs = _mixture_sample(64, 5)
    tr = _moons_trainer(X, 512)
    for _ in range(40):
        tr.step(X)
    mask = tr.program.param_mask == 0
    stats0 = _blob(tr)[mask]
    start = float(-np.mean(tr.forward(Xs, train=False).astype(np.float64)))
    cot = np.full(64, -1.0 / 64, F32)
    for _ in range(30):
        tr.forward(Xs, train=False)
        tr.backward(cot)
        tr.apply_gradient()
    end = float(-np.mean(tr.forward(Xs, train=False).astype(np.float64)))
    print(f"frozen-statistics fine-tuning: eval NLL {start:.6g} -> {end:.6g}")
    assert np.isfinite([start, end]).all() and end < start
    assert np.array_equal(_blob(tr)[mask].view(np.uint32), stats0.view(np.uint32))


# ---- 11. two ranks ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_two_ranks_match_one_device_bitwise(tmp_path, mode):
    """cfg4, 128 rows as 2 x 64 (dist.HostAllgather): lp (concatenated), the
    gradient and the blob after ``apply_gradient`` are one device's, bit for
    bit, on both ranks."""
    from zenflow_amd.launch import spawn

    name, N, seed = "cfg4", 128, 63
    env = dict(os.environ, ZF_TEST_CASE=f"{name}:{N}:{seed}", ZF_TEST_MODE=mode, ZF_DEVICE="0")
    assert spawn(2, [WORKER, str(tmp_path)], env=env, timeout=240) == 0
    ranks = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]
    case = make_case(name, N=N, seed=seed)
    tr = _trainer(case, N)
    lp = tr.forward(case["x"], case["c"], train=mode == "train")
    g = tr.backward(make_cot(N, seed).astype(F32))
    tr.apply_gradient(g)
    blob = _blob(tr)
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    lp2 = np.concatenate([ranks[0]["lp"], ranks[1]["lp"]])
    assert np.array_equal(lp2.view(np.uint32), lp.view(np.uint32)), f"{np.sum(lp2 != lp)} lp rows differ"
    for k, r in enumerate(ranks):
        assert np.array_equal(r["grad"].view(np.uint32), g.view(np.uint32)), \
            f"rank {k}: {np.sum(r['grad'] != g)} gradient entries differ"
        assert np.array_equal(r["blob"].view(np.uint32), blob.view(np.uint32)), \
            f"rank {k}: {np.sum(r['blob'] != blob)} blob entries differ"
