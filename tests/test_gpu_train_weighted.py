"""Weighted maximum likelihood on the GPU: ``Trainer.loss_grad / step(w=...)``
and ``train(W_train=, W_test=)``.

With the reference the loss is user-visible JAX: a user with weighted samples
(event weights, sWeights, importance weights) writes
``-(w * lp).sum() / w.sum()`` around ``flow.apply(..., train=True)`` and
``jax.grad`` does the rest.  Here that loss and its reverse pass run in the
device trainer; the float64 reference is tests/weighted_grad_oracle.py.

Every test uses the weights of ``weighted_grad_oracle.make_weights``:
exponential(1), an eighth of the rows at 0 and a sixteenth at -0.25 (from 8
rows on).  The parameter-gradient criterion is
tests/test_gpu_train.py::test_train_gradient_per_parameter's, the d loss / d c
criterion tests/test_gpu_input_grad.py::check_columns."""

import functools
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

from tests.flowcases import _blob, _trainer, make_case
from tests.weighted_grad_oracle import make_weights

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
WORKER = str(Path(__file__).resolve().parent / "dist_worker_weighted.py")
TINY_ROWS = 3


@functools.lru_cache(maxsize=None)
def oracle(name, N, seed):
    """The oracle's .npz of one case (a CPU-only child process), once per session."""
    with tempfile.TemporaryDirectory() as d:
        out = Path(d) / "w.npz"
        subprocess.run([sys.executable, "-m", "tests.weighted_grad_oracle", name, str(N), str(seed), str(out)],
                       cwd=ROOT, check=True, timeout=600)
        return dict(np.load(out))


def _get(tree, path):
    for k in path:
        tree = tree[k]
    return np.asarray(tree, np.float64)


def _record(rec):
    from tests.test_gpu_flow import _append_record

    _append_record("grad_parity.jsonl", rec)


GRAD_CASES = [("small", 128, 61), ("cfg2", 128, 62), ("cfg4", 128, 63), ("bounded", 256, 89), ("odd", 300, 69),
              ("small", 2, 86), ("cfg4", 3, 88), ("cfg2", 16384, 84)]


@pytest.mark.parametrize("name,N,seed", GRAD_CASES)
def test_weighted_gradient_per_parameter(name, N, seed):
    """The weighted loss within rel 2e-5 / abs 2e-5 of the float64 oracle's,
    and every element of every parameter tensor within
    |g - g64| <= 1e-5 max|g64| + 2 max(|g32 - g64|, |g64' - g64|) (maxima over
    the tensor; test_train_gradient_per_parameter's rule, its allowance for
    tensors that are identically zero in float64 at <= 3 rows included).

    The cases cover the fused (128, 256, 16384 rows) and unfused (300, 2, 3)
    loss-leaf forms, the single-block and the tree BatchNorm paths, the
    runtime-K (small, odd) and compiled-K spline reverse, one-sided
    ShiftBounds (bounded), a truncated-normal latent (odd)."""
    case = make_case(name, N=N, seed=seed)
    ref = oracle(name, N, seed)
    assert np.isfinite(ref["lp64"]).all()
    w = make_weights(N, seed)
    assert w.astype(np.float64).sum() > 0
    tr = _trainer(case, N)
    loss, g = tr.loss_grad(case["x"], case["c"], w=w)
    gg = tr.grad_tree(g)
    print(f"{name}/N={N}: weighted loss gpu {loss!r} oracle {float(ref['loss64'])!r}")
    assert loss == pytest.approx(float(ref["loss64"]), rel=2e-5, abs=2e-5)
    tiny = N <= TINY_ROWS
    worst, bad = {}, []
    tree_scale = max(np.abs(ref[k]).max() for k in ref if k.startswith("g64:"))
    for key in sorted(k for k in ref if k.startswith("g64:")):
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
        print(f"  {'/'.join(path)}: gpu {e.max() / scale:.3g} fp32 autograd {e32 / scale:.3g} conditioning "
              f"{cond / scale:.3g}")
        if not ok.all():
            bad.append(f"{'/'.join(path)}: {np.sum(~ok)} of {ok.size} over, max rel {e.max() / scale:.3g} "
                       f"(fp32 autograd {e32 / scale:.3g}, conditioning {cond / scale:.3g})")
    _record({"case": name, "rows": N, "what": "weighted parameter gradient", "leaves": len(worst),
             "gpu_max_rel_err_vs_fp64": max(v[0] for v in worst.values()),
             "torch32_max_rel_err_vs_fp64": max(v[1] for v in worst.values()),
             "conditioning_max_rel": max(v[2] for v in worst.values()), "over": bad})
    assert not bad, bad


@pytest.mark.parametrize("name,N,seed", [("cfg4", 128, 63), ("odd", 300, 69), ("bounded", 256, 89)])
def test_weighted_cond_grad(name, N, seed):
    """d loss / d c of the weighted loss by check_columns' rule (zero-weight
    rows carry a gradient through the batch statistics); loss and gradient
    have the same bits with and without ``cond_grad``."""
    from tests.test_gpu_input_grad import check_columns

    case = make_case(name, N=N, seed=seed)
    ref = oracle(name, N, seed)
    w = make_weights(N, seed)
    x, c = case["x"], case["c"]
    tr = _trainer(case, N)
    loss0, g0 = tr.loss_grad(x, c, w=w)
    loss, g, gc = tr.loss_grad(x, c, w=w, cond_grad=True)
    assert loss == loss0 and np.array_equal(g, g0)
    assert gc.shape == c.shape and gc.dtype == np.float32
    rec = {"case": f"{name}/weighted", "rows": N, "what": "d loss / d c (train, weighted)"}
    try:
        check_columns(f"{name}/weighted", "gc", gc, ref, rec)
    finally:
        _record(rec)
    # the step with gc (eager) and without (captured graph): the same parameters
    plain, cond = _trainer(case, N), _trainer(case, N)
    for _ in range(2):
        plain.step(x, c, w=w)
        gcs = cond.step(x, c, w=w, cond_grad=True)
    assert gcs.shape == c.shape and np.isfinite(gcs).all()
    assert plain.last_loss() == cond.last_loss()
    assert np.array_equal(_blob(plain), _blob(cond), equal_nan=True)


@pytest.mark.parametrize("name,N,seed", [("cfg4", 128, 63), ("odd", 300, 69)])
def test_weight_scale_invariance_bitwise(name, N, seed):
    """w and 4 w: the same loss, gradient and (after three steps) parameters,
    bit for bit — the fp64 weight sum scales exactly and every quotient by it
    is rounded once."""
    case = make_case(name, N=N, seed=seed)
    w = make_weights(N, seed)
    x, c = case["x"], case["c"]
    out = []
    for s in (1.0, 4.0):
        tr = _trainer(case, N)
        loss, g = tr.loss_grad(x, c, w=(s * w).astype(np.float32))
        for _ in range(3):
            tr.step(x, c, w=(s * w).astype(np.float32))
        out.append((loss, g, tr.last_loss(), _blob(tr)))
    assert np.isfinite(out[0][0]) and out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2]
    assert np.array_equal(out[0][3], out[1][3], equal_nan=True)


@pytest.mark.parametrize("name,N,seed", [("cfg4", 128, 63), ("bounded", 256, 89), ("cfg2", 1024, 81)])
def test_statistics_are_unweighted(name, N, seed):
    """After ``loss_grad(..., update_stats=True)`` the batch_stats tree (the
    BatchNorm running mean / var, the ShiftBounds running min / max) has the
    same bits with weights as without; the gradient does not."""
    from zenflow_amd.io import flatten_variables

    case = make_case(name, N=N, seed=seed)
    w = make_weights(N, seed)
    a, b = _trainer(case, N), _trainer(case, N)
    _, ga = a.loss_grad(case["x"], case["c"], update_stats=True, w=w)
    _, gb = b.loss_grad(case["x"], case["c"], update_stats=True)
    fa = flatten_variables({"batch_stats": a.variables()["batch_stats"]})
    fb = flatten_variables({"batch_stats": b.variables()["batch_stats"]})
    assert fa.keys() == fb.keys() and len(fa) > 0
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), k
    assert not np.array_equal(ga, gb)
    # and they did move off their initial values
    f0 = flatten_variables({"batch_stats": case["variables"]["batch_stats"]})
    assert any(k in f0 and f0[k].size == fa[k].size
               and not np.array_equal(np.asarray(f0[k], np.float32).ravel(), fa[k].ravel()) for k in fa)


def test_weighted_graph_matches_eager_and_caches_do_not_collide(monkeypatch):
    """One trainer alternates weighted and unweighted steps on the same batch
    size (each kind replays its own captured graph), a second does the same
    with ZF_TRAIN_GRAPH=0: the same losses and parameters, bit for bit."""
    name, N, seed = "cfg4", 300, 65
    case = make_case(name, N=N, seed=seed)
    w = make_weights(N, seed)
    x, c = case["x"], case["c"]
    out = []
    for graph in ("1", "0"):
        monkeypatch.setenv("ZF_TRAIN_GRAPH", graph)
        tr = _trainer(case, 256)
        losses = []
        for i in range(6):
            if i % 2 == 0:
                tr.step(x[:256], c[:256], w=w[:256])
            else:
                tr.step(x[:256], c[:256])
            losses.append(tr.last_loss())
        out.append((losses, _blob(tr)))
    assert np.isfinite(out[0][0]).all()
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1], equal_nan=True)
    # the weighted and the unweighted loss of one batch differ: the steps were of both kinds
    assert len(set(out[0][0])) == 6


def test_weighted_graph_cache_eviction(monkeypatch):
    """The weighted step's graph cache holds eight batch sizes and is
    emptied when a ninth arrives, like the unweighted one
    (tests/test_gpu_train.py::test_step_graph_cache_eviction): ten sizes in
    two passes, bit-identical to the eagerly launched steps."""
    w = make_weights(73, 90)
    out = []
    for graph in ("1", "0"):
        monkeypatch.setenv("ZF_TRAIN_GRAPH", graph)
        case = make_case("small", N=73, seed=90)
        tr = _trainer(case, 73)
        losses = []
        for _ in range(2):
            for rows in range(64, 74):
                tr.step(case["x"][:rows], None, w=w[:rows])
                losses.append(tr.last_loss())
        out.append((losses, _blob(tr)))
    assert np.isfinite(out[0][0]).all()
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))


def test_train_weighted_two_moons():
    """``train(W_train=, W_test=)`` with weight 1 on one moon and 0 on the
    other: the reference's return structure, finite losses, and a final
    weighted test loss below the weighted test loss of the variables an
    unweighted ``train()`` returns (same seed and epochs) — the unweighted
    model spreads its mass over both moons, at least log 2 worse at the
    optimum.

    Both runs train for all 30 epochs (``warmup=30``: no early stopping).
    With 30 epochs the default patience is int(0.05 * 30) = 1, which stops at
    the first epoch after the sixth whose test loss is not below the one
    before; the two runs would then stop at different epochs, and the
    comparison is meant at the same seed and epochs.  (The eval-mode metric
    runs on the running statistics, momentum 0.99, which lag the parameters
    early on: measured here, the weighted run's test loss rises from 6.93 to
    7.97 over epochs 1 to 8 before it falls, so the default rule stops it after
    epoch 6 at 7.82 while the unweighted run, at 5.90 by this measure, goes on
    to epoch 29.  Over all 30 epochs: 4.22 against 5.90; over 100: -0.25
    against 0.77.)"""
    from sklearn.datasets import make_moons

    import zenflow_amd as zf
    from tests.dist_worker import two_moons_data, two_moons_flow
    from zenflow_amd.train import weighted_nll

    X = two_moons_data()
    _, y = make_moons(3000, noise=0.05, random_state=2)  # two_moons_data's labels
    W = (y == 0).astype(np.float32)
    flow = two_moons_flow()
    kw = dict(epochs=30, warmup=30, batch_size=512, progress=False, seed=0)
    best, best_epoch, lt, ls = zf.train(flow, X[:2400], X[2400:], W_train=W[:2400], W_test=W[2400:], **kw)
    assert isinstance(best, dict) and set(best) == {"params", "batch_stats"}
    assert len(lt) == len(ls) == 30 and 0 <= best_epoch < 30
    assert np.all(np.isfinite(lt)) and np.all(np.isfinite(ls))
    assert weighted_nll(flow.apply(best, X[2400:]), W[2400:]) == ls[best_epoch]
    plain, _, _, _ = zf.train(flow, X[:2400], X[2400:], **kw)
    ref = weighted_nll(flow.apply(plain, X[2400:]), W[2400:])
    print(f"weighted test loss: weighted training {ls[-1]:.6g} (best {ls[best_epoch]:.6g}), unweighted training {ref:.6g}")
    assert ls[-1] < ref


def test_train_rejects_a_non_positive_batch_sum():
    """Every epoch's batches are checked before its first step: weights whose
    sum over some batch is not positive raise ValueError."""
    import zenflow_amd as zf
    from tests.dist_worker import two_moons_data, two_moons_flow

    X = two_moons_data()
    W = np.ones(2400, np.float32)
    W[::2] = -1.5
    with pytest.raises(ValueError, match="batch"):
        zf.train(two_moons_flow(), X[:2400], X[2400:], epochs=20, batch_size=512, progress=False, W_train=W)


def _one_device(name, N, seed, steps=3):
    case = make_case(name, N=N, seed=seed)
    w = make_weights(N, seed)
    tr = _trainer(case, N)
    loss, g = tr.loss_grad(case["x"], case["c"], w=w)
    for _ in range(steps):
        tr.step(case["x"], case["c"], w=w)
    return loss, g, tr.last_loss(), _blob(tr)


@pytest.mark.parametrize("name,N,seed", [("cfg2", 1024, 81), ("cfg4", 2048, 82)])
def test_two_ranks_match_one_device_bitwise(tmp_path, name, N, seed):
    """Two ranks on one GPU (dist.HostAllgather), each on its half of the
    rows and weights: loss, gradient, and the parameters after three weighted
    steps are one device's, bit for bit, on both ranks."""
    from zenflow_amd.launch import spawn

    env = dict(os.environ, ZF_TEST_CASE=f"{name}:{N}:{seed}", ZF_TEST_STEPS="3", ZF_DEVICE="0")
    assert spawn(2, [WORKER, "dp", str(tmp_path)], env=env, timeout=240) == 0
    ranks = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]
    loss, g, last, blob = _one_device(name, N, seed)
    assert np.isfinite(loss)
    for k, r in enumerate(ranks):
        assert float(r["loss"]) == loss, f"rank {k} loss"
        assert np.array_equal(r["grad"], g), f"rank {k}: {np.sum(r['grad'] != g)} gradient entries differ"
        assert float(r["last_loss"]) == last, f"rank {k} last loss"
        assert np.array_equal(r["blob"], blob, equal_nan=True), f"rank {k}: {np.sum(r['blob'] != blob)} blob entries"


def test_train_function_two_ranks_match_one_device(tmp_path):
    """``train(..., W_train=, W_test=, comm=)`` on 2400 rows in batches of
    512 (the last one ragged): both ranks return the one-device losses, best
    epoch and variables, bit for bit."""
    import zenflow_amd as zf
    from tests.dist_worker import two_moons_data, two_moons_flow
    from tests.dist_worker_weighted import train_fn_weights
    from zenflow_amd.io import flatten_variables
    from zenflow_amd.launch import spawn

    env = dict(os.environ, ZF_TEST_EPOCHS="20", ZF_DEVICE="0")
    assert spawn(2, [WORKER, "train_fn", str(tmp_path)], env=env, timeout=300) == 0
    X = two_moons_data()
    Wtr, Wte = train_fn_weights()
    best, best_epoch, lt, ls = zf.train(two_moons_flow(), X[:2400], X[2400:], epochs=20, batch_size=512,
                                        progress=False, W_train=Wtr, W_test=Wte)
    assert np.all(np.isfinite(lt)) and np.all(np.isfinite(ls))
    flat = flatten_variables(best)
    for k in range(2):
        r = np.load(tmp_path / f"rank{k}.npz")
        assert int(r["best_epoch"]) == best_epoch
        assert np.array_equal(r["lt"], np.asarray(lt)) and np.array_equal(r["ls"], np.asarray(ls))
        for name, v in flat.items():
            assert np.array_equal(r["v:" + name], v), f"rank {k}: {name}"
