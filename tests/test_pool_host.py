"""Host side of the max pooling and of the standalone mean (zenflow_amd/nn.py
``ConditionNet(pool="max")``, zf_segment_pool): the plan accepts the max's
code, the variable tree does not depend on the pooling, the new entries reject bad
arguments before their first HIP call, and the oracle of tests/pool_oracle.py
against hand-computed cases.  No GPU is used."""

import ctypes
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def _desc(pool):
    from zenflow_amd import _lib as L

    d = L.ZfCondnetDesc()
    d.in_dim, d.out_dim, d.n_hidden, d.batch_norm, d.pool = 2, 8, 2, 1, pool
    d.hidden[0], d.hidden[1] = 16, 5
    return d


def test_plan_accepts_max():
    """Code 3: the blob size and every offset of code 1; 4 is still unknown
    (and so is 2, the standalone mean's code: tests/test_condnet_host.py)."""
    from zenflow_amd import _lib as L

    lib = L.load_library()
    assert (L.ZF_POOL_NONE, L.ZF_POOL_SUM, L.ZF_POOL_MEAN, L.ZF_POOL_MAX) == (0, 1, 2, 3)
    plans = []
    for pool in (L.ZF_POOL_SUM, L.ZF_POOL_MAX):
        d, n = _desc(pool), ctypes.c_int64()
        assert lib.zf_condnet_plan(ctypes.byref(d), ctypes.byref(n)) == 0, pool
        plans.append((n.value, d.off_bn, list(d.off_w), list(d.off_b)))
    assert plans[0][0] > 0 and plans[1] == plans[0]
    n = ctypes.c_int64()
    assert lib.zf_condnet_plan(ctypes.byref(_desc(4)), ctypes.byref(n)) == -1
    assert b"unknown pool" in lib.zf_last_error()
    assert lib.zf_condnet_plan(ctypes.byref(_desc(-1)), ctypes.byref(n)) == -1


def test_variable_tree_does_not_depend_on_the_pooling():
    from tests.test_condnet_host import _shapes
    from zenflow_amd import nn

    x, off = np.zeros((10, 2), np.float32), np.array([0, 4, 10])
    base = nn.ConditionNet(8, pool="sum").init(5, x, off)
    v = nn.ConditionNet(8, pool="max").init(5, x, off)
    assert _shapes(v) == _shapes(base)
    for col in ("params", "batch_stats"):
        a, b = dict(_flat(v[col])), dict(_flat(base[col]))
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    with pytest.raises(NotImplementedError):
        nn.ConditionNet(8, pool="median")
    assert {"segment_mean", "segment_max", "segment_sum"} <= set(nn.__all__)


def _flat(tree):
    from tests import condnet_oracle as CO

    return CO._flat(tree)


@pytest.mark.parametrize("pool,null,rc", [(0, None, -1), (4, None, -1), (-1, None, -1), (2, "h", -1), (3, "h", -1),
                                          (3, "ws", -1), (2, "out", -1), (1, "h", -1)])
def test_segment_pool_rejects_before_any_launch(pool, null, rc):
    """An unknown mode or a NULL pointer: ZF_EINVAL before the first HIP call,
    so host pointers stand in for device ones (as tests/test_abi.py does)."""
    from zenflow_amd import _lib as L

    lib = L.load_library()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    a = {k: (None if null == k else p) for k in ("h", "off", "out", "ws")}
    assert lib.zf_segment_pool(a["h"], 8, 3, a["off"], 2, pool, 0.0, 0, a["out"], None, None, a["ws"], None) == rc
    assert lib.zf_last_error()


def test_segment_pool_bcast_rejects_before_any_launch():
    from zenflow_amd import _lib as L

    lib = L.load_library()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data

    def call(pool, gc=p, idx=p, h=p, out=p, count=p, g=p, rate=0.0, F=3):
        return lib.zf_segment_pool_bcast(gc, idx, 8, F, 2, pool, rate, 0, h, out, count, g, None)

    assert call(4) == -1 and b"unknown pool" in lib.zf_last_error()
    assert call(0) == -1
    for pool in (L.ZF_POOL_MEAN, L.ZF_POOL_MAX):
        assert call(pool, count=None) == -1 and call(pool, gc=None) == -1 and call(pool, g=None) == -1
        assert call(pool, rate=1.0) == -1 and call(pool, F=65) == -2
    assert call(L.ZF_POOL_MAX, h=None) == -1 and call(L.ZF_POOL_MAX, out=None) == -1


def test_pool_workspace_bytes():
    """The sum's and the mean's workspace is zf_segment_sum's; the max adds one
    int32 per column and first-level chunk; 0 for what the entry rejects."""
    from zenflow_amd import _lib as L

    lib = L.load_library()
    base = lib.zf_segment_workspace_bytes(50_000, 1000, 8)
    assert lib.zf_segment_pool_workspace_bytes(50_000, 1000, 8, L.ZF_POOL_SUM) == base
    assert lib.zf_segment_pool_workspace_bytes(50_000, 1000, 8, L.ZF_POOL_MEAN) == base
    assert lib.zf_segment_pool_workspace_bytes(50_000, 1000, 8, L.ZF_POOL_MAX) == base + (50_000 // 512 + 1001) * 8 * 4
    assert lib.zf_segment_pool_workspace_bytes(50_000, 1000, 8, 4) == 0
    assert lib.zf_segment_pool_workspace_bytes(50_000, 1000, 65, L.ZF_POOL_MAX) == 0


# ---- the oracle against hand-computed cases ------------------------------------------------
def _pool_and_grad(d, ids, S, how, gc):
    import torch

    from tests import pool_oracle as PO

    t = torch.tensor(d, dtype=torch.float64, requires_grad=True)
    c = PO.pool(t, np.asarray(ids), S, how)
    (torch.tensor(gc, dtype=torch.float64) * c).sum().backward()
    return c.detach().numpy(), t.grad.numpy()


def test_oracle_max_by_hand():
    """Ties split the gradient evenly, an empty set gives a zero row and takes
    no gradient, rows in no set get none."""
    d = np.array([[1.0, -2.0], [3.0, -2.0], [3.0, -5.0], [0.5, 7.0], [9.0, 9.0]])
    ids = [0, 0, 0, 2, -1]  # set 1 is empty, the last row is in no set
    gc = np.array([[6.0, 4.0], [100.0, 100.0], [1.0, 2.0]])
    c, g = _pool_and_grad(d, ids, 3, "max", gc)
    assert np.array_equal(c, [[3.0, -2.0], [0.0, 0.0], [0.5, 7.0]])
    assert np.array_equal(g, [[0.0, 2.0], [3.0, 2.0], [3.0, 0.0], [1.0, 2.0], [0.0, 0.0]])


def test_oracle_mean_by_hand():
    d = np.array([[1.0, -2.0], [3.0, -2.0], [5.0, -5.0], [0.5, 7.0], [9.0, 9.0]])
    ids = [0, 0, 0, 2, -1]
    gc = np.array([[6.0, 3.0], [100.0, 100.0], [1.0, 2.0]])
    c, g = _pool_and_grad(d, ids, 3, "mean", gc)
    assert np.array_equal(c, [[3.0, -3.0], [0.0, 0.0], [0.5, 7.0]])
    assert np.array_equal(g, [[2.0, 1.0], [2.0, 1.0], [2.0, 1.0], [1.0, 2.0], [0.0, 0.0]])


def test_oracle_max_propagates_nan():
    import torch

    from tests import pool_oracle as PO

    d = np.array([[1.0, 2.0], [np.nan, 0.0], [4.0, -np.inf], [-np.inf, -np.inf]])
    c = PO.pool(torch.tensor(d), np.array([0, 0, 0, 1]), 2, "max").numpy()
    assert np.isnan(c[0, 0]) and c[0, 1] == 2.0 and np.isneginf(c[1]).all()
    gap, dmax = PO.max_gap(np.array([[1.0], [3.0], [3.0], [2.5], [7.0]]), np.array([0, 0, 0, 0, 1]), 2)
    assert gap == 0.5 and dmax == 7.0  # the tie at 3 is one distinct value; a set of one row has no gap


@pytest.mark.parametrize("pool", ["mean", "max"])
def test_oracle_worker_and_central_differences(pool):
    """``python -m tests.pool_oracle JOB OUT`` writes condnet_oracle's keys plus
    gx; the float64 gradients agree with central differences of sum(gc * c)
    along random directions in the parameters and in x."""
    import torch

    from tests import condnet_oracle as CO
    from tests import pool_oracle as PO
    from tests.test_condnet_host import _small_case

    cfg, variables, x, offsets, keep, rng = _small_case(4, pool, True, 0.3)
    ids, S = CO.ids_of(offsets, len(x)), len(offsets) - 1
    gc = rng.standard_normal((S, cfg["features"]))
    with tempfile.TemporaryDirectory() as d:
        job, out = Path(d) / "job.npz", Path(d) / "out.npz"
        CO.pack_job(job, cfg, variables, x, ids, S, keep=keep, gc=gc)
        subprocess.run([sys.executable, "-m", "tests.pool_oracle", str(job), str(out)], cwd=ROOT, check=True,
                       timeout=600)
        res = dict(np.load(out))
    assert res["c64"].shape == (S, cfg["features"]) and not res["c64"][1].any()  # the empty set
    for r in range(3):
        assert np.abs(res[f"c32_{r}"] - res["c64"]).max() <= 1e-5 * np.abs(res["c64"]).max()
    assert res["gx64"].shape == x.shape and "g64p_1:NNBlock_0/Dense_0/kernel" in res
    assert ("gap64" in res) == (pool == "max")
    jobd = {"cfg": cfg, "variables": variables, "x": x, "ids": ids, "S": S, "train": True, "mode": "net", "keep": keep}
    base = dict(CO._flat(variables["params"]))
    leaves = {k: res["g64:" + k] for k in base}

    def value(params, xs):
        r = PO.evaluate({**jobd, "x": xs}, torch.float64, variables={**variables, "params": params})
        return float((gc * r["c"]).sum())

    for trial in range(3):
        dp = {k: rng.standard_normal(v.shape) for k, v in base.items()}
        dx = rng.standard_normal(x.shape)
        an = sum(float((leaves[k] * dp[k]).sum()) for k in base) + float((res["gx64"] * dx).sum())
        eps = 1e-6
        plus = CO._unflat((k, base[k] + eps * dp[k]) for k in base)
        minus = CO._unflat((k, base[k] - eps * dp[k]) for k in base)
        fd = (value(plus, x + eps * dx) - value(minus, x - eps * dx)) / (2 * eps)
        assert abs(an - fd) <= 1e-6 * max(1.0, abs(an)), (trial, an, fd)
