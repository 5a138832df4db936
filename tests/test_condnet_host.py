"""Host side of the conditioning network (zenflow_amd/nn.py, zf_condnet_*):
the oracle of tests/condnet_oracle.py against the notebook's dense
``sum_matrix`` and against central differences, the variable layout of
examples/deep_set.ipynb's ``Phi``, the header against the ctypes mirror, the
host validation of offsets, the dropout rule, and the argument checks that
return before the first HIP call.  No GPU is used."""

import ctypes
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "zenflow_amd.h").read_text()

# jax.tree_map(lambda x: x.shape, best_variables["params"])["phi"], the notebook's last cells
NOTEBOOK_PHI = {
    "BatchNorm_0": {"bias": (2,), "scale": (2,)},
    "NNBlock_0": {
        "Dense_0": {"bias": (128,), "kernel": (2, 128)},
        "Dense_1": {"bias": (128,), "kernel": (128, 128)},
        "Dense_2": {"bias": (128,), "kernel": (128, 128)},
        "Dense_3": {"bias": (8,), "kernel": (128, 8)},
    },
}


def _shapes(tree):
    return {k: _shapes(v) for k, v in tree.items()} if isinstance(tree, dict) else tuple(np.shape(tree))


def _small_case(seed=0, pool="sum", batch_norm=True, dropout=0.3):
    rng = np.random.default_rng(seed)
    cfg = {"layers": [6, 5], "features": 3, "act": "swish", "batch_norm": batch_norm, "dropout": dropout, "pool": pool}
    offsets = np.array([0, 1, 1, 7, 12])
    rows, in_dim = 15, 2  # three trailing rows in no set
    x = rng.standard_normal((rows, in_dim))
    params = {"NNBlock_0": {}}
    w = in_dim
    for l, o in enumerate(cfg["layers"] + [cfg["features"]]):
        params["NNBlock_0"][f"Dense_{l}"] = {"kernel": rng.standard_normal((w, o)) / np.sqrt(w),
                                             "bias": 0.3 * rng.standard_normal(o)}
        w = o
    variables = {"params": params}
    if batch_norm:
        params["BatchNorm_0"] = {"scale": 1 + 0.2 * rng.standard_normal(in_dim), "bias": 0.2 * rng.standard_normal(in_dim)}
        variables["batch_stats"] = {"BatchNorm_0": {"mean": 0.1 * rng.standard_normal(in_dim),
                                                    "var": 1 + 0.2 * rng.random(in_dim)}}
    keep = rng.random((rows, cfg["features"])) >= dropout
    return cfg, variables, x, offsets, keep, rng


def test_oracle_segment_sum_is_the_notebooks_sum_matrix():
    """``segment_sum`` over the row ids equals ``sum_matrix @ h`` with the
    matrix built as the notebook's ``preprocess`` builds it (an empty set and
    trailing padding rows included)."""
    import torch

    from tests import condnet_oracle as CO

    rng = np.random.default_rng(3)
    offsets = np.array([0, 1, 1, 64, 129, 700])
    rows = 720
    h = rng.standard_normal((rows, 5))
    ids = CO.ids_of(offsets, rows)
    assert (ids[700:] == -1).all() and ids[0] == 0 and ids[1] == 2
    got = CO.segment_sum(torch.tensor(h), ids, len(offsets) - 1).numpy()
    want = CO.sum_matrix(offsets, rows).astype(np.float64) @ h
    assert got.shape == want.shape == (5, 5)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(h).sum(axis=0).max()
    assert not got[1].any()  # the empty set


@pytest.mark.parametrize("pool,batch_norm,dropout", [("sum", True, 0.3), (None, True, 0.0), ("sum", False, 0.3)])
def test_oracle_autograd_matches_central_differences(pool, batch_norm, dropout):
    """d / d params of sum(gc * c) from the oracle's float64 autograd against
    central differences along random directions."""
    import torch

    from tests import condnet_oracle as CO

    cfg, variables, x, offsets, keep, rng = _small_case(1, pool, batch_norm, dropout)
    ids = CO.ids_of(offsets, len(x))
    S = len(offsets) - 1
    n_out = S if pool == "sum" else len(x)
    gc = rng.standard_normal((n_out, cfg["features"]))
    job = {"cfg": cfg, "variables": variables, "x": x, "ids": ids, "S": S, "train": True, "mode": "net", "keep": keep,
           "gc": gc}
    res = CO.evaluate(job, torch.float64)
    leaves = dict(CO._flat(res["g"]))
    base = dict(CO._flat(variables["params"]))
    assert leaves.keys() == base.keys()

    def value(params):
        r = CO.evaluate({**job, "gc": None}, torch.float64, variables={**variables, "params": params})
        return float((gc * r["c"]).sum())

    for trial in range(3):
        d = {k: rng.standard_normal(v.shape) for k, v in base.items()}
        an = sum(float((leaves[k] * d[k]).sum()) for k in base)
        eps = 1e-6
        plus = CO._unflat((k, base[k] + eps * d[k]) for k in base)
        minus = CO._unflat((k, base[k] - eps * d[k]) for k in base)
        fd = (value(plus) - value(minus)) / (2 * eps)
        assert abs(an - fd) <= 1e-7 * max(1.0, abs(an)), (trial, an, fd)


def test_oracle_worker_runs_in_a_child_process():
    """``python -m tests.condnet_oracle JOB OUT`` writes the float64 result,
    three float32 row orders and two jittered float64 runs."""
    from tests import condnet_oracle as CO

    cfg, variables, x, offsets, keep, rng = _small_case(2)
    S = len(offsets) - 1
    gc = rng.standard_normal((S, cfg["features"]))
    with tempfile.TemporaryDirectory() as d:
        job, out = Path(d) / "job.npz", Path(d) / "out.npz"
        CO.pack_job(job, cfg, variables, x, CO.ids_of(offsets, len(x)), S, keep=keep, gc=gc)
        subprocess.run([sys.executable, "-m", "tests.condnet_oracle", str(job), str(out)], cwd=ROOT, check=True,
                       timeout=600)
        res = dict(np.load(out))
    assert res["c64"].shape == (S, cfg["features"])
    for r in range(3):
        assert np.abs(res[f"c32_{r}"] - res["c64"]).max() <= 1e-5 * np.abs(res["c64"]).max()
    assert "g64p_1:NNBlock_0/Dense_0/kernel" in res and "stats64:BatchNorm_0/mean" in res


def test_variable_tree_is_the_notebooks():
    """in_dim 2, layers (128,) * 3, features 8: the ``params`` tree printed in
    the notebook's last cells, and BatchNorm's statistics; no BatchNorm entry
    with batch_norm=False; nested as ``phi`` in a DeepSetFlow."""
    import zenflow_amd as zf
    from zenflow_amd import nn

    x = np.zeros((10, 2), np.float32)
    off = np.array([0, 4, 10])
    net = nn.ConditionNet(8, layers=(128,) * 3, dropout=0.3, pool="sum")
    v = net.init(zf.PRNGKey(0), x, off)
    assert _shapes(v["params"]) == NOTEBOOK_PHI
    assert _shapes(v["batch_stats"]) == {"BatchNorm_0": {"mean": (2,), "var": (2,)}}
    bn = v["params"]["BatchNorm_0"]
    assert (bn["scale"] == 1).all() and not bn["bias"].any()
    assert not v["batch_stats"]["BatchNorm_0"]["mean"].any() and (v["batch_stats"]["BatchNorm_0"]["var"] == 1).all()
    from tests.condnet_oracle import _flat

    assert all(a.dtype == np.float32 for _, a in _flat(v))
    k = v["params"]["NNBlock_0"]["Dense_1"]["kernel"]
    assert 0.5 / 128 < k.var() < 2.0 / 128  # lecun_normal
    v2 = nn.ConditionNet(8, layers=(128,) * 3, batch_norm=False).init(0, x)
    assert "batch_stats" not in v2 and "BatchNorm_0" not in v2["params"]
    assert _shapes(v2["params"]["NNBlock_0"]) == NOTEBOOK_PHI["NNBlock_0"]

    from zenflow_amd.bijectors import rolling_spline_coupling

    class DeepSetFlow(zf.Module):
        def setup(self):
            self.phi = nn.ConditionNet(8, layers=(128,) * 3, dropout=0.3, pool="sum")
            self.flow = zf.Flow(rolling_spline_coupling(2, layers=(32, 32)))

        def __call__(self, x, offsets, y, train: bool = False):
            return self.flow(y, self.phi(x, offsets, train=train), train=train)

    vv = DeepSetFlow().init(zf.PRNGKey(1), x, off, np.zeros((2, 2), np.float32))
    assert _shapes(vv["params"]["phi"]) == NOTEBOOK_PHI
    assert set(vv["batch_stats"]) == {"phi", "flow"}
    # the flow's first BatchNorm sees D - D // 2 + features = 9 inputs, as in the notebook's tree
    first = sorted(k for k in vv["params"]["flow"]["bijector"] if "BatchNorm_0" in vv["params"]["flow"]["bijector"][k])[0]
    assert vv["params"]["flow"]["bijector"][first]["BatchNorm_0"]["scale"].shape == (9,)


def test_blob_layout_round_trip():
    from zenflow_amd import nn

    net = nn.ConditionNet(3, layers=(6, 5), pool="sum")
    v = net.init(4, np.zeros((4, 2), np.float32), np.array([0, 4]))
    lay = net._layout(2)
    d = lay.desc
    assert d.off_bn == 0 and d.off_w[0] == 8 and d.off_b[0] == 20 and d.off_w[1] == 28
    assert all(int(d.off_w[l]) % 4 == 0 and int(d.off_b[l]) % 4 == 0 for l in range(3))
    blob = lay.to_blob(v)
    back = lay.to_tree(blob)
    from tests.condnet_oracle import _flat

    assert dict((k, a.tobytes()) for k, a in _flat(back)) == dict((k, np.asarray(a, np.float32).tobytes())
                                                                  for k, a in _flat(v))
    n_params = sum(a.size for _, a in _flat(v["params"]))
    assert lay.param_mask.sum() == n_params and lay.param_mask[:4].sum() == 0  # mean, var: statistics


def test_header_constants_and_struct_layout_match_lib():
    from zenflow_amd import _lib as L

    defs = dict(re.findall(r"^#define (ZF_[A-Z0-9_]+)\s+((?:0x[0-9a-fA-F]+|-?\d+))u?\b", HEADER, re.M))
    for name in ("ZF_SEG_CHUNK", "ZF_DROPOUT_STREAM", "ZF_DROPOUT_WORD", "ZF_POOL_NONE", "ZF_POOL_SUM"):
        assert int(defs[name], 0) == getattr(L, name), name
    # zf_condnet_desc: 24 int32-sized fields (in_dim, n_hidden, hidden[16], out_dim, act, batch_norm, pool, dropout,
    # _pad), then off_bn, off_w[17], off_b[17]
    assert ctypes.sizeof(L.ZfCondnetDesc) == 4 * 24 + 8 * 35
    assert L.ZfCondnetDesc.out_dim.offset == 4 * 18 and L.ZfCondnetDesc.dropout.offset == 4 * 22
    assert L.ZfCondnetDesc.off_bn.offset == 96 and L.ZfCondnetDesc.off_b.offset == 96 + 8 * 18
    fields = re.search(r"typedef struct zf_condnet_desc \{(.*?)\} zf_condnet_desc;", HEADER, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"\b([a-z_]+)(?:\[\d+\])?(?:,\s*([a-z_]+)\[\d+\])?;", fields)
    flat = [n for pair in names for n in pair if n]
    assert flat == [f[0] for f in L.ZfCondnetDesc._fields_]
    for fn in ("zf_segment_sum", "zf_segment_bcast", "zf_condnet_forward", "zf_condnet_backward"):
        assert fn in L.SIGNATURES


@pytest.mark.parametrize("offsets", [[0, 5, 3, 8], [-1, 2, 8], [0, 4, 11], [0, 4, 2]])
def test_host_offsets_are_validated(offsets):
    """Decreasing, negative and past ``rows`` each raise ValueError, from
    check_offsets and from the module's call before it touches a device."""
    from zenflow_amd import nn

    with pytest.raises(ValueError):
        nn.check_offsets(offsets, 10)
    net = nn.ConditionNet(3, layers=(4,), pool="sum")
    x = np.zeros((10, 2), np.float32)
    v = net.init(0, x, np.array([0, 10]))
    with pytest.raises(ValueError):
        net.apply(v, x, np.asarray(offsets))


def test_offsets_helpers():
    from zenflow_amd import nn

    assert nn.check_offsets([0, 0, 3, 10], 10).dtype == np.int64
    assert nn.clamp_offsets([3, -2, 5, 4, 99], 10).tolist() == [3, 3, 5, 5, 10]
    with pytest.raises(ValueError):
        nn.ConditionNet(3, pool=None).apply({}, np.zeros((4, 2), np.float32), np.array([0, 4]))
    with pytest.raises(ValueError):
        nn.check_offsets([0], 10)


@pytest.mark.parametrize("rate", [0.3, 0.5])
def test_dropout_rule_keeps_the_right_share(rate):
    """The rule of include/zenflow_amd.h restated with
    tests/sampler_oracle.py's philox_at / u01_co: zenflow_amd.nn.dropout_keep
    has the same bits, and on 2^16 draws the kept share is within five
    binomial standard deviations of 1 - rate."""
    from tests import sampler_oracle as SO
    from zenflow_amd import _lib as L
    from zenflow_amd import nn

    rows, F, seed = 1 << 13, 8, 20250307
    r = np.arange(rows, dtype=np.int64)
    keep = np.stack([SO.u01_co(SO.philox_at(seed, r, f, L.ZF_DROPOUT_STREAM)[..., L.ZF_DROPOUT_WORD])
                     >= np.float32(rate) for f in range(F)], axis=1)
    assert keep.shape == (rows, F) and keep.size == 1 << 16
    assert np.array_equal(keep, nn.dropout_keep(seed, rows, F, rate))
    n = keep.size
    assert abs(keep.mean() - (1 - rate)) <= 5 * np.sqrt(rate * (1 - rate) / n)
    other = nn.dropout_keep(seed + 1, rows, F, rate)
    assert 0.3 < (other != keep).mean() < 0.7  # another seed, another mask
    # a row index array addresses the same draws
    assert np.array_equal(nn.dropout_keep(seed, np.array([5, 9000 - 1000]), F, rate), keep[[5, 8000]])


def test_constructor_rejections():
    from zenflow_amd import nn

    with pytest.raises(NotImplementedError):
        nn.ConditionNet(8, layers=(5000,))
    with pytest.raises(NotImplementedError):
        nn.ConditionNet(8, layers=(8,) * 17)
    with pytest.raises(NotImplementedError):
        nn.ConditionNet(65)
    with pytest.raises(NotImplementedError):
        nn.ConditionNet(8, pool="mean")
    with pytest.raises(ValueError):
        nn.ConditionNet(8, dropout=1.0)
    with pytest.raises(NotImplementedError):
        nn.ConditionNet(8, layers=(4,)).init(0, np.zeros((3, 65), np.float32))


def _desc(**kw):
    from zenflow_amd import _lib as L

    d = L.ZfCondnetDesc()
    d.in_dim, d.out_dim, d.n_hidden = 2, 8, 1
    d.hidden[0] = 16
    for k, v in kw.items():
        if k == "hidden0":
            d.hidden[0] = v
        else:
            setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,rc", [
    (dict(in_dim=65), -2), (dict(in_dim=0), -1), (dict(out_dim=65), -2), (dict(out_dim=0), -1),
    (dict(hidden0=4097), -2), (dict(hidden0=0), -1), (dict(n_hidden=17), -2), (dict(n_hidden=-1), -1),
    (dict(act=8), -1), (dict(pool=2), -1), (dict(dropout=1.0), -1), (dict(dropout=-0.1), -1),
])
def test_condnet_plan_rejects(kw, rc):
    from zenflow_amd import _lib as L

    n = ctypes.c_int64()
    lib = L.load_library()
    assert lib.zf_condnet_plan(ctypes.byref(_desc(**kw)), ctypes.byref(n)) == rc
    assert lib.zf_last_error()


@pytest.mark.parametrize("rows,F,S,rate,null,rc", [
    (8, 65, 2, 0.0, None, -2), (8, 0, 2, 0.0, None, -1), (8, 3, -1, 0.0, None, -1), (-1, 3, 2, 0.0, None, -1),
    (8, 3, 2, 1.0, None, -1), (8, 3, (1 << 24) + 1, 0.0, None, -2), (1 << 31, 3, 2, 0.0, None, -2),
    (8, 3, 2, 0.0, "h", -1), (8, 3, 2, 0.0, "off", -1), (8, 3, 2, 0.0, "out", -1), (8, 3, 2, 0.0, "ws", -1),
])
def test_segment_entries_reject_before_any_launch(rows, F, S, rate, null, rc):
    """Every check returns before the first HIP call, so host pointers stand
    in for device ones (as tests/test_abi.py does for the other standalone
    entries)."""
    from zenflow_amd import _lib as L

    lib = L.load_library()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    a = {k: (None if null == k else p) for k in ("h", "off", "out", "ws")}
    assert lib.zf_segment_sum(a["h"], rows, F, a["off"], S, rate, 0, a["out"], None, a["ws"], None) == rc
    assert lib.zf_last_error()
    if null in (None, "h", "off", "out"):
        assert lib.zf_segment_bcast(a["h"], a["off"], rows, F, S, rate, 0, a["out"], None) == rc
    # 50,000 rows: two levels (512^2 >= rows), each with o[S + 1] and cb[S + 1]; the first level's chunk sums
    assert lib.zf_segment_workspace_bytes(50_000, 1000, 8) == 2 * 2 * 1001 * 8 + (50_000 // 512 + 1001) * 8 * 4
    assert lib.zf_segment_workspace_bytes(512, 1000, 8) == 2 * 1001 * 8  # one level: no intermediate sums


def test_package_exports():
    import zenflow_amd as zf

    assert zf.ConditionNet is zf.nn.ConditionNet and zf.ConditionTrainer is zf.nn.ConditionTrainer
    assert "zf_condnet.hip" in __import__("zenflow_amd.build").build.SOURCES
