"""Host side of the input gradient, the stacked networks and the segment
repeat (zenflow_amd/nn.py, zf_condnet_backward_input, zf_segment_repeat): the
oracle of tests/deepset_oracle.py against central differences, the argument
checks that return before the first HIP call, the header against the ctypes
mirror, and the conversion of ``repeats`` to offsets.  No GPU is used."""

import re
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

from tests.test_condnet_host import _small_case

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "zenflow_amd.h").read_text()


def _rho_case(in_dim, rng, batch_norm=False):
    cfg = {"layers": [5, 4], "features": 1, "act": "swish", "batch_norm": batch_norm, "dropout": 0.0, "pool": None}
    params = {"NNBlock_0": {}}
    w = in_dim
    for l, o in enumerate(cfg["layers"] + [cfg["features"]]):
        params["NNBlock_0"][f"Dense_{l}"] = {"kernel": rng.standard_normal((w, o)) / np.sqrt(w),
                                             "bias": 0.3 * rng.standard_normal(o)}
        w = o
    return cfg, {"params": params}


def _directional(job, res, rng, names):
    """sum over the differentiated inputs of <gradient, direction> against the
    central difference of the oracle's value along three random directions."""
    import torch

    from tests import condnet_oracle as CO
    from tests import deepset_oracle as DO

    base = {"x": {"x": np.asarray(job["x"], np.float64)}, "g": dict(CO._flat(job["variables"]["params"]))}
    grads = {"x": {"x": res["gx"]}, "g": dict(CO._flat(res["g"]))}
    if "rg" in names:
        base["rg"] = dict(CO._flat(job["rvariables"]["params"]))
        grads["rg"] = dict(CO._flat(res["rg"]))
    for n in names:
        assert grads[n].keys() == base[n].keys()

    def value(sign, d, eps):
        at = {n: {k: base[n][k] + sign * eps * d[n][k] for k in base[n]} for n in base}
        kw = {"x": at["x"]["x"], "variables": {**job["variables"], "params": CO._unflat(at["g"].items())}}
        if "rg" in at:
            kw["rvariables"] = {**job["rvariables"], "params": CO._unflat(at["rg"].items())}
        return DO.evaluate(job, torch.float64, **kw)["value"]

    for trial in range(3):
        d = {n: {k: (rng.standard_normal(v.shape) if n in names else np.zeros(v.shape)) for k, v in base[n].items()}
             for n in base}
        an = sum(float((grads[n][k] * d[n][k]).sum()) for n in names for k in base[n])
        eps = 1e-6
        fd = (value(+1, d, eps) - value(-1, d, eps)) / (2 * eps)
        assert abs(an - fd) <= 1e-7 * max(1.0, abs(an)), (names, trial, an, fd)


@pytest.mark.parametrize("pool,batch_norm,dropout", [("sum", True, 0.3), (None, True, 0.0), ("sum", False, 0.3),
                                                     (None, False, 0.3)])
def test_oracle_input_gradient_matches_central_differences(pool, batch_norm, dropout):
    """d / d x of sum(gc * c) from float64 autograd against central
    differences, alone and together with the parameters.  The small case has
    three trailing padding rows, which are in BatchNorm's statistics: with
    BatchNorm their gx is not zero (the batch terms), without it and pooled it
    is."""
    import torch

    from tests import condnet_oracle as CO
    from tests import deepset_oracle as DO

    cfg, variables, x, offsets, keep, rng = _small_case(11, pool, batch_norm, dropout)
    S = len(offsets) - 1
    gc = rng.standard_normal((S if pool == "sum" else len(x), cfg["features"]))
    job = {"cfg": cfg, "variables": variables, "x": x, "ids": CO.ids_of(offsets, len(x)), "S": S, "mode": "net",
           "keep": keep, "gc": gc}
    res = DO.evaluate(job, torch.float64)
    assert res["gx"].shape == x.shape
    _directional(job, res, rng, ["x"])
    _directional(job, res, rng, ["x", "g"])
    pad = res["gx"][offsets[-1]:]
    if pool == "sum":
        assert pad.any() == batch_norm
    # the parameter gradients are condnet_oracle's
    ref = CO.evaluate({**job, "train": True}, torch.float64)["g"]
    assert all(np.array_equal(a, dict(CO._flat(res["g"]))[k]) for k, a in CO._flat(ref))
    # a permutation of the rows going in comes back out
    perm = np.random.default_rng(5).permutation(len(x))
    again = DO.evaluate(job, torch.float64, perm=perm)
    assert np.abs(again["gx"] - res["gx"]).max() <= 1e-12 * np.abs(res["gx"]).max()
    assert np.abs(again["c"] - res["c"]).max() <= 1e-12 * np.abs(res["c"]).max()


@pytest.mark.parametrize("rho_batch_norm", [False, True])
def test_oracle_stack_matches_central_differences(rho_batch_norm):
    """phi (BatchNorm, dropout, sum; padding rows present) -> rho: the
    gradients of sum(gy * rho(phi(x))) with respect to x and to both networks'
    parameters against central differences."""
    import torch

    from tests import condnet_oracle as CO
    from tests import deepset_oracle as DO

    cfg, variables, x, offsets, keep, rng = _small_case(12, "sum", True, 0.3)
    S = len(offsets) - 1
    rcfg, rvariables = _rho_case(cfg["features"], rng, rho_batch_norm)
    if rho_batch_norm:
        rvariables["params"]["BatchNorm_0"] = {"scale": 1 + 0.2 * rng.standard_normal(3), "bias": 0.2 * rng.standard_normal(3)}
        rvariables["batch_stats"] = {"BatchNorm_0": {"mean": np.zeros(3), "var": np.ones(3)}}
    gy = rng.standard_normal((S, 1))
    job = {"cfg": cfg, "variables": variables, "x": x, "ids": CO.ids_of(offsets, len(x)), "S": S, "mode": "stack",
           "keep": keep, "rcfg": rcfg, "rvariables": rvariables, "gy": gy}
    res = DO.evaluate(job, torch.float64)
    assert res["y"].shape == (S, 1) and res["c"].shape == (S, cfg["features"])
    for names in (["x"], ["g"], ["rg"], ["x", "g", "rg"]):
        _directional(job, res, rng, names)
    assert res["gx"][offsets[-1]:].any()  # phi's BatchNorm: the padding rows carry the batch terms


def test_oracle_worker_runs_in_a_child_process():
    """``python -m tests.deepset_oracle JOB OUT`` writes the float64 result,
    three float32 row orders and two jittered float64 runs under the keys
    tests/test_gpu_condnet.py::_check reads."""
    from tests import condnet_oracle as CO
    from tests import deepset_oracle as DO

    cfg, variables, x, offsets, keep, rng = _small_case(13)
    S = len(offsets) - 1
    rcfg, rvariables = _rho_case(cfg["features"], rng)
    gy = rng.standard_normal((S, 1))
    with tempfile.TemporaryDirectory() as d:
        job, out = Path(d) / "job.npz", Path(d) / "out.npz"
        DO.pack_job(job, cfg, variables, x, CO.ids_of(offsets, len(x)), S, mode="stack", rcfg=rcfg,
                    rvariables=rvariables, keep=keep, gy=gy)
        subprocess.run([sys.executable, "-m", "tests.deepset_oracle", str(job), str(out)], cwd=ROOT, check=True,
                       timeout=600)
        res = dict(np.load(out))
    assert res["gx64"].shape == x.shape and res["y64"].shape == (S, 1)
    for r in range(3):
        assert f"gx32_{r}" in res and np.abs(res[f"gx32_{r}"] - res["gx64"]).max() <= 1e-4 * np.abs(res["gx64"]).max()
    for key in ("gx64p_1", "g64:NNBlock_0/Dense_0/kernel", "g32_2:BatchNorm_0/scale", "rg64:NNBlock_0/Dense_2/bias",
                "rg64p_0:NNBlock_0/Dense_0/kernel", "c64", "y32_1"):
        assert key in res, key


@pytest.mark.parametrize("F,S,rows,null,rc", [
    (65, 2, 8, None, -2), (0, 2, 8, None, -1), (3, -1, 8, None, -1), (3, 2, -1, None, -1),
    (3, (1 << 24) + 1, 8, None, -2), (3, 2, 1 << 31, None, -2),
    (3, 2, 8, "c", -1), (3, 2, 8, "off", -1), (3, 2, 8, "out", -1), (3, 2, 8, "ws", -1),
])
def test_segment_repeat_rejects_before_any_launch(F, S, rows, null, rc):
    """Every check returns before the first HIP call, so host pointers stand in
    for device ones (tests/test_condnet_host.py::
    test_segment_entries_reject_before_any_launch); the limits and codes are
    zf_segment_sum's."""
    from zenflow_amd import _lib as L

    lib = L.load_library()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    a = {k: (None if null == k else p) for k in ("c", "off", "out", "ws")}
    assert lib.zf_segment_repeat(a["c"], S, F, a["off"], rows, a["out"], None, a["ws"], None) == rc
    assert lib.zf_last_error()
    # a set_index changes no check
    assert lib.zf_segment_repeat(a["c"], S, F, a["off"], rows, a["out"], p, a["ws"], None) == rc


def test_new_entries_are_in_header_library_and_signatures():
    from zenflow_amd import _lib as L

    lib = L.load_library()
    for fn, nargs in (("zf_condnet_backward_input", 5), ("zf_segment_repeat", 9)):
        m = re.search(r"^int " + fn + r"\((.*?)\);", HEADER, re.M | re.S)
        assert m, fn
        assert len(m.group(1).split(",")) == nargs
        assert fn in L.SIGNATURES and len(L.SIGNATURES[fn][1]) == nargs
        assert getattr(lib, fn).argtypes is not None and len(getattr(lib, fn).argtypes) == nargs
    # each names the reference callable it replaces, and the repeat its reverse
    assert "jnp.repeat(c, sizes, axis=0)" in HEADER and "class DeepSet" in HEADER
    rep = HEADER[HEADER.index("Repeat over ragged sets"):HEADER.index("int zf_segment_repeat")]
    assert "reverse" in rep and "zf_segment_sum" in rep
    # a NULL handle is rejected by both reverse entries alike
    assert lib.zf_condnet_backward_input(None, None, None, None, None) == -1
    assert lib.zf_condnet_backward(None, None, None, None) == -1


def test_repeats_become_offsets():
    from zenflow_amd import nn

    assert nn.repeats_to_offsets(3, 4).tolist() == [0, 3, 6, 9, 12]
    assert nn.repeats_to_offsets(0, 2).tolist() == [0, 0, 0]
    assert nn.repeats_to_offsets([2, 0, 0, 5, 1], 5).tolist() == [0, 2, 2, 2, 7, 8]
    assert nn.repeats_to_offsets(np.array([2.0, 1.0]), 2).dtype == np.int64
    for r, rows in (([2, 0, 3], 3), (5, 3)):  # np.repeat's own result
        off = nn.repeats_to_offsets(r, rows)
        ids = np.repeat(np.arange(rows), r)
        assert off[-1] == len(ids) and all((ids[off[s]:off[s + 1]] == s).all() for s in range(rows))
    for bad in ([1, 2], [1, -1, 2], [[1, 2, 3]], [1.5, 1, 1]):
        with pytest.raises(ValueError):
            nn.repeats_to_offsets(bad, 3)
    with pytest.raises(ValueError):
        nn.repeats_to_offsets(-1, 3)
    c = np.zeros((3, 2), np.float32)
    # both given, neither given, too few rows, a wrong number of offsets: before any device is touched
    with pytest.raises(ValueError, match="not both"):
        nn.segment_repeat(c, [0, 1, 2, 3], repeats=2)
    with pytest.raises(ValueError):
        nn.segment_repeat(c)
    with pytest.raises(ValueError):
        nn.segment_repeat(c, repeats=[1, 2, 3], rows=5)
    with pytest.raises(ValueError):
        nn.segment_repeat(c, [0, 1, 2])
    with pytest.raises(ValueError):
        nn.segment_repeat(c, [0, 2, 1, 3])
    with pytest.raises(ValueError):
        nn.segment_sum(c, [0, 2, 4])
    assert "segment_repeat" in nn.__all__ and "segment_sum" in nn.__all__
