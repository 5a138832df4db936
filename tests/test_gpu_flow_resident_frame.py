"""The resident form's specialised frame (flow_kernel_x3r FR)
against the streaming form on the same inputs: every
output must have the same bits — log_prob, the fp64 NLL sum, the forward y /
log_det, the inverse x and a seeded sample — NaN positions included.  One
program is bound with ZF_X3_RESIDENT=0 (never the resident form) and one with
=1 (the resident form whenever the call is eligible).  Needs the GPU.

Flows: cfg2 (every ShiftBounds row of mode NONE) must take the specialised
frame, and so must its two neighbours with two-sided bounds, whose rows of
mode BOTH have constants and a no-clip path of their own in the frame: one
two-sided dim among unbounded ones, and all four dims two-sided with four
different intervals (asserted through the handle's launch counters).  Four
neighbours must stay on the generic frame — one log-mode ShiftBounds row, a
truncated-normal latent, one condition, D = 5.

Row counts: those of test_gpu_flow_resident.py, for its reasons, and
128 * CUs * 4 + 33 (16-17 tiles per block: some waves of a block take a second
tile and some do not).

Inputs carry rows with NaN in x and rows far outside the ShiftBounds range, so
the clip, nan_to_num and a -3.4e38 term of the fp64 sum are on the tested path;
a two-sided dim is drawn inside (a, b) with every 13th row a little below a and
every 13th a little above b."""

import functools

import numpy as np
import pytest

from tests.flowcases import build_flow, chain_spec, make_variables

pytestmark = pytest.mark.gpu

FMIN = np.float32(np.finfo(np.float32).min)
BASE = dict(D=4, C=0, K=16, layers=(128, 128), latent="normal")
CFGS = {
    "cfg2": dict(BASE),
    "both1": dict(BASE, bounds=((2, -1.0, 1.0),)),
    "both4": dict(BASE, bounds=((0, -1.0, 1.0), (1, -2.0, 3.0), (2, 0.0, 1.0), (3, -0.5, 0.25))),
    "logbound": dict(BASE, bounds=((0, 0.0, None),)),
    "truncnorm": dict(BASE, latent="truncated_normal"),
    "c1": dict(BASE, C=1),
    "d5": dict(BASE, D=5),
}
FRAME = {"cfg2": "resident_frame", "both1": "resident_frame", "both4": "resident_frame", "logbound": "resident", "truncnorm": "resident", "c1": "resident", "d5": "resident"}


def _cus():
    try:
        import torch

        return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        return 256


def _row_counts():
    return [1, 100, 129, 4097, 128 * _cus() + 33, 50000, 128 * _cus() * 4 + 33]


def _draw(cfg, rng, n):
    x = rng.standard_normal((n, cfg["D"])).astype(np.float32)
    for d, a, b in cfg.get("bounds", ()):
        if b is None:
            x[:, d] = a + np.exp(x[:, d])
        elif a is not None:
            u = 0.5 + 0.5 * np.tanh(x[:, d])
            u[5::13] = 1.2
            u[9::13] = -0.3
            x[:, d] = (a + (b - a) * u).astype(np.float32)
    return x


def _spoil(x):
    """NaN inputs and rows far outside the stored range, among the first 100 rows and throughout."""
    D = x.shape[1]
    for r0 in range(0, x.shape[0], 997):
        for k, (dr, v) in enumerate([(3, np.nan), (7, 1e6), (11, -1e6), (69, np.nan), (70, 3e38)]):
            if r0 + dr < x.shape[0]:
                if k % 2:
                    x[r0 + dr, :] = v
                else:
                    x[r0 + dr, (r0 + k) % D] = v
    return x


@functools.lru_cache(maxsize=None)
def _case(name, n=None):
    """One seeded case per flow at the largest N; the smaller batches are its leading rows."""
    from oracle import zf_oracle as O

    cfg = dict(CFGS[name])
    n = n or max(_row_counts())
    rng = np.random.default_rng(171)
    spec, variables = make_variables(cfg, rng)
    assert spec == chain_spec(cfg)
    _, _, sb = O.shift_bounds_forward(spec["bijectors"][0], {}, _draw(cfg, rng, 4096), train=True)
    variables["batch_stats"]["bijector"]["bijectors_0"] = {k: np.asarray(v, np.float32) for k, v in sb.items()}
    x = _spoil(_draw(cfg, rng, n))
    c = rng.standard_normal((n, cfg["C"])).astype(np.float32) if cfg["C"] else None
    return {"cfg": cfg, "variables": variables, "x": x, "c": c, "name": name}


def _bind(case, monkeypatch, mode):
    """A freshly built flow (its own program cache) bound with ZF_X3_RESIDENT=mode."""
    monkeypatch.setenv("ZF_X3_RESIDENT", mode)
    flow = build_flow(case["cfg"])
    bf = flow.bind(case["variables"], case["cfg"]["D"], case["cfg"]["C"])
    assert bf.program.kernel_variant == "f16x2"
    return bf


def _dev(a, n):
    from zenflow_amd._lib import DeviceArray

    return None if a is None else DeviceArray.from_numpy(np.ascontiguousarray(a[:n]))


def _log_prob(bf, case, n):
    from zenflow_amd._lib import DeviceArray

    nll = DeviceArray((1,), np.float64)
    lp = bf.log_prob(_dev(case["x"], n), _dev(case["c"], n), nll_sum=nll).numpy()
    return lp, nll.numpy().copy()


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert np.array_equal(a, b, equal_nan=True), f"{what}: {np.sum(~((a == b) | (np.isnan(a) & np.isnan(b))))} differ"
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN positions"


def _check_forms(name, stream, res):
    """The streaming program never left the streaming form; the resident one took the frame it must."""
    other = "resident" if FRAME[name] == "resident_frame" else "resident_frame"
    assert stream.program.launch_count("resident") == 0 and stream.program.launch_count("resident_frame") == 0
    assert stream.program.launch_count("streaming") > 0
    assert res.program.launch_count(FRAME[name]) > 0, f"{name}: no launch on the {FRAME[name]} form"
    assert res.program.launch_count(other) == 0, f"{name}: launches on the {other} form"
    assert res.program.launch_count("streaming") == 0


@pytest.mark.parametrize("name", list(CFGS))
def test_log_prob_and_nll_bits(name, monkeypatch):
    case = _case(name)
    stream = _bind(case, monkeypatch, "0")
    res = _bind(case, monkeypatch, "1")
    for n in _row_counts():
        lp0, nll0 = _log_prob(stream, case, n)
        lp1, nll1 = _log_prob(res, case, n)
        if n == 100:
            # the inputs do what they are there for, on the streaming form itself
            assert np.isnan(case["x"][:100]).any(axis=1).sum() >= 1
            assert (lp0 == FMIN).sum() >= 1, "no finite-minimum row among the first 100"
            assert np.isfinite(lp0).all()
        _same_bits(lp1, lp0, f"{name}/N={n} log_prob")
        _same_bits(nll1, nll0, f"{name}/N={n} nll")
    _check_forms(name, stream, res)


@pytest.mark.parametrize("name", list(CFGS))
def test_forward_bits(name, monkeypatch):
    case = _case(name)
    stream = _bind(case, monkeypatch, "0")
    res = _bind(case, monkeypatch, "1")
    for n in _row_counts():
        y0, ld0 = stream.forward(_dev(case["x"], n), _dev(case["c"], n))
        y1, ld1 = res.forward(_dev(case["x"], n), _dev(case["c"], n))
        _same_bits(y1.numpy(), y0.numpy(), f"{name}/N={n} y")
        _same_bits(ld1.numpy(), ld0.numpy(), f"{name}/N={n} log_det")
    _check_forms(name, stream, res)


@pytest.mark.parametrize("name", list(CFGS))
def test_inverse_and_sample_bits(name, monkeypatch):
    case = _case(name)
    stream = _bind(case, monkeypatch, "0")
    res = _bind(case, monkeypatch, "1")
    rng = np.random.default_rng(172)
    z = _spoil((0.5 + 0.1 * rng.standard_normal(case["x"].shape)).astype(np.float32))
    for n in _row_counts():
        x0 = stream.inverse(_dev(z, n), _dev(case["c"], n)).numpy()
        x1 = res.inverse(_dev(z, n), _dev(case["c"], n)).numpy()
        _same_bits(x1, x0, f"{name}/N={n} inverse")
        s0 = stream.program.sample(n, 1234, _dev(case["c"], n)).numpy()
        s1 = res.program.sample(n, 1234, _dev(case["c"], n)).numpy()
        _same_bits(s1, s0, f"{name}/N={n} sample")
    _check_forms(name, stream, res)
