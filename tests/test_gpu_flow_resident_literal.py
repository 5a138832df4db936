"""The literal coupling body of the resident form's specialised frame
(x3_nsc LIT): the frame's couplings are compiled for the
flagship shape alone and take their remaining constants once per pass, so the
frame is open only to flows whose couplings all have exactly the kernel's
K = 16 knots.  Against the streaming form on the same inputs every output must
have the same bits — log_prob, the fp64 NLL sum, the forward y / log_det, the
inverse x and a seeded sample — NaN positions included.  One program is bound
with ZF_X3_RESIDENT=0 and one with =1, as tests/test_gpu_flow_resident_frame.py
does.  Needs the GPU.

Flows and the form each must take (asserted through the launch counters):
cfg2's shape and `both4` (four two-sided dims) run the specialised frame; a
D = 4 flow with one padded knot (K = 15: the sliver starts at the padded knot),
one with inert padded knots (K = 12) and a chain that mixes knot counts
(16, 12, 15, 16) run the resident form, but not the frame: its generic frame
keeps the per-coupling knot count, the padded-knot sliver and the runtime
layer loops, and like the specialised one takes the knot constants stored with
the flow at the pass head.

Row counts: 1 (a single row), 129 (a second NLL slot with one row), 4097,
128 * CUs + 33 (most blocks hold one slot; a wave has at most one tile per
pass) and 128 * CUs * 4 + 33 (16-17 tiles per block: some waves take a second
tile, so the prefetch and the constants carried through the pass meet a second
iteration).

Inputs carry NaN rows and rows far outside the stored range, as the frame test's."""

import functools

import numpy as np
import pytest

from tests.flowcases import build_flow, chain_spec, make_variables

pytestmark = pytest.mark.gpu

FMIN = np.float32(np.finfo(np.float32).min)
BASE = dict(D=4, C=0, K=16, layers=(128, 128), latent="normal")
CFGS = {
    "cfg2": dict(BASE),
    "both4": dict(BASE, bounds=((0, -1.0, 1.0), (1, -2.0, 3.0), (2, 0.0, 1.0), (3, -0.5, 0.25))),
    "k15": dict(BASE, K=15),
    "k12": dict(BASE, K=12),
    "kmix": dict(BASE, K=(16, 12, 15, 16)),
}
FORM = {"cfg2": "resident_frame", "both4": "resident_frame", "k15": "resident", "k12": "resident", "kmix": "resident"}


def _cus():
    try:
        import torch

        return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        return 256


def _row_counts():
    return [1, 129, 4097, 128 * _cus() + 33, 128 * _cus() * 4 + 33]


def _draw(cfg, rng, n):
    x = rng.standard_normal((n, cfg["D"])).astype(np.float32)
    for d, a, b in cfg.get("bounds", ()):
        u = 0.5 + 0.5 * np.tanh(x[:, d])
        u[5::13] = 1.2
        u[9::13] = -0.3
        x[:, d] = (a + (b - a) * u).astype(np.float32)
    return x


def _spoil(x):
    """NaN inputs and rows far outside the stored range, among the first 129 rows and throughout."""
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
def _case(name):
    """One seeded case per flow at the largest N; the smaller batches are its leading rows."""
    from oracle import zf_oracle as O

    cfg = dict(CFGS[name])
    n = max(_row_counts())
    rng = np.random.default_rng(181)
    spec, variables = make_variables(cfg, rng)
    assert spec == chain_spec(cfg)
    _, _, sb = O.shift_bounds_forward(spec["bijectors"][0], {}, _draw(cfg, rng, 4096), train=True)
    variables["batch_stats"]["bijector"]["bijectors_0"] = {k: np.asarray(v, np.float32) for k, v in sb.items()}
    x = _spoil(_draw(cfg, rng, n))
    z = _spoil((0.5 + 0.1 * rng.standard_normal(x.shape)).astype(np.float32))
    return {"cfg": cfg, "variables": variables, "x": x, "z": z, "name": name}


def _bind(case, monkeypatch, mode):
    """A freshly built flow (its own program cache) bound with ZF_X3_RESIDENT=mode."""
    monkeypatch.setenv("ZF_X3_RESIDENT", mode)
    flow = build_flow(case["cfg"])
    bf = flow.bind(case["variables"], case["cfg"]["D"], case["cfg"]["C"])
    assert bf.program.kernel_variant == "f16x2"
    return bf


def _dev(a, n):
    from zenflow_amd._lib import DeviceArray

    return DeviceArray.from_numpy(np.ascontiguousarray(a[:n]))


def _log_prob(bf, case, n):
    from zenflow_amd._lib import DeviceArray

    nll = DeviceArray((1,), np.float64)
    lp = bf.log_prob(_dev(case["x"], n), None, nll_sum=nll).numpy()
    return lp, nll.numpy().copy()


def _same_bits(a, b, what):
    """The same bits wherever a is a number (signed zeros included), and NaN in the same places."""
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN positions"
    num = ~np.isnan(a)
    ua, ub = a[num].view(np.uint8), b[num].view(np.uint8)
    assert np.array_equal(ua, ub), f"{what}: {int(np.sum(a[num] != b[num]))} values differ"


def _check_forms(name, stream, res):
    """The streaming program never left the streaming form; the resident one took the form it must."""
    other = "resident" if FORM[name] == "resident_frame" else "resident_frame"
    assert stream.program.launch_count("resident") == 0 and stream.program.launch_count("resident_frame") == 0
    assert stream.program.launch_count("streaming") > 0
    assert res.program.launch_count(FORM[name]) > 0, f"{name}: no launch on the {FORM[name]} form"
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
        if n == 129:
            # the inputs do what they are there for, on the streaming form itself
            assert np.isnan(case["x"][:129]).any(axis=1).sum() >= 2
            assert (lp0 == FMIN).sum() >= 1, "no finite-minimum row among the first 129"
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
        y0, ld0 = stream.forward(_dev(case["x"], n), None)
        y1, ld1 = res.forward(_dev(case["x"], n), None)
        _same_bits(y1.numpy(), y0.numpy(), f"{name}/N={n} y")
        _same_bits(ld1.numpy(), ld0.numpy(), f"{name}/N={n} log_det")
    _check_forms(name, stream, res)


@pytest.mark.parametrize("name", list(CFGS))
def test_inverse_and_sample_bits(name, monkeypatch):
    case = _case(name)
    stream = _bind(case, monkeypatch, "0")
    res = _bind(case, monkeypatch, "1")
    for n in _row_counts():
        x0 = stream.inverse(_dev(case["z"], n), None).numpy()
        x1 = res.inverse(_dev(case["z"], n), None).numpy()
        _same_bits(x1, x0, f"{name}/N={n} inverse")
        s0 = stream.program.sample(n, 1234, None).numpy()
        s1 = res.program.sample(n, 1234, None).numpy()
        _same_bits(s1, s0, f"{name}/N={n} sample")
    _check_forms(name, stream, res)
