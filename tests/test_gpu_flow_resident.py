"""Resident form of the f16x2 split-MFMA flow kernel (flow_kernel_x3r,
DESIGN.md §2 K3) against the streaming form on the same inputs: every output
must have the same bits — log_prob, the fp64 NLL sum, the forward y / log_det,
the inverse x and a seeded sample — NaN positions included.  One program is
built with ZF_X3_RESIDENT=0 (never the resident form) and one with =1 (the
resident form whenever the call is eligible, whatever N is); a flow, or a
direction, the resident form is not enabled for runs the streaming form in
both programs and passes trivially.  Oracle parity and run-to-run determinism
of the resident form on its own follow.  Needs the GPU.

Row counts (the resident form runs one 12-wave block per CU over whole
128-row NLL slots, 32-row tiles round-robin over the waves):
  1                  one lane valid; 11 waves and every other block idle at every barrier
  100                one ragged slot; four tiles on 12 waves
  129                a full slot followed by a one-row slot
  4097               several blocks; a ragged last tile
  128 * CUs + 33     every block owns one slot; a ragged tail
  50000              several rounds per wave, tile counts no multiple of 12; the state
                     round trip and the rotation carry across all four couplings"""

import functools

import numpy as np
import pytest

from tests.flowcases import build_flow, make_case

pytestmark = pytest.mark.gpu

NMAX = 50000
# cfg2: the flagship shape; cfg4: C = 2, one transformed dim; cfg1: K = 8, one
# transformed dim; k7: K = 8 (padded) with two transformed dims; cfg4c1: one condition
FLOWS = ["cfg2", "cfg4", "cfg1", "k7", "cfg4c1"]


def _cus():
    try:
        import torch

        return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        return 256


def _row_counts():
    return [1, 100, 129, 4097, 128 * _cus() + 33, NMAX]


@functools.lru_cache(maxsize=None)
def _case(name):
    """One seeded case per flow at the largest N; the smaller batches are its leading rows."""
    return make_case(name, N=max(NMAX, 128 * _cus() + 33), seed=71)


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


@pytest.mark.parametrize("name", FLOWS)
def test_log_prob_and_nll_bits(name, monkeypatch):
    case = _case(name)
    stream = _bind(case, monkeypatch, "0")
    res = _bind(case, monkeypatch, "1")
    for n in _row_counts():
        lp0, nll0 = _log_prob(stream, case, n)
        lp1, nll1 = _log_prob(res, case, n)
        _same_bits(lp1, lp0, f"{name}/N={n} log_prob")
        _same_bits(nll1, nll0, f"{name}/N={n} nll")


@pytest.mark.parametrize("name", FLOWS)
def test_forward_bits(name, monkeypatch):
    case = _case(name)
    stream = _bind(case, monkeypatch, "0")
    res = _bind(case, monkeypatch, "1")
    for n in _row_counts():
        y0, ld0 = stream.forward(_dev(case["x"], n), _dev(case["c"], n))
        y1, ld1 = res.forward(_dev(case["x"], n), _dev(case["c"], n))
        _same_bits(y1.numpy(), y0.numpy(), f"{name}/N={n} y")
        _same_bits(ld1.numpy(), ld0.numpy(), f"{name}/N={n} log_det")


@pytest.mark.parametrize("name", FLOWS)
def test_inverse_and_sample_bits(name, monkeypatch):
    case = _case(name)
    stream = _bind(case, monkeypatch, "0")
    res = _bind(case, monkeypatch, "1")
    rng = np.random.default_rng(72)
    z = (0.5 + 0.1 * rng.standard_normal(case["x"].shape)).astype(np.float32)
    for n in _row_counts():
        x0 = stream.inverse(_dev(z, n), _dev(case["c"], n)).numpy()
        x1 = res.inverse(_dev(z, n), _dev(case["c"], n)).numpy()
        _same_bits(x1, x0, f"{name}/N={n} inverse")
        s0 = stream.program.sample(n, 1234, _dev(case["c"], n)).numpy()
        s1 = res.program.sample(n, 1234, _dev(case["c"], n)).numpy()
        _same_bits(s1, s0, f"{name}/N={n} sample")


@pytest.mark.parametrize("name", ["cfg2", "cfg4", "cfg1"])
def test_oracle_parity_resident(name, monkeypatch):
    """The resident form against the oracle, by test_gpu_flow.py::test_log_prob_parity's bars."""
    from tests.test_gpu_flow import check_lp

    case = make_case(name, N=4097, seed=73)
    res = _bind(case, monkeypatch, "1")
    lp, _ = _log_prob(res, case, 4097)
    check_lp(lp, case, f"{name}/resident")


def test_resident_determinism(monkeypatch):
    case = _case("cfg2")
    res = _bind(case, monkeypatch, "1")
    lp0, nll0 = _log_prob(res, case, NMAX)
    lp1, nll1 = _log_prob(res, case, NMAX)
    _same_bits(lp1, lp0, "log_prob twice")
    _same_bits(nll1, nll0, "nll twice")
