"""K1 parity: zenflow_amd.utils (HIP kernels via the C ABI) vs the oracle and
the reference's own utils tests (tests/test_utils.py).  Needs the GPU."""

import numpy as np
import pytest
from numpy.testing import assert_allclose

from oracle import zf_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32


def _zu():
    from zenflow_amd import utils

    return utils


def random_params(rng, M, N, K, scale=1.0):
    dx = (scale * rng.standard_normal((M, N, K))).astype(F32)
    dy = (scale * rng.standard_normal((M, N, K))).astype(F32)
    sl = (scale * rng.standard_normal((M, N, K - 1))).astype(F32)
    return O.normalize_spline_params(dx, dy, sl)


def test_rational_quadratic_spline_1():
    """test_utils.py:7-13 through the HIP kernel."""
    u = _zu()
    x = np.linspace(-1, 2, 10).reshape(-1, 1)
    W = np.tile([0.25] * 4, len(x)).reshape(*x.shape, -1)
    D = np.tile([1.0] * 3, len(x)).reshape(*x.shape, -1)
    y, log_det = u.rational_quadratic_spline_forward(x, W, W, D)
    assert_allclose(y, x, atol=1e-5)


def test_rational_quadratic_spline_2():
    """test_utils.py:16-50 through the HIP kernel (jacobi -> fp64 central differences)."""
    u = _zu()
    rng = np.random.default_rng(1)
    x = np.linspace(-0.1, 1.1, 1000).reshape(1000, 1)
    dx, dy, slope = u.normalize_spline_params(
        0.1 * rng.normal(size=3), 0.1 * rng.normal(size=3), 0.1 * rng.normal(size=2)
    )
    nx = x.size
    dx = np.tile(dx, nx).reshape(*x.shape, -1)
    dy = np.tile(dy, nx).reshape(*x.shape, -1)
    slope = np.tile(slope, nx).reshape(*x.shape, -1)
    y, log_det = u.rational_quadratic_spline_forward(x, dx, dy, slope)
    h = 1e-7
    d64 = [v.astype(np.float64) for v in (dx, dy, slope)]
    j = ((O.rqs_forward(x + h, *d64)[0] - O.rqs_forward(x - h, *d64)[0]) / (2 * h)).ravel()
    assert_allclose(y, x, atol=0.1)
    assert_allclose(log_det, np.log(j), atol=0.01)
    x2 = u.rational_quadratic_spline_inverse(y, dx, dy, slope)
    assert_allclose(x2, x, atol=1e-4)


@pytest.mark.parametrize("threshold", (0, 0.1))
def test_softmax_with_threshold(threshold):
    """test_utils.py:77-94."""
    u = _zu()
    y = u.softmax_with_threshold(np.array([(-5.0, 1.0, 2.0), (-4.0, 2.0, 3.0)]), threshold)
    assert_allclose(y.sum(-1), 1, rtol=1e-6)
    assert np.all(y >= threshold * (1 - 1e-6))
    assert_allclose(y, O.softmax_with_threshold(np.array([(-5.0, 1.0, 2.0), (-4.0, 2.0, 3.0)], F32), threshold), rtol=1e-6)


def test_normalize_and_squareplus_vs_oracle():
    u = _zu()
    rng = np.random.default_rng(5)
    a = (3 * rng.standard_normal((257, 16))).astype(F32)
    b = (3 * rng.standard_normal((257, 16))).astype(F32)
    c = (3 * rng.standard_normal((257, 15))).astype(F32)
    got = u.normalize_spline_params(a, b, c)
    ref = O.normalize_spline_params(a, b, c)
    for g, r in zip(got, ref):
        assert_allclose(g, r, rtol=2e-6, atol=1e-7)
    # x*x+b may contract to an fma on the GPU; cancellation at large negative x
    assert_allclose(u.squareplus(a), O.squareplus(a), rtol=1e-5)


@pytest.mark.parametrize("K", [2, 4, 5, 8, 16, 32])
@pytest.mark.parametrize("M", [1, 3, 1023, 4099])
def test_normalize_spline_params_shapes(K, M):
    """The float4 stream kernel (K in {4, 8, 16, 32}: ragged tails, rows on
    K/4 lanes, slope tails) and the LDS row kernel (other K) vs the oracle."""
    u = _zu()
    rng = np.random.default_rng(K * 7 + M)
    a = (3 * rng.standard_normal((M, 2, K))).astype(F32)
    b = (3 * rng.standard_normal((M, 2, K))).astype(F32)
    c = (3 * rng.standard_normal((M, 2, K - 1))).astype(F32)
    got = u.normalize_spline_params(a, b, c)
    ref = O.normalize_spline_params(a, b, c)
    # rtol = the north star's 1e-5: x*x + 4 contracts to an fma on the GPU, and
    # squareplus cancels at large negative logits (a 2-knot row divides two
    # such values directly: up to ~3e-6 here)
    for g, r in zip(got, ref):
        assert g.shape == r.shape
        assert_allclose(g, r, rtol=1e-5, atol=1e-7)
    assert_allclose(got[0].sum(-1), 1, rtol=2e-6)


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8, 16, 32, 64])
@pytest.mark.parametrize("N", [1, 2, 3, 8])
def test_rqs_parity(K, N):
    """Random normalised params incl. out-of-bounds x; y, log_det and inverse."""
    u = _zu()
    rng = np.random.default_rng(K * 100 + N)
    M = 3001  # ragged: not a multiple of the block's rows
    dx, dy, sl = random_params(rng, M, N, K, scale=1.5)
    x = rng.uniform(-0.2, 1.2, size=(M, N)).astype(F32)
    y, ld = u.rational_quadratic_spline_forward(x, dx, dy, sl)
    yr, ldr = O.rqs_forward(x, dx, dy, sl)
    fin = np.isfinite(yr)
    assert np.array_equal(fin, np.isfinite(y))
    assert_allclose(y[fin], yr[fin], rtol=2e-6, atol=2e-6)
    finl = np.isfinite(ldr)
    assert np.array_equal(finl, np.isfinite(ld))
    assert_allclose(ld[finl], ldr[finl], rtol=1e-5, atol=1e-5)
    xi = u.rational_quadratic_spline_inverse(yr, dx, dy, sl)
    xr = O.rqs_inverse(yr, dx, dy, sl)
    fin = np.isfinite(xr)
    assert np.array_equal(fin, np.isfinite(xi))
    assert_allclose(xi[fin], xr[fin], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("K", [16, 32])
def test_rqs_parity_bench_shape(K):
    """K1 at the bench's timed shape — one cfg2 coupling over 2^20 rows x 2
    transformed dims (bench.py spline_kernel) — against the oracle on every
    row: y, log_det, and the inverse of the reference's y."""
    u = _zu()
    rng = np.random.default_rng(K)
    M = 1 << 20
    dx, dy, sl = random_params(rng, M, 2, K, scale=1.5)
    x = rng.uniform(-0.05, 1.05, size=(M, 2)).astype(F32)
    y, ld = u.rational_quadratic_spline_forward(x, dx, dy, sl)
    yr, ldr = O.rqs_forward(x, dx, dy, sl)
    fin = np.isfinite(yr)
    assert np.array_equal(fin, np.isfinite(y))
    assert_allclose(y[fin], yr[fin], rtol=2e-6, atol=2e-6)
    finl = np.isfinite(ldr)
    assert np.array_equal(finl, np.isfinite(ld))
    assert_allclose(ld[finl], ldr[finl], rtol=1e-5, atol=1e-5)
    xi = u.rational_quadratic_spline_inverse(yr, dx, dy, sl)
    xr = O.rqs_inverse(yr, dx, dy, sl)
    fin = np.isfinite(xr)
    assert np.array_equal(fin, np.isfinite(xi))
    assert_allclose(xi[fin], xr[fin], rtol=1e-5, atol=1e-5)


def test_rqs_edge_cases():
    """Sliver idx == K (fill-mode gather -> NaN), x == 1 (OOB identity), NaN x,
    empty batch."""
    u = _zu()
    K = 4
    dx = np.full((1, 5, K), 0.2499999, F32)  # sums to < 1
    dy = np.full((1, 5, K), 0.25, F32)
    sl = np.ones((1, 5, K - 1), F32)
    x = np.array([[0.99999994, 1.0, np.nan, 0.5, -0.0]], F32)
    y, ld = u.rational_quadratic_spline_forward(x, dx, dy, sl)
    yr, ldr = O.rqs_forward(x, dx, dy, sl)
    assert np.isnan(y[0, 0]) and np.isnan(yr[0, 0])
    assert y[0, 1] == 1.0 and yr[0, 1] == 1.0
    assert np.isnan(y[0, 2]) and np.isnan(yr[0, 2])
    assert_allclose(y[0, 3:], yr[0, 3:], atol=1e-6)
    assert np.isnan(ld[0]) and np.isnan(ldr[0])
    y0, ld0 = u.rational_quadratic_spline_forward(
        np.zeros((0, 2), F32), np.zeros((0, 2, K), F32), np.zeros((0, 2, K), F32), np.zeros((0, 2, K - 1), F32)
    )
    assert y0.shape == (0, 2) and ld0.shape == (0,)


def test_rqs_golden():
    """Committed golden vectors (tests/golden/make_golden.py)."""
    from pathlib import Path

    u = _zu()
    g = Path(__file__).parent / "golden"
    for f in sorted(g.glob("rqs_K*.npz")):
        d = np.load(f)
        y, ld = u.rational_quadratic_spline_forward(d["x"], d["dx"], d["dy"], d["slope"])
        fin = np.isfinite(d["y"])
        assert_allclose(y[fin], d["y"][fin], rtol=2e-6, atol=2e-6, err_msg=f.name)
        assert_allclose(ld, d["log_det"], rtol=1e-5, atol=1e-5, err_msg=f.name)
        xi = u.rational_quadratic_spline_inverse(d["y"], d["dx"], d["dy"], d["slope"])
        fin = np.isfinite(d["x_inv"])
        assert_allclose(xi[fin], d["x_inv"][fin], rtol=1e-5, atol=1e-5, err_msg=f.name)


@pytest.mark.parametrize("N", [1, 2, 3, 8, 40])
@pytest.mark.parametrize("monotone", [True, False])
def test_rqs_k32_two_lane_matches_one_lane(N, monotone, monkeypatch):
    """K = 32 runs two lanes per item (rqs_kernel_pair: lane 1 continues lane
    0's in-order knot sums, so bins and knots carry the one-lane kernel's
    bits): the same results as the one-lane kernel (ZF_K1_ONE_LANE=1) up to
    the compiler's fma contraction of the evaluation (a few ulp), forward,
    log_det (lane-shuffle rows, N <= 32, and the LDS rows, N = 40) and
    inverse, on normalised and on raw (non-monotone knots: the generic-search
    fallback) parameters; identical finiteness (same bins)."""
    u = _zu()
    K = 32
    rng = np.random.default_rng(900 + N)
    M = 2051
    if monotone:
        dx, dy, sl = random_params(rng, M, N, K, scale=1.5)
    else:
        dx = (0.06 * rng.standard_normal((M, N, K)) + 0.03).astype(F32)
        dy = (0.06 * rng.standard_normal((M, N, K)) + 0.03).astype(F32)
        sl = np.abs(rng.standard_normal((M, N, K - 1))).astype(F32) + 0.1
    x = rng.uniform(-0.1, 1.1, size=(M, N)).astype(F32)
    y2, ld2 = u.rational_quadratic_spline_forward(x, dx, dy, sl)
    xi2 = u.rational_quadratic_spline_inverse(x, dx, dy, sl)
    monkeypatch.setenv("ZF_K1_ONE_LANE", "1")
    y1, ld1 = u.rational_quadratic_spline_forward(x, dx, dy, sl)
    xi1 = u.rational_quadratic_spline_inverse(x, dx, dy, sl)
    for a, b in ((y1, y2), (ld1, ld2), (xi1, xi2)):
        assert np.array_equal(np.isfinite(a), np.isfinite(b))
        f = np.isfinite(a)
        assert_allclose(b[f], a[f], rtol=1e-6, atol=1e-6)


# ---------------------------------------------------------------------------
# The raw C ABI: branches zenflow_amd.utils never reaches (its fresh
# DeviceArrays are 16-byte aligned, its outputs never NULL).
# ---------------------------------------------------------------------------


def _upload(a, off=0):
    """Host array -> `base + off` bytes of a DeviceArray one float4 larger;
    returns (owner, device pointer)."""
    from zenflow_amd import _lib as L

    a = np.ascontiguousarray(a, F32)
    d = L.DeviceArray((a.size + 4,))
    if a.size:
        L.check(L.load_library().zf_memcpy_htod(d.ptr + off, a.ctypes.data, a.nbytes, L.stream()), "htod")
        L.synchronize()
    return d, d.ptr + off


def _download(ptr, shape):
    from zenflow_amd import _lib as L

    out = np.empty(shape, F32)
    if out.size:
        L.check(L.load_library().zf_memcpy_dtoh(out.ctypes.data, ptr, out.nbytes, L.stream()), "dtoh")
        L.synchronize()
    return out


def raw_rqs(x, dx, dy, sl, inverse=False, offs=(0, 0, 0), want_y=True, want_ld=True, rc_only=False):
    """zf_rqs_forward / zf_rqs_inverse with dx, dy, slope at `offs` bytes past
    a 16-byte boundary; forward returns (y or None, log_det or None)."""
    from zenflow_amd import _lib as L

    lib = L.load_library()
    M, N = x.shape
    K = dx.shape[-1]
    keep = [_upload(x)] + [_upload(a, o) for a, o in zip((dx, dy, sl), offs)]
    px, pdx, pdy, psl = (p for _, p in keep)
    y = L.DeviceArray((M, N)) if want_y else None
    yp = None if y is None else y.ptr
    if inverse:
        rc = lib.zf_rqs_inverse(px, pdx, pdy, psl, yp, M, N, K, L.stream())
    else:
        ld = L.DeviceArray((M,)) if want_ld else None
        rc = lib.zf_rqs_forward(px, pdx, pdy, psl, yp, None if ld is None else ld.ptr, M, N, K, L.stream())
    if rc_only:
        return rc
    L.check(rc, "zf_rqs")
    if inverse:
        return y.numpy()
    return (None if y is None else y.numpy(), None if ld is None else ld.numpy())


def raw_normalize(a, b, c, offs=(0, 0, 0)):
    """zf_normalize_spline_params in place on uploads at `offs`; c may be None
    (slope = NULL, K = 1)."""
    from zenflow_amd import _lib as L

    M, K = a.shape
    keep = [_upload(v, o) for v, o in zip((a, b), offs)]
    pc = None
    if c is not None:
        keep.append(_upload(c, offs[2]))
        pc = keep[2][1]
    L.check(L.load_library().zf_normalize_spline_params(keep[0][1], keep[1][1], pc, M, K, L.stream()),
            "zf_normalize_spline_params")
    out = [_download(keep[0][1], a.shape), _download(keep[1][1], b.shape)]
    if c is not None:
        out.append(_download(pc, c.shape))
    return out


def _rqs_case(K, N, M, seed):
    rng = np.random.default_rng(seed)
    dx, dy, sl = random_params(rng, M, N, K, scale=1.5)
    x = rng.uniform(-0.2, 1.2, size=(M, N)).astype(F32)
    return x, dx, dy, sl


def _assert_rqs_vs_oracle(x, dx, dy, sl, y, ld, xi, yr=None):
    """The tolerances of test_rqs_parity; xi = inverse of the oracle's y."""
    yr, ldr = O.rqs_forward(x, dx, dy, sl)
    fin = np.isfinite(yr)
    assert np.array_equal(fin, np.isfinite(y))
    assert_allclose(y[fin], yr[fin], rtol=2e-6, atol=2e-6)
    finl = np.isfinite(ldr)
    assert np.array_equal(finl, np.isfinite(ld))
    assert_allclose(ld[finl], ldr[finl], rtol=1e-5, atol=1e-5)
    xr = O.rqs_inverse(yr, dx, dy, sl)
    fin = np.isfinite(xr)
    assert np.array_equal(fin, np.isfinite(xi))
    assert_allclose(xi[fin], xr[fin], rtol=1e-5, atol=1e-5)


def _raw_all(x, dx, dy, sl, offs=(0, 0, 0)):
    """(y, log_det, inverse of the oracle's y) through the raw ABI."""
    y, ld = raw_rqs(x, dx, dy, sl, offs=offs)
    yr, _ = O.rqs_forward(x, dx, dy, sl)
    xi = raw_rqs(yr, dx, dy, sl, inverse=True, offs=offs)
    return y, ld, xi


@pytest.mark.parametrize("K", [4, 8, 16, 32])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("offs", [(4, 4, 4), (0, 4, 0)], ids=["all+4", "dy+4"])
def test_rqs_unaligned_fallback(K, N, offs):
    """dx / dy off a 16-byte boundary (either one: the alignment test ORs the
    pointers) run the LDS-staged rqs_kernel<FWD, K>: oracle parity, and the
    aligned kernels' results on the same values within 1e-6 (the bound of the
    one-lane / two-lane test) with identical finiteness."""
    x, dx, dy, sl = _rqs_case(K, N, 1031, 40 * K + N)
    got = _raw_all(x, dx, dy, sl, offs)
    _assert_rqs_vs_oracle(x, dx, dy, sl, *got)
    ref = _raw_all(x, dx, dy, sl)
    for a, b in zip(ref, got):
        assert np.array_equal(np.isfinite(a), np.isfinite(b))
        f = np.isfinite(a)
        assert_allclose(b[f], a[f], rtol=1e-6, atol=1e-6)


def _normalize_case(K, M, seed):
    rng = np.random.default_rng(seed)
    a = (3 * rng.standard_normal((M, K))).astype(F32)
    b = (3 * rng.standard_normal((M, K))).astype(F32)
    c = (3 * rng.standard_normal((M, K - 1))).astype(F32)
    return a, b, c


@pytest.mark.parametrize("K", [4, 8, 16, 32])
@pytest.mark.parametrize("M", [1, 1023])
@pytest.mark.parametrize("offs", [(4, 4, 4), (0, 4, 0)], ids=["all+4", "dy+4"])
def test_normalize_unaligned_fallback(K, M, offs):
    """Unaligned arrays at the stream kernel's K run normalize_kernel."""
    a, b, c = _normalize_case(K, M, 50 * K + M)
    got = raw_normalize(a, b, c, offs)
    for g, r in zip(got, O.normalize_spline_params(a, b, c)):
        assert_allclose(g, r, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("K", [4, 8, 16, 32])
@pytest.mark.parametrize("M", [1, 1023])
def test_normalize_row_kernel_switch(K, M, monkeypatch):
    """ZF_NORM_ROWS=1: the row kernel on aligned arrays, against the oracle and
    within 2e-6 of the stream kernel (sequential row sum vs lane partials)."""
    a, b, c = _normalize_case(K, M, 60 * K + M)
    vec = raw_normalize(a, b, c)
    monkeypatch.setenv("ZF_NORM_ROWS", "1")
    row = raw_normalize(a, b, c)
    for g, v, r in zip(row, vec, O.normalize_spline_params(a, b, c)):
        assert_allclose(g, r, rtol=1e-5, atol=1e-7)
        assert_allclose(g, v, rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize(
    "K,N",
    [(16, n) for n in (64, 100, 128, 200, 256)]
    + [(32, n) for n in (64, 100, 128, 129, 256)]
    + [(5, n) for n in (64, 100, 256)]
    + [(4, 256)],
)
def test_rqs_wide_rows(K, N):
    """N > 40: the direct kernel's LDS log-det rows (N > 64 or not a power of
    two), one row per block (N in 129..256), the pair kernel at N = 128 and
    K = 32 past it on rqs_kernel_direct<32>; K = 5 on the LDS-staged kernel."""
    x, dx, dy, sl = _rqs_case(K, N, 37, 1000 * K + N)
    _assert_rqs_vs_oracle(x, dx, dy, sl, *_raw_all(x, dx, dy, sl))


@pytest.mark.parametrize("K", [100, 200, 256])
@pytest.mark.parametrize("N", [1, 2])
def test_rqs_large_k(K, N):
    """K above 64 (runtime-K rqs_kernel, few rows per block)."""
    x, dx, dy, sl = _rqs_case(K, N, 301, 7 * K + N)
    _assert_rqs_vs_oracle(x, dx, dy, sl, *_raw_all(x, dx, dy, sl))


def test_rqs_valid_call_after_rejected():
    """A rejected shape (N = 257: ZF_ENOTSUP) leaves no state behind."""
    from zenflow_amd import _lib as L

    x, dx, dy, sl = _rqs_case(16, 257, 2, 3)
    assert raw_rqs(x, dx, dy, sl, rc_only=True) == -2
    assert L.load_library().zf_last_error()
    assert raw_rqs(x, dx, dy, sl, inverse=True, rc_only=True) == -2
    x, dx, dy, sl = _rqs_case(16, 3, 301, 4)
    _assert_rqs_vs_oracle(x, dx, dy, sl, *_raw_all(x, dx, dy, sl))


@pytest.mark.parametrize(
    "K,offs",
    [(16, (0, 0, 0)), (32, (0, 0, 0)), (5, (0, 0, 0)), (16, (4, 4, 4))],
    ids=["direct16", "pair32", "lds5", "unaligned16"],
)
@pytest.mark.parametrize("N", [2, 3])
def test_rqs_null_outputs(K, offs, N):
    """y = NULL or log_det = NULL (both allowed by the header): the surviving
    output carries the bits of the call that returns both."""
    x, dx, dy, sl = _rqs_case(K, N, 301, 9 * K + N)
    y, ld = raw_rqs(x, dx, dy, sl, offs=offs)
    y1, ld1 = raw_rqs(x, dx, dy, sl, offs=offs, want_ld=False)
    y2, ld2 = raw_rqs(x, dx, dy, sl, offs=offs, want_y=False)
    assert ld1 is None and y2 is None
    assert np.array_equal(y1.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(ld2.view(np.uint32), ld.view(np.uint32))


def _softmax_raw(x, threshold):
    from zenflow_amd import _lib as L

    M, K = x.shape
    xd = L.DeviceArray.from_numpy(x)
    out = L.DeviceArray((M, K))
    L.check(L.load_library().zf_softmax_with_threshold(xd.ptr, out.ptr, M, K, float(threshold), L.stream()),
            "zf_softmax_with_threshold")
    return out.numpy()


def _softmax_thresholds(K):
    """0, 1e-5, 1e-3 and 0.5 / K, where the reference is defined:
    c = t / (1 - K t) needs K t < 1 (at K = 1000, t = 1e-3 it divides by zero,
    beyond that c < 0 and `threshold` is no longer the minimum)."""
    return [t for t in (0.0, 1e-5, 1e-3, 0.5 / K) if K * t < 1]


@pytest.mark.parametrize(
    "K,M",
    [(k, m) for k in (1, 2, 3, 7, 16, 33, 64, 255) for m in (1, 255, 257, 1025)]
    + [(k, m) for k in (1000, 6144) for m in (1, 5)],
)
def test_softmax_with_threshold_shapes(K, M):
    """Rows per block from 256 (small K) down to 1 (K = 6144), ragged last
    blocks, every threshold: oracle parity, rows sum to 1, min >= threshold."""
    rng = np.random.default_rng(K * 13 + M)
    x = (3 * rng.standard_normal((M, K))).astype(F32)
    for t in _softmax_thresholds(K):
        y = _softmax_raw(x, t)
        assert_allclose(y, O.softmax_with_threshold(x, t), rtol=1e-5, atol=1e-7, err_msg=f"threshold {t}")
        assert_allclose(y.astype(np.float64).sum(-1), 1, rtol=0, atol=2e-6, err_msg=f"threshold {t}")
        assert np.all(y >= t * (1 - 1e-6)), t


@pytest.mark.parametrize("K", [3, 16, 33])
def test_softmax_row_isolation(K):
    """Poisoned rows (all -1e4: squareplus cancels to 0 and the row is 0 / 0;
    one NaN; one +1e30) keep the oracle's finiteness pattern and leave every
    other row's bits alone."""
    M = 600
    rng = np.random.default_rng(K)
    x = (3 * rng.standard_normal((M, K))).astype(F32)
    clean = _softmax_raw(x, 1e-5)
    p = x.copy()
    p[300] = -1e4
    p[301, K // 2] = np.nan
    p[302, K - 1] = 1e30
    got = _softmax_raw(p, 1e-5)
    with np.errstate(all="ignore"):
        ref = O.softmax_with_threshold(p, 1e-5)
    assert np.isnan(ref[300]).all()
    assert np.array_equal(np.isfinite(got[300:303]), np.isfinite(ref[300:303]))
    keep = np.ones(M, bool)
    keep[300:303] = False
    assert np.array_equal(got[keep].view(np.uint32), clean[keep].view(np.uint32))


@pytest.mark.parametrize(
    "K,M",
    [(k, m) for k in (1, 3, 24, 64, 100, 200) for m in (1, 3, 257)] + [(3000, 3), (6143, 3)],
)
def test_normalize_spline_params_other_k(K, M):
    """normalize_kernel at K = 1 (slope = NULL), odd and even K, K = 24 (the
    LDS request closest to the 48 KiB budget) and up to the largest K one
    block holds."""
    a, b, c = _normalize_case(K, M, 70 * K + M)
    got = raw_normalize(a, b, c if K > 1 else None)
    for g, r in zip(got, O.normalize_spline_params(a, b, c)):
        assert g.shape == r.shape
        assert_allclose(g, r, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("n", [1, 255, 257, 100003])
@pytest.mark.parametrize("b", [4, 1, 0.25])
def test_squareplus_sizes(n, b):
    u = _zu()
    x = (3 * np.random.default_rng(n).standard_normal(n)).astype(F32)
    assert_allclose(u.squareplus(x, b), O.squareplus(x, b), rtol=1e-5)
