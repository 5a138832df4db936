"""zf_colstats (zenflow_amd/csrc/zf_stats.hip) through the raw C ABI against
a float64 host reference: min / max are np.min / np.max of the float32 column,
sum / sumsq are math.fsum over float64(v) and float64(v)**2.

Tolerances.  min / max of untransformed columns are exact.  Sums:
|got - ref| <= 1e-12 * sum|term| — the longest in-order chain of the two
passes is rows-per-lane + lanes + blocks (at most ~1.1e3 additions at 4096
rows per block and one column, ~2.3e3 on the capped grid), each addition
contributing 1.1e-16 of the running absolute sum.  Pre-transformed columns
(safe_log): the device's logf and NumPy's differ in the last bit, so min /
max are held to rtol 1e-6 and the sums to 2.4e-7 * sum|v| (one float32 ulp,
2^-23, per side and term) and twice that for the squares, on top of the above."""

import ctypes
import math

import numpy as np
import pytest

from zenflow_amd import _lib as L

pytestmark = pytest.mark.gpu
F32 = np.float32
FLT_MIN = F32(1.17549435e-38)
SUM_RTOL = 1e-12
LOG_ULP = 2.4e-7


def colstats(xd, N, ncols, ld, off, modes=None, params=None, want=(True, True, True, True), ws_fill=None):
    """One raw zf_colstats call; outputs not wanted are passed as NULL and
    returned as None."""
    lib = L.load_library()
    ws = L.DeviceArray((int(lib.zf_colstats_workspace_bytes(N, ncols)),), np.uint8)
    if ws_fill is not None:
        L.check(lib.zf_memset_async(ws.ptr, ws_fill, ws.nbytes, L.stream()), "memset")
    outs = [L.DeviceArray((ncols,), dt) if w else None for w, dt in zip(want, (F32, F32, np.float64, np.float64))]
    for o in outs:  # a value no call writes: an output left untouched shows
        if o is not None:
            L.check(lib.zf_memset_async(o.ptr, 0x5A, o.nbytes, L.stream()), "memset")
    m = None if modes is None else np.ascontiguousarray(modes, F32)
    p = None if params is None else np.ascontiguousarray(params, F32)
    rc = lib.zf_colstats(None if xd is None else xd.ptr, N, ncols, ld, off,
                         None if m is None else m.ctypes.data, None if p is None else p.ctypes.data,
                         *[None if o is None else o.ptr for o in outs], ws.ptr, L.stream())
    L.check(rc, "zf_colstats")
    return tuple(None if o is None else o.numpy() for o in outs)


def reference(v):
    """(min, max, sum, sumsq, sum|v|, sum v^2) per column of float32 v (N, ncols)."""
    cols = []
    for j in range(v.shape[1]):
        c = v[:, j].astype(np.float64)
        sq = c * c
        s2 = math.fsum(sq.tolist())
        cols.append((v[:, j].min(), v[:, j].max(), math.fsum(c.tolist()), s2, math.fsum(np.abs(c).tolist()), s2))
    return [np.array(a) for a in zip(*cols)]


def bits(a):
    return a.view(np.uint32 if a.dtype == F32 else np.uint64)


def assert_bit_equal(a, b, cols=None):
    for u, v in zip(a, b):
        if u is None or v is None:
            continue
        if cols is not None:
            u, v = u[cols], v[cols]
        assert np.array_equal(bits(u), bits(v))


def make_data(rng, N, ncols):
    scale = 10.0 ** rng.uniform(-3, 3, size=ncols)  # sumsq spans decades
    return (rng.standard_normal((N, ncols)) * scale).astype(F32)


def check_against_reference(got, v):
    mn, mx, s1, s2, a1, a2 = reference(v)
    assert np.array_equal(got[0], mn.astype(F32))
    assert np.array_equal(got[1], mx.astype(F32))
    print("sum err / bound", np.max(np.abs(got[2] - s1) / (SUM_RTOL * a1)),
          "sumsq err / bound", np.max(np.abs(got[3] - s2) / (SUM_RTOL * a2)))
    assert np.all(np.abs(got[2] - s1) <= SUM_RTOL * a1)
    assert np.all(np.abs(got[3] - s2) <= SUM_RTOL * a2)


@pytest.mark.parametrize("ncols", [1, 2, 3, 5, 48, 64])
@pytest.mark.parametrize("N", [1, 7, 255, 4096, 4097, 12289, 100003])
def test_colstats_vs_fp64(N, ncols):
    """One block and several (N > 4096), idle lanes (ncols not dividing 256),
    ncols = 64, ragged last blocks."""
    rng = np.random.default_rng(1000 * ncols + N)
    v = make_data(rng, N, ncols)
    got = colstats(L.DeviceArray.from_numpy(v), N, ncols, ncols, 0)
    check_against_reference(got, v)


def test_colstats_block_cap():
    """N = 2048 * 4096 + 4097: the grid stops at 2048 blocks and every block
    reduces more than 4096 rows."""
    N = 2048 * 4096 + 4097
    rng = np.random.default_rng(3)
    v = (rng.standard_normal((N, 1)) * 30.0).astype(F32)
    got = colstats(L.DeviceArray.from_numpy(v), N, 1, 1, 0)
    check_against_reference(got, v)


@pytest.mark.parametrize("ncols", [1, 3, 48])
@pytest.mark.parametrize("N", [7, 4097, 12289])
def test_colstats_window(N, ncols):
    """ld = ncols + 5, col_offset = 2: the five outside columns (NaN, 1e38)
    are never read — bit-equal to the compact copy."""
    rng = np.random.default_rng(7 * ncols + N)
    v = make_data(rng, N, ncols)
    wide = np.empty((N, ncols + 5), F32)
    wide[:, :2] = (np.nan, 1e38)
    wide[:, 2:2 + ncols] = v
    wide[:, 2 + ncols:] = (1e38, np.nan, -1e38)
    got = colstats(L.DeviceArray.from_numpy(wide), N, ncols, ncols + 5, 2)
    ref = colstats(L.DeviceArray.from_numpy(v), N, ncols, ncols, 0)
    assert_bit_equal(got, ref)
    check_against_reference(got, v)


@pytest.mark.parametrize("ncols", [1, 5, 64])
def test_colstats_empty_batch(ncols):
    """N = 0: the identities the kernel writes."""
    mn, mx, s1, s2 = colstats(None, 0, ncols, ncols, 0)
    assert np.all(mn == np.inf) and np.all(mx == -np.inf)
    assert np.all(s1 == 0) and np.all(s2 == 0)


def test_colstats_nonfinite():
    """A NaN anywhere in a column (first row, last row, a row of a later
    block) gives min = max = NaN and NaN sums for that column alone; +inf and
    -inf give min = -inf, max = +inf."""
    N, ncols = 12289, 5
    rng = np.random.default_rng(11)
    v = make_data(rng, N, ncols)
    clean = colstats(L.DeviceArray.from_numpy(v), N, ncols, ncols, 0)
    others = [0, 1, 3, 4]
    for row in (0, N - 1, 5000):
        w = v.copy()
        w[row, 2] = np.nan
        got = colstats(L.DeviceArray.from_numpy(w), N, ncols, ncols, 0)
        for g in got:
            assert np.isnan(g[2]), (row, g)
        assert_bit_equal(got, clean, others)
    w = v.copy()
    w[17, 2] = np.inf
    w[9000, 2] = -np.inf
    got = colstats(L.DeviceArray.from_numpy(w), N, ncols, ncols, 0)
    assert got[0][2] == -np.inf and got[1][2] == np.inf
    assert_bit_equal(got, clean, others)


def _pre_case(rng, N):
    modes = np.array([L.ZF_SB_NONE, L.ZF_SB_LOWER, L.ZF_SB_UPPER, L.ZF_SB_LOWER, L.ZF_SB_NONE], F32)
    a = np.array([0.0, 0.0, 10.0, -1.0, 0.0], F32)
    g = rng.standard_normal((N, 5))
    x = np.stack([g[:, 0], np.exp(g[:, 1]), 10 - np.exp(g[:, 2]), -1 + np.exp(g[:, 3]), np.tanh(g[:, 4])],
                 axis=1).astype(F32)
    return modes, a, x


def _pre_reference(modes, a, x):
    """safe_log of the one-sided columns in float32, as the kernel states it."""
    v = x.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        for j, m in enumerate(modes):
            if m == L.ZF_SB_LOWER:
                v[:, j] = np.log((x[:, j] - a[j]) + FLT_MIN)
            elif m == L.ZF_SB_UPPER:
                v[:, j] = np.log((a[j] - x[:, j]) + FLT_MIN)
    return v


@pytest.mark.parametrize("N", [300, 12289])
def test_colstats_pre_transform(N):
    """Mixed modes per column with a in {0, 10, -1}; one value sits exactly on
    its bound, so log(FLT_MIN) ~ -87.34 is that column's minimum."""
    rng = np.random.default_rng(N)
    modes, a, x = _pre_case(rng, N)
    x[N // 2, 1] = 0.0  # at the lower bound a = 0
    x[N - 1, 2] = 10.0  # at the upper bound a = 10
    v = _pre_reference(modes, a, x)
    assert np.isfinite(v).all()
    got = colstats(L.DeviceArray.from_numpy(x), N, 5, 5, 0, modes, a)
    mn, mx, s1, s2, a1, a2 = reference(v)
    plain = modes == L.ZF_SB_NONE
    assert np.array_equal(got[0][plain], mn[plain].astype(F32))
    assert np.array_equal(got[1][plain], mx[plain].astype(F32))
    np.testing.assert_allclose(got[0], mn, rtol=1e-6)
    np.testing.assert_allclose(got[1], mx, rtol=1e-6)
    np.testing.assert_allclose(got[0][1:3], math.log(float(FLT_MIN)), rtol=1e-6)
    ulp = np.where(plain, 0.0, LOG_ULP)
    assert np.all(np.abs(got[2] - s1) <= (SUM_RTOL + ulp) * a1)
    assert np.all(np.abs(got[3] - s2) <= (SUM_RTOL + 2 * ulp) * a2)


def test_colstats_pre_transform_past_bound():
    """A value past its bound makes safe_log NaN, which propagates through
    both passes; the other columns do not see it."""
    N = 12289
    rng = np.random.default_rng(5)
    modes, a, x = _pre_case(rng, N)
    clean = colstats(L.DeviceArray.from_numpy(x), N, 5, 5, 0, modes, a)
    x[6000, 3] = -1.5  # below the lower bound a = -1
    got = colstats(L.DeviceArray.from_numpy(x), N, 5, 5, 0, modes, a)
    for g in got:
        assert np.isnan(g[3])
    assert_bit_equal(got, clean, [0, 1, 2, 4])


def test_colstats_null_outputs_and_determinism():
    """Each output NULL in turn leaves the others bit-equal to the full call;
    two calls are bit-equal, and so are a fresh workspace and one pre-filled
    with 0xFF bytes (nothing is accumulated into it)."""
    N, ncols = 12289, 5
    v = make_data(np.random.default_rng(13), N, ncols)
    xd = L.DeviceArray.from_numpy(v)
    full = colstats(xd, N, ncols, ncols, 0)
    check_against_reference(full, v)
    for k in range(4):
        want = tuple(i != k for i in range(4))
        got = colstats(xd, N, ncols, ncols, 0, want=want)
        assert got[k] is None
        assert_bit_equal(got, full)
    assert_bit_equal(colstats(xd, N, ncols, ncols, 0), full)
    assert_bit_equal(colstats(xd, N, ncols, ncols, 0, ws_fill=0xFF), full)
    assert_bit_equal(colstats(xd, N, ncols, ncols, 0, ws_fill=0x00), full)
