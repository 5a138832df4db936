"""zf_segment_take on the GPU (``nn.segment_take`` / ``nn.take_rows``): whole
sets gathered by index out of a resident ragged batch, with their CSR offsets
rebuilt.  A gather is exact, so every comparison is ``array_equal`` against
the NumPy restatement below, never a tolerance.

Shapes: the gather kernel takes one block per 256 output rows, so the lengths
of case (a) put sets inside, across and over several blocks (255, 256, 257,
700) between empty neighbours; the plan is one block of 1,024 threads, so case
(b) takes 2,500 of 3,000 sets: slices of three entries per thread and offsets
past the first 1,024."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = F32(-12345.5)

LENGTHS = [5, 0, 0, 255, 0, 256, 257, 0, 700, 1, 1, 0, 3, 64, 0, 0, 17, 2, 130, 0,
           9, 31, 0, 1, 6, 0, 44, 12, 0, 0, 7, 100, 1, 0, 8, 23, 0, 5, 60, 0]


def _ref_take(x, off, take, rows_out):
    """The header's definition in NumPy.  off None: every row is its own set."""
    from zenflow_amd import nn

    rows, F = x.shape
    o = np.arange(rows + 1, dtype=np.int64) if off is None else nn.clamp_offsets(off, rows)
    S = len(o) - 1
    out = np.zeros((rows_out, F), F32)
    off_out = np.zeros(len(take) + 1, np.int64)
    for t, s in enumerate(take):
        n = int(o[s + 1] - o[s]) if 0 <= s < S else 0
        off_out[t + 1] = min(off_out[t] + n, rows_out)
        k = int(off_out[t + 1] - off_out[t])
        out[off_out[t]:off_out[t + 1]] = x[o[s]:o[s] + k] if k else 0
    return out, off_out


def _raw_take(x, off, take, rows_out, guard=0):
    """zf_segment_take itself on device copies of x (rows, F), off (any int64s,
    or None) and take (any int64s): (out, off_out, the guard region behind
    out).  out and the guard are pre-filled with SENTINEL, off_out with -7."""
    from zenflow_amd import _lib as L

    lib = L.load_library()
    L.ensure_device()
    rows, F = x.shape
    S = rows if off is None else len(off) - 1
    n = len(take)
    xd = L.DeviceArray.from_numpy(np.ascontiguousarray(x, F32))
    od = None if off is None else L.DeviceArray.from_numpy(np.asarray(off, np.int64))
    td = L.DeviceArray.from_numpy(np.asarray(take, np.int64))
    out = L.DeviceArray.from_numpy(np.full((rows_out + guard) * F, SENTINEL, F32))
    off_out = L.DeviceArray.from_numpy(np.full(n + 1, -7, np.int64))
    ws = L.DeviceArray((max(1, lib.zf_segment_take_workspace_bytes(S, n)),), np.uint8)
    L.check(lib.zf_segment_take(xd.ptr, rows, F, None if od is None else od.ptr, S, td.ptr, n, rows_out, out.ptr,
                                off_out.ptr, ws.ptr, L.stream()), "zf_segment_take")
    flat = out.numpy()
    return flat[:rows_out * F].reshape(rows_out, F), off_out.numpy(), flat[rows_out * F:]


@pytest.fixture(scope="module")
def batch():
    """x (rows, 64) and the offsets of LENGTHS; narrower cases take its first columns."""
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((int(off[-1]), 64)).astype(F32)
    x.setflags(write=False)
    return x, off


def _take_of(S, seed):
    """A permutation of the sets plus duplicates."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.permutation(S), rng.integers(0, S, 9)]).astype(np.int64)


@pytest.mark.parametrize("F", [1, 3, 64])
def test_take_matches_numpy(batch, F):
    """(a) host arrays through nn.segment_take, and the same on DeviceArrays."""
    from zenflow_amd import _lib as L
    from zenflow_amd import nn

    x, off = batch
    x = np.ascontiguousarray(x[:, :F])
    take = _take_of(len(off) - 1, F)
    rows = int(np.diff(off)[take].sum())
    want, want_off = _ref_take(x, off, take, rows)
    assert want_off[-1] == rows >= int(off[-1])
    got, got_off = nn.segment_take(x, off, take)
    assert got.dtype == F32 and got.shape == (rows, F) and got_off.dtype == np.int64
    assert np.array_equal(got_off, want_off)
    assert np.array_equal(got, want)
    xd, od, td = (L.DeviceArray.from_numpy(a) for a in (x, off, take))
    dev, dev_off = nn.segment_take(xd, od, td, rows=rows)
    assert isinstance(dev, L.DeviceArray) and isinstance(dev_off, L.DeviceArray) and dev_off.dtype == np.int64
    assert np.array_equal(dev.numpy(), want) and np.array_equal(dev_off.numpy(), want_off)


def test_take_many_short_sets():
    """(b) 3,000 sets of 0 - 3 rows, 2,500 of them taken."""
    from zenflow_amd import nn

    rng = np.random.default_rng(2)
    lengths = rng.integers(0, 4, 3000)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    x = rng.standard_normal((int(off[-1]), 3)).astype(F32)
    take = rng.permutation(3000)[:2500].astype(np.int64)
    want, want_off = _ref_take(x, off, take, int(lengths[take].sum()))
    got, got_off = nn.segment_take(x, off, take)
    assert np.array_equal(got_off, want_off) and want_off[-1] > 1024
    assert np.array_equal(got, want)


def test_take_makes_device_garbage_harmless(batch):
    """(c) indices outside [0, S) are empty sets, offsets are clamped by the rule of zf_segment_sum."""
    x, off = batch
    x = np.ascontiguousarray(x[:, :3])
    rows, S = len(x), len(off) - 1
    take = np.array([3, -1, 8, S, 0, 1 << 40, 6, -(1 << 40), 8, S + 1, 5], np.int64)
    bad = off.copy()
    bad[4] = -50          # below 0
    bad[7] = bad[6] - 90  # decreasing
    bad[9] = rows + 1000  # beyond x: every later offset is clamped to rows
    bad[20] = -(1 << 50)
    for o in (off, bad):
        rows_out = int(rows + 300)
        want, want_off = _ref_take(x, o, take, rows_out)
        got, got_off, _ = _raw_take(x, o, take, rows_out)
        assert np.array_equal(got_off, want_off)
        assert np.array_equal(got, want)


def test_take_rows_out_above_and_below_the_sum(batch):
    """(d) a zero tail above the sum; below it truncated offsets, and nothing written behind out."""
    x, off = batch
    x = np.ascontiguousarray(x[:, :3])
    take = _take_of(len(off) - 1, 4)
    total = int(np.diff(off)[take].sum())
    for rows_out in (total + 257, total + 1):
        got, got_off, _ = _raw_take(x, off, take, rows_out)
        want, want_off = _ref_take(x, off, take, rows_out)
        assert np.array_equal(got_off, want_off) and got_off[-1] == total
        assert np.array_equal(got, want) and not got[total:].any()
    for rows_out in (total - 1, total // 2, 700, 256, 1):
        got, got_off, guard = _raw_take(x, off, take, rows_out, guard=600)
        want, want_off = _ref_take(x, off, take, rows_out)
        assert got_off[-1] == rows_out and np.array_equal(got_off, want_off)
        assert np.array_equal(got, want)
        assert (guard == SENTINEL).all()


def test_take_nothing(batch):
    """(e) take_n == 0 and rows_out == 0."""
    x, off = batch
    x = np.ascontiguousarray(x[:, :3])
    got, got_off, guard = _raw_take(x, off, np.zeros(0, np.int64), 40, guard=8)
    assert got_off.tolist() == [0] and not got.any() and (guard == SENTINEL).all()
    got, got_off, guard = _raw_take(x, off, np.array([3, 5, 8], np.int64), 0, guard=8)
    assert got.shape == (0, 3) and got_off.tolist() == [0, 0, 0, 0] and (guard == SENTINEL).all()
    got, got_off, guard = _raw_take(x, off, np.zeros(0, np.int64), 0, guard=8)
    assert got_off.tolist() == [0] and (guard == SENTINEL).all()


def test_take_rows_is_fancy_indexing():
    """(f) unit mode: y[take] for 1-D and 2-D y, host and device."""
    from zenflow_amd import _lib as L
    from zenflow_amd import nn

    rng = np.random.default_rng(6)
    take = np.concatenate([rng.permutation(700), rng.integers(0, 700, 50)]).astype(np.int64)
    for shape in ((700,), (700, 1), (700, 2), (700, 64)):
        y = rng.standard_normal(shape).astype(F32)
        got = nn.take_rows(y, take)
        assert got.shape == y[take].shape and np.array_equal(got, y[take])
        dev = nn.take_rows(L.DeviceArray.from_numpy(y), L.DeviceArray.from_numpy(take))
        assert isinstance(dev, L.DeviceArray) and dev.shape == y[take].shape and np.array_equal(dev.numpy(), y[take])
    # a device index outside [0, S) is an empty set, as in every mode: its row is left out, the rows behind it
    # move up and zero rows close the result (the header's off_out rule with len_t = 0)
    y = rng.standard_normal((5, 2)).astype(F32)
    bad = np.array([4, 5, -1, 0], np.int64)
    dev = nn.take_rows(L.DeviceArray.from_numpy(y), L.DeviceArray.from_numpy(bad))
    assert np.array_equal(dev.numpy(), _ref_take(y, None, bad, 4)[0])
    assert np.array_equal(dev.numpy(), np.stack([y[4], y[0], np.zeros(2, F32), np.zeros(2, F32)]))


def test_sum_of_taken_sets_is_the_taken_sum(batch):
    """(g) the sum's order of additions depends on the set alone: pooling the
    packed batch gives the rows of the full batch's pooling, bit for bit."""
    from zenflow_amd import nn

    x, off = batch
    x = np.ascontiguousarray(x[:, :3])
    take = _take_of(len(off) - 1, 7)
    full = nn.segment_sum(x, off)
    packed = nn.segment_sum(*nn.segment_take(x, off, take))
    assert packed.shape == (len(take), 3)
    assert np.array_equal(packed, full[take])
