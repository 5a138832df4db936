"""Host side of the deep-set minibatch driver (zf_segment_take,
``nn.segment_take`` / ``nn.take_rows``, ``zenflow_amd.train.train_sets``): the
entries exist with their signatures, every argument check returns before the
first HIP call (host pointers stand in for device ones, as in
tests/test_pool_host.py; on a host without a GPU a device call would raise
RuntimeError, not ValueError), and the batch plan's capacities bound every
batch of every permutation.  No GPU compute is called here."""

import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "zenflow_amd.h").read_text()
F32 = np.float32


def test_entries_are_in_header_library_and_signatures():
    from zenflow_amd import _lib as L
    from zenflow_amd import nn

    lib = L.load_library()
    m = re.search(r"^int64_t zf_segment_take_workspace_bytes\((.*?)\);", HEADER, re.M | re.S)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["int64_t sets", "int64_t take_n"]
    m = re.search(r"^int zf_segment_take\((.*?)\);", HEADER, re.M | re.S)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const float* x", "int64_t rows", "int F", "const int64_t* off", "int64_t sets",
                    "const int64_t* take", "int64_t take_n", "int64_t rows_out", "float* out", "int64_t* off_out",
                    "void* workspace", "void* stream"]
    for fn, nargs in (("zf_segment_take_workspace_bytes", 2), ("zf_segment_take", 12)):
        assert fn in L.SIGNATURES and len(L.SIGNATURES[fn][1]) == nargs
        assert len(getattr(lib, fn).argtypes) == nargs
    # it stands next to the repeat, and names the clamping rule and unit mode
    assert HEADER.index("int zf_segment_repeat") < HEADER.index("int zf_segment_take") < HEADER.index("Dropout —")
    doc = HEADER[HEADER.index("Take whole sets by index"):HEADER.index("int zf_segment_take(")]
    assert "zf_segment_sum" in doc and "unit mode" in doc and "No atomics" in doc
    assert {"segment_take", "take_rows"} <= set(nn.__all__)
    # the workspace: the clamped offsets
    assert lib.zf_segment_take_workspace_bytes(1000, 10) == 1001 * 8
    assert lib.zf_segment_take_workspace_bytes(-1, 10) == 0 and lib.zf_segment_take_workspace_bytes(5, -1) == 0


# (F, rows, sets, take_n, rows_out, NULL argument, unit mode, code)
REJECTED = [(3, 8, 2, 4, 8, k, False, -1) for k in ("x", "take", "out", "off_out", "ws")] + [
    (3, -1, 2, 4, 8, None, False, -1), (3, 8, -1, 4, 8, None, False, -1), (3, 8, 2, -1, 8, None, False, -1),
    (3, 8, 2, 4, -1, None, False, -1),
    (0, 8, 2, 4, 8, None, False, -1), (65, 8, 2, 4, 8, None, False, -1),
    (3, 8, 2, 4, 8, None, True, -1),  # off NULL: every set is one row, so sets must be rows
    (3, 8, (1 << 24) + 1, 4, 8, None, False, -2), (3, 8, 2, (1 << 24) + 1, 8, None, False, -2),
    (3, 1 << 31, 2, 4, 8, None, False, -2), (3, 8, 2, 4, 1 << 31, None, False, -2),
]


@pytest.mark.parametrize("F,rows,sets,take_n,rows_out,null,unit,rc", REJECTED)
def test_segment_take_rejects_before_any_launch(F, rows, sets, take_n, rows_out, null, unit, rc):
    from zenflow_amd import _lib as L

    lib = L.load_library()
    buf = np.zeros(64, F32)
    p = buf.ctypes.data
    a = {k: (None if null == k else p) for k in ("x", "take", "out", "off_out", "ws")}
    got =lib.zf_segment_take(a["x"], rows, F, None if unit else p, sets, a["take"], take_n, rows_out, a["out"],
                              a["off_out"], a["ws"], None)
    assert got == rc
    assert lib.zf_last_error()
    assert not buf.any()  # nothing was written through the host pointers


def _fake_device(shape, dtype):
    """A DeviceArray that owns nothing: what the checks read (shape, dtype) without a device."""
    from zenflow_amd._lib import DeviceArray

    d = DeviceArray.__new__(DeviceArray)
    d.ptr, d.shape, d.dtype, d.nbytes, d._fin = 0, tuple(shape), np.dtype(dtype), 0, None
    return d


@pytest.mark.parametrize("take", [[[0, 1]], [0.5, 1.0], [0, -1], [0, 4], ["a"]])
def test_python_take_is_validated(take):
    from zenflow_amd import nn

    x = np.zeros((10, 3), F32)
    off = [0, 2, 5, 5, 10]  # S = 4
    with pytest.raises(ValueError, match="take"):
        nn.segment_take(x, off, take)
    with pytest.raises(ValueError, match="take"):
        nn.take_rows(np.zeros((4, 2), F32), take)
    with pytest.raises(ValueError, match="take"):
        nn.take_rows(np.zeros(4, F32), take)


def test_python_rows_rules():
    from zenflow_amd import nn

    x = np.zeros((10, 3), F32)
    off = np.array([0, 2, 5, 5, 10])
    # device-style arguments are not read back: rows must be given
    with pytest.raises(ValueError, match="give rows"):
        nn.segment_take(x, _fake_device((5,), np.int64), [0, 1])
    with pytest.raises(ValueError, match="give rows"):
        nn.segment_take(x, off, _fake_device((2,), np.int64))
    with pytest.raises(ValueError, match="int64"):
        nn.segment_take(x, off, _fake_device((2,), np.int32), rows=4)
    with pytest.raises(ValueError, match="int64"):
        nn.take_rows(x, _fake_device((2, 1), np.int64))
    # rows below the host-known sum, negative rows, bad offsets, bad shapes
    with pytest.raises(ValueError, match="7 rows"):
        nn.segment_take(x, off, [3, 0], rows=6)
    with pytest.raises(ValueError, match="negative"):
        nn.segment_take(x, off, [2], rows=-1)
    with pytest.raises(ValueError, match="offsets"):
        nn.segment_take(x, [0, 5, 2, 10], [0])
    with pytest.raises(ValueError, match="2-D"):
        nn.segment_take(np.zeros(10, F32), off, [0])
    with pytest.raises(ValueError, match="1-D or 2-D"):
        nn.take_rows(np.zeros((2, 2, 2), F32), [0])
    assert nn.check_take(np.array([3.0, 0.0]), 4).dtype == np.int64
    assert nn.check_take([], 4).shape == (0,)


class _Comm:
    """A communicator that is never used: the checks come first."""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world

    def trainer_comm_desc(self):  # pragma: no cover
        raise AssertionError("a device call before the checks")


def _toy(S=10, seed=0):
    from tests.flowcases import build_flow
    from zenflow_amd import nn

    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 6, S)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    X = rng.standard_normal((int(off[-1]), 2)).astype(F32)
    Y = rng.standard_normal((S, 2)).astype(F32)
    flow = build_flow(dict(D=2, C=3, K=8, layers=(32, 32), latent="beta"))
    phi = nn.ConditionNet(3, layers=(16, 16), pool="sum")
    return flow, phi, X, off, Y


def test_train_sets_checks_before_any_device_call():
    from zenflow_amd import nn
    from zenflow_amd.train import train_sets

    flow, phi, X, off, Y = _toy()
    kw = dict(epochs=2, progress=False)
    with pytest.raises(ValueError, match="Y_train has 9 rows for the 10 sets"):
        train_sets(flow, phi, X, off, Y[:9], X, off, Y, **kw)
    with pytest.raises(ValueError, match="Y_test has 9 rows"):
        train_sets(flow, phi, X, off, Y, X, off, Y[:9], **kw)
    with pytest.raises(ValueError, match="batch_sets"):
        train_sets(flow, phi, X, off, Y, X, off, Y, batch_sets=0, **kw)
    with pytest.raises(ValueError, match="pooled"):
        train_sets(flow, nn.ConditionNet(3, layers=(16,), pool=None), X, off, Y, X, off, Y, **kw)
    # S = 10 in batches of 3 leaves a last batch of 1 set for 4 ranks
    with pytest.raises(ValueError, match=r"S = 10 .*batch_sets = 3 .*world = 4"):
        train_sets(flow, phi, X, off, Y, X, off, Y, batch_sets=3, comm=_Comm(1, 4), **kw)
    with pytest.raises(ValueError, match="offsets"):
        train_sets(flow, phi, X, off[::-1], Y, X, off, Y, **kw)
    with pytest.raises(ValueError, match="2-D"):
        train_sets(flow, phi, X[:, 0], off, Y, X, off, Y, **kw)
    with pytest.raises(ValueError, match="2-D"):
        train_sets(flow, phi, X, off, Y[:, 0], X, off, Y, **kw)
    with pytest.raises(ValueError, match="columns"):
        train_sets(flow, phi, X, off, Y, X[:, :1], off, Y, **kw)
    # empty sets that could fill a shard: rejected up front
    off0 = np.concatenate([off, [off[-1]] * 2])
    Y0 = np.concatenate([Y, Y[:2]])
    with pytest.raises(ValueError, match="empty sets"):
        train_sets(flow, phi, X, off0, Y0, X, off, Y, batch_sets=4, comm=_Comm(0, 2), **kw)


def _brute_force(lengths, batch_sets, world, seeds):
    """The largest shard (sets, element rows) over the epochs of ``seeds``, by train_sets' own cutting rule."""
    from zenflow_amd.dist import shard_rows

    S, most_sets, most_rows = len(lengths), 0, 0
    for seed in seeds:
        perm = np.random.default_rng([seed, 0]).permutation(S)
        for first in range(0, S, batch_sets):
            batch = perm[first:first + batch_sets]
            for rank in range(world):
                lo, hi = shard_rows(len(batch), rank, world)
                most_sets = max(most_sets, hi - lo)
                most_rows = max(most_rows, int(lengths[batch[lo:hi]].sum()))
    return most_sets, most_rows


@pytest.mark.parametrize("S,batch_sets,world", [(96, 40, 1), (96, 40, 2), (37, 8, 3), (10, 64, 1), (64, 16, 4)])
def test_batch_plan_bounds_every_batch(S, batch_sets, world):
    from zenflow_amd.train import plan_set_batches

    rng = np.random.default_rng(S + batch_sets)
    lengths = rng.integers(1, 13, S)
    lengths[rng.integers(0, S)] = 300  # one long set
    off = np.concatenate([[0], np.cumsum(lengths)])
    sizes, sets_max, rows_max = plan_set_batches(off, batch_sets, world)
    assert sum(sizes) == S and all(n == min(batch_sets, S) for n in sizes[:-1]) and 1 <= sizes[-1] <= batch_sets
    assert sizes == [len(range(k, min(S, k + batch_sets))) for k in range(0, S, batch_sets)]
    most_sets, most_rows = _brute_force(lengths, batch_sets, world, range(6))
    assert most_sets == sets_max  # the first batch's largest shard has exactly that many
    assert most_rows <= rows_max == int(np.sort(lengths)[-sets_max:].sum())
    # the bound is attained by the permutation that puts the longest sets into one shard
    assert rows_max <= int(lengths.sum())


def test_batch_plan_rejects():
    from zenflow_amd.train import plan_set_batches

    off = np.arange(11)
    with pytest.raises(ValueError, match="batch_sets"):
        plan_set_batches(off, 0)
    with pytest.raises(ValueError, match=r"S = 10 .*batch_sets = 3 .*world = 4"):
        plan_set_batches(off, 3, 4)
    assert plan_set_batches(off, 5, 4) == ([5, 5], 2, 2)
    with pytest.raises(ValueError, match="empty sets"):
        plan_set_batches([0, 0, 1, 2, 3], 2, 2)  # one empty set, shards of one set
    assert plan_set_batches([0, 0, 1, 2, 3], 4, 2) == ([4], 2, 2)
