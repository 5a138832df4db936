"""The forwarding lattice of the trainer's eight loss_grad / step entries,
pinned at the C ABI (include/zenflow_amd.h): weighted -> cond -> shard ->
plain.  ``w == NULL`` is the unweighted loss, ``gc == NULL`` or ``C == 0``
writes no gc (and the step may replay its graph), the plain entries use
``global_rows = B * world``.  Everything is compared bit for bit: one trainer
per entry, built from the same variables, on the same batch."""

import functools

import numpy as np
import pytest

from tests.flowcases import _blob, _trainer, make_case
from tests.weighted_grad_oracle import make_weights
from zenflow_amd import _lib as L
from zenflow_amd._lib import DeviceArray

pytestmark = pytest.mark.gpu

CASES = {"cfg4": ("cfg4", 128, 63), "small": ("small", 73, 90)}  # C = 2, C = 0
ENTRIES = ["", "_shard", "_cond_shard", "_weighted_shard"]
SENTINEL = np.float32(-1234.5)


@functools.lru_cache(maxsize=None)
def _case(key):
    name, N, seed = CASES[key]
    case = make_case(name, N=N, seed=seed)
    assert (case["cfg"]["C"] > 0) == (key == "cfg4")
    return case, N, seed


def _inputs(case):
    xd = DeviceArray.from_numpy(case["x"])
    cd = None if case["c"] is None else DeviceArray.from_numpy(case["c"])
    return xd, cd


def _ptr(a):
    return None if a is None else a.ptr


def _bits(a):
    return a.numpy().view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _call(kind, suffix, tr, xd, cd, outs, w=None, gc=None, global_rows=None):
    """One call of ``zf_trainer_<kind><suffix>`` on the whole batch; ``outs``:
    the arguments between the row counts and gc (update_stats, loss, grad)."""
    rows = xd.shape[0]
    counts = (rows,) if suffix == "" else (rows, rows if global_rows is None else global_rows)
    args = (xd.ptr, _ptr(cd)) + ((_ptr(w),) if suffix == "_weighted_shard" else ()) + counts + outs
    if suffix in ("_cond_shard", "_weighted_shard"):
        args += (_ptr(gc),)
    name = f"zf_trainer_{kind}{suffix}"
    L.check(getattr(L.load_library(), name)(tr.handle, *args, L.stream()), name)


def _loss_grad(key, suffix, w=None, gc=None):
    """(loss bits, gradient bits) of one entry on a fresh trainer, update_stats = 0."""
    case, N, _ = _case(key)
    tr = _trainer(case, N)
    xd, cd = _inputs(case)
    loss, g = DeviceArray((1,), np.float64), DeviceArray((tr.program.blob.size,))
    _call("loss_grad", suffix, tr, xd, cd, (0, loss.ptr, g.ptr), w=w, gc=gc)
    return _bits(loss)[0], _bits(g)


def _step(key, suffix, w=None, gc=None, steps=2):
    """(loss bits of every step, blob bits after the last) of one entry on a fresh trainer."""
    case, N, _ = _case(key)
    tr = _trainer(case, N)
    xd, cd = _inputs(case)
    loss, losses = DeviceArray((1,), np.float64), []
    for _ in range(steps):
        _call("step", suffix, tr, xd, cd, (loss.ptr,), w=w, gc=gc)
        losses.append(_bits(loss)[0])
    return losses, _blob(tr).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("key", list(CASES))
def test_loss_grad_entries_agree(key):
    """The four entries without gc and without weights: the same loss and
    gradient bits; on the conditional case, the two entries that take a gc
    also agree on it and leave loss and gradient as they are."""
    plain = _loss_grad(key, "")
    assert np.isfinite(np.uint64(plain[0]).view(np.float64)) and plain[1].any()
    for suffix in ENTRIES[1:]:
        assert _same(_loss_grad(key, suffix), plain), suffix
    if key != "cfg4":
        return
    case, N, _ = _case(key)
    gcs = []
    for suffix in ENTRIES[2:]:
        gc = DeviceArray.from_numpy(np.full((N, case["cfg"]["C"]), SENTINEL))
        assert _same(_loss_grad(key, suffix, gc=gc), plain), suffix
        gcs.append(_bits(gc))
    assert np.array_equal(gcs[0], gcs[1])
    assert not (gcs[0] == SENTINEL.view(np.uint32)).any() and np.isfinite(gcs[0].view(np.float32)).all()


@pytest.mark.parametrize("key", list(CASES))
def test_step_entries_agree_graph_and_eager(key, monkeypatch):
    """Two steps through each of the four entries, with the captured graph
    (ZF_TRAIN_GRAPH unset) and eagerly (=0): eight times the same loss and
    blob bits."""
    out = []
    for graph in (None, "0"):
        if graph is None:
            monkeypatch.delenv("ZF_TRAIN_GRAPH", raising=False)
        else:
            monkeypatch.setenv("ZF_TRAIN_GRAPH", graph)
        out += [_step(key, suffix) for suffix in ENTRIES]
    assert len(out) == 8
    assert np.isfinite(np.array(out[0][0], np.uint64).view(np.float64)).all()
    first = _trainer(*_case(key)[:2])
    assert not np.array_equal(out[0][1], _blob(first).view(np.uint32))  # the steps moved the blob
    for k, o in enumerate(out[1:], 1):
        assert o[0] == out[0][0] and np.array_equal(o[1], out[0][1]), (k, ENTRIES[k % 4])


def test_unconditional_flow_ignores_gc():
    """C == 0 with a non-NULL gc: nothing is written through it, the results
    are the plain entries', and the weighted step's are those of the weighted
    step without gc (gc is dropped before graph or eager is chosen)."""
    key = "small"
    _, N, seed = _case(key)
    gc = DeviceArray.from_numpy(np.full(16, SENTINEL))
    plain_lg, plain_st = _loss_grad(key, ""), _step(key, "")
    for suffix in ENTRIES[2:]:
        assert _same(_loss_grad(key, suffix, gc=gc), plain_lg), suffix
        got = _step(key, suffix, gc=gc)
        assert got[0] == plain_st[0] and np.array_equal(got[1], plain_st[1]), suffix
    w = DeviceArray.from_numpy(make_weights(N, seed))
    a, b = _step(key, "_weighted_shard", w=w, gc=gc), _step(key, "_weighted_shard", w=w)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert a[0] != plain_st[0]  # the weights did enter
    assert np.array_equal(_bits(gc), np.full(16, SENTINEL).view(np.uint32))


def test_failed_call_leaves_the_trainer_usable():
    """One device, global_rows = rows + 1: ValueError naming global_rows; the
    valid step after it has the bits of a fresh trainer's first step."""
    key = "cfg4"
    case, N, _ = _case(key)
    tr = _trainer(case, N)
    xd, cd = _inputs(case)
    loss = DeviceArray((1,), np.float64)
    with pytest.raises(ValueError, match="global_rows"):
        _call("step", "_shard", tr, xd, cd, (loss.ptr,), global_rows=N + 1)
    _call("step", "_shard", tr, xd, cd, (loss.ptr,))
    fresh = _step(key, "_shard", steps=1)
    assert _bits(loss)[0] == fresh[0][0]
    assert np.array_equal(_blob(tr).view(np.uint32), fresh[1])
