"""Deep sets on the GPU (zenflow_amd/nn.py, zf_condnet_backward_input,
zf_segment_repeat): the input gradient of a conditioning network, a second
network ``rho`` trained behind ``phi`` (examples/deep_set.ipynb, ``class
DeepSet`` / ``loss_fn`` / ``step``), a ``rho`` between the pooled sum and the
flow, and ``jnp.repeat(c, sizes, axis=0)`` of ``DeepSetFlow.sample`` on the
device, against the float64 / float32 oracle of tests/deepset_oracle.py.

The batches are tests/test_gpu_condnet.py's: set lengths 1, 0, 63, 64, 65,
chunk - 1, chunk, chunk + 1, 2 chunk + 76, and 37 trailing padding rows.

The parity rule is the project's own (tests/test_gpu_train.py::
test_train_gradient_per_parameter), per tensor and with nothing left out:
    |v_gpu - v64| <= 1e-5 max|v64| + 2 max(|v32 - v64|, |v64' - v64|)
with v32 the float32 oracle over three row orders and v64' float64 at inputs
and parameters jittered by 2^-22 relative."""

import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

from tests import condnet_oracle as CO
from tests import deepset_oracle as DO
from tests.test_gpu_condnet import GRAD_CASES, PAD, _batch, _cfg, _check, _chunk, _flow_case, _leaves, _net, _offsets

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
F32 = np.float32


def _oracle(net, variables, x, off, mode="net", rnet=None, rvariables=None, **extra):
    """The oracle's result for one job, from its CPU-only child process."""
    rows, S = len(x), len(off) - 1
    with tempfile.TemporaryDirectory() as d:
        job, out = Path(d) / "job.npz", Path(d) / "out.npz"
        DO.pack_job(job, _cfg(net), variables, x, CO.ids_of(off, rows), S, mode=mode,
                    rcfg=None if rnet is None else _cfg(rnet), rvariables=rvariables, **extra)
        subprocess.run([sys.executable, "-m", "tests.deepset_oracle", str(job), str(out)], cwd=ROOT, check=True,
                       timeout=600)
        return dict(np.load(out))


def _record(rec):
    from tests.test_gpu_flow import _append_record

    _append_record("deepset_parity.jsonl", rec)


def _check_tree(ref, name, tree, bad, rec):
    assert set(f"{name}64:" + k for k in tree) == set(k for k in ref if k.startswith(f"{name}64:"))
    for k, a in tree.items():
        _check(ref, name, ":" + k, a, bad, rec)


# ---- d / d x of one network -------------------------------------------------------------------
@pytest.mark.parametrize("F,in_dim,dropout,batch_norm,pool", GRAD_CASES)
def test_input_gradient(F, in_dim, dropout, batch_norm, pool):
    """ConditionTrainer.backward(gc, input_grad=True) for a random cotangent:
    every element of gx (and of every parameter gradient) against float64
    autograd; g has the bits of backward(gc) on an identical pass; an identical
    pass gives the same gx bits; without BatchNorm the padding rows of a pooled
    network get exactly zero (with it they carry the batch terms)."""
    from zenflow_amd import nn

    net, v = _net(F, in_dim, dropout=dropout, batch_norm=batch_norm, pool=pool, seed=10 * F + in_dim)
    x, off, rows = _batch(in_dim, 3 * F + in_dim)
    seed = 2**40 + 5
    n_out = len(off) - 1 if pool == "sum" else rows
    gc = np.random.default_rng(5).standard_normal((n_out, F)).astype(F32)
    keep = nn.dropout_keep(seed, rows, F, dropout) if dropout else None
    ref = _oracle(net, v, x, off, keep=keep, gc=gc)
    ct_ = nn.ConditionTrainer(net, v, in_dim, rows)
    offs = off if pool == "sum" else None
    c = ct_.forward(x, offs, seed=seed)
    g, gx = ct_.backward(gc, input_grad=True)
    assert gx.dtype == F32 and gx.shape == (rows, in_dim)
    assert g.dtype == F32 and g.shape == (ct_.layout.size,)
    bad, rec = [], {"what": "input gradient", "F": F, "in_dim": in_dim, "dropout": dropout, "batch_norm": batch_norm,
                    "pool": pool}
    _check(ref, "c", "", c, bad, rec)
    _check(ref, "gx", "", gx, bad, rec)
    _check_tree(ref, "g", _leaves(ct_.grad_tree(g)), bad, rec)
    _record(rec)
    assert not bad, bad
    # the parameter gradient of the plain entry on an identical pass: the same bits
    ct_.forward(x, offs, seed=seed)
    assert np.array_equal(ct_.backward(gc), g)
    # an identical pass again: the same gx bits (and g once more)
    ct_.forward(x, offs, seed=seed)
    g2, gx2 = ct_.backward(gc, input_grad=True)
    assert np.array_equal(gx2, gx) and np.array_equal(g2, g)
    if pool == "sum":
        if batch_norm:
            assert gx[-PAD:].any()  # padding rows are in the statistics
        else:
            assert not gx[-PAD:].any()


# ---- rho behind phi ---------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [3, 8])
def test_stack_gradient(F):
    """phi (BatchNorm, dropout 0.3, sum) -> rho (no BatchNorm, per row) under a
    random cotangent on rho's output, all on DeviceArrays: rho's gradient,
    phi's gradient and phi's gx against float64 autograd of the composition."""
    from zenflow_amd import _lib as L
    from zenflow_amd import nn

    in_dim = 2
    phi, pv = _net(F, in_dim, dropout=0.3, seed=110 + F)
    rho, rv = _net(1, F, batch_norm=False, pool=None, seed=120 + F)
    x, off, rows = _batch(in_dim, 130 + F)
    S = len(off) - 1
    seed = 17
    gy = np.random.default_rng(6).standard_normal((S, 1)).astype(F32)
    ref = _oracle(phi, pv, x, off, mode="stack", rnet=rho, rvariables=rv, keep=nn.dropout_keep(seed, rows, F, 0.3),
                  gy=gy)
    pt, rt = nn.ConditionTrainer(phi, pv, in_dim, rows, sets_max=S), nn.ConditionTrainer(rho, rv, F, S)
    c = pt.forward(L.DeviceArray.from_numpy(x), L.DeviceArray.from_numpy(off), seed=seed)
    yp = rt.forward(c)
    assert isinstance(yp, L.DeviceArray) and yp.shape == (S, 1)
    rg, gc = rt.backward(L.DeviceArray.from_numpy(gy), input_grad=True)
    assert isinstance(gc, L.DeviceArray) and gc.shape == (S, F) and isinstance(rg, L.DeviceArray)
    g, gx = pt.backward(gc, input_grad=True)
    assert isinstance(gx, L.DeviceArray) and gx.shape == (rows, in_dim)
    bad, rec = [], {"what": "stack gradient", "F": F}
    _check(ref, "c", "", c.numpy(), bad, rec)
    _check(ref, "y", "", yp.numpy(), bad, rec)
    _check_tree(ref, "rg", _leaves(rt.grad_tree(rg.numpy())), bad, rec)
    _check_tree(ref, "g", _leaves(pt.grad_tree(g.numpy())), bad, rec)
    _check(ref, "gx", "", gx.numpy(), bad, rec)
    _record(rec)
    assert not bad, bad


def test_flow_behind_rho():
    """A rho between the pooled sum and the flow: tr.loss_grad(Y, c2,
    cond_grad=True) -> rho.backward(gc, input_grad=True) -> phi.backward(...),
    phi's (and rho's) gradient against float64 autograd of the whole loss."""
    from tests.flowcases import _trainer
    from zenflow_amd import _lib as L
    from zenflow_amd import nn

    in_dim, Fp, C = 2, 8, 3
    phi, pv = _net(Fp, in_dim, dropout=0.3, seed=140)
    rho, rv = _net(C, Fp, batch_norm=False, pool=None, seed=141)
    x, off, rows = _batch(in_dim, 142, extra_sets=[5, 9, 2, 31] * 6)
    S = len(off) - 1
    case = _flow_case(C, S, 143)
    seed = 9
    ref = _oracle(phi, pv, x, off, mode="flow", rnet=rho, rvariables=rv, keep=nn.dropout_keep(seed, rows, Fp, 0.3),
                  model=case["model"], flow_variables=case["variables"], y=case["x"])
    pt, rt = nn.ConditionTrainer(phi, pv, in_dim, rows, sets_max=S), nn.ConditionTrainer(rho, rv, Fp, S)
    tr = _trainer(case, S)
    c = pt.forward(L.DeviceArray.from_numpy(x), L.DeviceArray.from_numpy(off), seed=seed)
    c2 = rt.forward(c)
    loss, _, gc = tr.loss_grad(L.DeviceArray.from_numpy(case["x"]), c2, cond_grad=True)
    rg, gc1 = rt.backward(gc, input_grad=True)
    g = pt.backward(gc1)
    assert loss == pytest.approx(float(ref["loss64"]), rel=2e-5, abs=2e-5)
    bad, rec = [], {"what": "flow behind rho", "F": Fp, "C": C}
    _check(ref, "y", "", c2.numpy(), bad, rec)
    _check_tree(ref, "g", _leaves(pt.grad_tree(g.numpy())), bad, rec)
    # rho's gradient too, but for its last bias: the flow's first layer is a train-mode BatchNorm over [y, c2], so
    # a constant added to a column of c2 changes nothing and that gradient is zero analytically (1e-17 in float64,
    # rounding in any float32 order): there is no scale to hold it to
    rtree = _leaves(rt.grad_tree(rg.numpy()))
    last = f"NNBlock_0/Dense_{len(rho.layers)}/bias"
    gmax = max(np.abs(a).max() for a in rtree.values())
    assert np.abs(ref["rg64:" + last]).max() <= 1e-12 * gmax
    for k, a in rtree.items():
        if k != last:
            _check(ref, "rg", ":" + k, a, bad, rec)
    _record(rec)
    assert not bad, bad


def test_deep_set_regression_lowers_the_loss():
    """The notebook's first half as the documentation writes it (DeepSet /
    loss_fn / step: Phi, then rho, under optax.l2_loss), on its toy mapping at
    small size: sets of 1 - 39 elements, ym = sqrt(n).  Only yp (S floats)
    touches the host."""
    from zenflow_amd import _lib as L
    from zenflow_amd import nn
    from zenflow_amd._lib import DeviceArray

    rng = np.random.default_rng(181)
    S = 200
    n = rng.integers(1, 40, S)
    off = _offsets(n)
    rows = int(off[-1]) + PAD
    X = np.concatenate([rng.standard_normal((int(off[-1]), 2)), np.zeros((PAD, 2))]).astype(F32)
    ym = np.sqrt(n)
    phi = nn.ConditionNet(8, layers=(32, 32), dropout=0.3, pool="sum")
    rho = nn.ConditionNet(1, layers=(32, 32), batch_norm=False, pool=None)
    pv, rv = phi.init(3, X, off), rho.init(4, np.zeros((S, 8), F32))
    pt, rt = nn.ConditionTrainer(phi, pv, 2, rows, sets_max=S), nn.ConditionTrainer(rho, rv, 8, S)
    Xd, off_d = L.DeviceArray.from_numpy(X), L.DeviceArray.from_numpy(off)
    losses = []
    for epoch in range(40):
        c = pt.forward(Xd, off_d, seed=epoch)
        yp = rt.forward(c)
        r = yp.numpy()[:, 0] - ym
        losses.append(float(np.mean(0.5 * r * r)))  # mean(optax.l2_loss(yp, ym))
        gy = DeviceArray.from_numpy((r / S).astype("f4")[:, None])
        pt.step(rt.step(gy, input_grad=True))
    assert np.isfinite(losses).all() and np.mean(losses[-5:]) < np.mean(losses[:5]), losses
    for tr_, start in ((pt, pv), (rt, rv)):
        moved = _leaves(tr_.variables()["params"])
        assert any(not np.array_equal(moved[k], a) for k, a in _leaves(start["params"]).items())


# ---- the repeat ----------------------------------------------------------------------------------------
def _repeat_entry(c, off, rows, want_index=True):
    """zf_segment_repeat itself on device copies of c (S, F) and off (any int64s)."""
    from zenflow_amd import _lib as L

    lib = L.load_library()
    S, F = c.shape
    cd = L.DeviceArray.from_numpy(np.ascontiguousarray(c, F32))
    od = L.DeviceArray.from_numpy(np.ascontiguousarray(off, np.int64))
    out = L.DeviceArray((rows, F))
    idx = L.DeviceArray((rows,), np.int32) if want_index else None
    ws = L.DeviceArray((lib.zf_segment_workspace_bytes(rows, S, F),), np.uint8)
    L.check(lib.zf_segment_repeat(cd.ptr, S, F, od.ptr, rows, out.ptr, None if idx is None else idx.ptr, ws.ptr,
                                  L.stream()), "zf_segment_repeat")
    return (out.numpy(), idx.numpy()) if want_index else out.numpy()


def _host_repeat(c, off, rows):
    ids = CO.ids_of(off, rows)
    return np.where(ids[:, None] >= 0, c[np.maximum(ids, 0)], F32(0)), ids


@pytest.mark.parametrize("F", [3, 8, 64])
def test_segment_repeat(F):
    """out[i] = c[set(i)], bit for bit, and +0 for rows in no set."""
    from zenflow_amd import _lib as L
    from zenflow_amd import nn

    rng = np.random.default_rng(200 + F)
    lengths = [1, 0, 63, 64, 65, _chunk() - 1, _chunk(), _chunk() + 1, 2 * _chunk() + 76]
    off = _offsets(lengths)
    S = len(lengths)
    rows = int(off[-1]) + PAD
    c = rng.standard_normal((S, F)).astype(F32)
    want, ids = _host_repeat(c, off, rows)
    out = nn.segment_repeat(c, off, rows=rows)
    assert isinstance(out, np.ndarray) and out.dtype == F32 and np.array_equal(out, want)
    assert not out[-PAD:].any() and not np.signbit(out[-PAD:]).any()
    assert np.array_equal(nn.segment_repeat(c, off), want[:off[-1]])  # rows defaults to the last offset
    outd = nn.segment_repeat(L.DeviceArray.from_numpy(c), L.DeviceArray.from_numpy(off), rows=rows)
    assert isinstance(outd, L.DeviceArray) and np.array_equal(outd.numpy(), want)
    got, idx = _repeat_entry(c, off, rows)
    assert np.array_equal(got, want) and np.array_equal(idx, ids.astype(np.int32))
    # offsets that start above 0: leading rows in no set
    off5 = off + 5
    want5, ids5 = _host_repeat(c, off5, rows + 5)
    got5, idx5 = _repeat_entry(c, off5, rows + 5)
    assert np.array_equal(got5, want5) and np.array_equal(idx5, ids5.astype(np.int32)) and not got5[:5].any()
    assert np.array_equal(nn.segment_repeat(c, off5, rows=rows + 5), want5)
    # repeats: np.repeat itself
    assert np.array_equal(nn.segment_repeat(c, repeats=5), np.repeat(c, 5, axis=0))
    r = np.array([3, 0, 0, 7, 1, 0, 600, 2, 0])
    assert np.array_equal(nn.segment_repeat(c, repeats=r), np.repeat(c, r, axis=0))
    padded = nn.segment_repeat(c, repeats=r, rows=int(r.sum()) + 3)
    assert np.array_equal(padded[:-3], np.repeat(c, r, axis=0)) and not padded[-3:].any()


def test_segment_repeat_clamps_bad_device_offsets():
    """The bad device offsets of tests/test_gpu_condnet.py::
    test_segment_sum_clamps_bad_device_offsets: what clamp_offsets makes of
    them, finite, and the index zf_segment_sum writes."""
    from zenflow_amd import _lib as L
    from zenflow_amd import nn

    rng = np.random.default_rng(231)
    rows, F = 700, 3
    for bad in ([5, -3, 70, 40, 10**12, 200], [-(2**62), 2**62, 0, 10], [900, 800, 100], [0, 650, 2**40],
                [3, 3, 3, 2, 699, 701]):
        S = len(bad) - 1
        c = rng.standard_normal((S, F)).astype(F32)
        got, idx = _repeat_entry(c, np.asarray(bad, np.int64), rows)
        o = nn.clamp_offsets(bad, rows)
        want, ids = _host_repeat(c, o, rows)
        assert np.isfinite(got).all() and np.array_equal(got, want), bad
        assert np.array_equal(idx, ids.astype(np.int32)) and np.array_equal(ids, CO.ids_of(bad, rows))
        assert np.array_equal(_repeat_entry(c, o, rows)[0], want)
        viad = nn.segment_repeat(L.DeviceArray.from_numpy(c), L.DeviceArray.from_numpy(np.asarray(bad, np.int64)),
                                 rows=rows)
        assert np.array_equal(viad.numpy(), want)
        # the index is the one zf_segment_sum writes for the same offsets
        from tests.test_gpu_condnet import _segment_sum

        assert np.array_equal(_segment_sum(np.zeros((rows, F), F32), np.asarray(bad, np.int64), want_index=True)[1], idx)


def test_segment_repeat_one_long_set_among_short_ones():
    """One set of 10^5 rows among 300 sets of tens (correctness only)."""
    from zenflow_amd import nn

    rng = np.random.default_rng(232)
    r = rng.integers(10, 100, 301)
    r[137] = 100_000
    c = rng.standard_normal((301, 8)).astype(F32)
    assert np.array_equal(nn.segment_repeat(c, repeats=r), np.repeat(c, r, axis=0))


@pytest.mark.parametrize("F", [3, 8])
def test_segment_repeat_and_sum_are_adjoint(F):
    """sum(repeat(c) * h) = sum(c * segment_sum(h)).  The repeat is a copy, so
    in float64 the left side is sum(c * s64) with s64 the float64 sum of each
    set's rows of h; the right side has the device's fp32 sums s32 in its
    place.  The two differ by at most sum(|c| |s32 - s64|), the summation's own
    error as measured, plus the float64 rounding of the two evaluations."""
    from zenflow_amd import nn

    rng = np.random.default_rng(240 + F)
    lengths = [1, 0, 63, 64, 65, _chunk() - 1, _chunk(), _chunk() + 1, 2 * _chunk() + 76]
    off = _offsets(lengths)
    rows = int(off[-1]) + PAD
    c = rng.standard_normal((len(lengths), F)).astype(F32)
    h = rng.standard_normal((rows, F)).astype(F32)
    rep = nn.segment_repeat(c, off, rows=rows).astype(np.float64)
    s32 = nn.segment_sum(h, off).astype(np.float64)
    h64, c64 = h.astype(np.float64), c.astype(np.float64)
    s64 = np.stack([h64[off[s]:off[s + 1]].sum(axis=0) for s in range(len(lengths))])
    lhs, rhs = (rep * h64).sum(), (c64 * s32).sum()
    bound = (np.abs(c64) * np.abs(s32 - s64)).sum() + 2.0**-40 * (np.abs(rep) * np.abs(h64)).sum()
    print(f"adjointness F={F}: |lhs - rhs| {abs(lhs - rhs):.3g}, bound {bound:.3g}")
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    assert s32.shape == (len(lengths), F) and not s32[1].any()


def test_sample_through_repeat():
    """DeepSetFlow.sample: the flow's samples at nn.segment_repeat(c_dev,
    repeats=5) have the bits of those at np.repeat(c, 5, axis=0)."""
    from tests.flowcases import build_flow
    from zenflow_amd import _lib as L
    from zenflow_amd import nn

    F, in_dim = 3, 2
    phi, pv = _net(F, in_dim, dropout=0.3, seed=150)
    x, off, rows = _batch(in_dim, 151)
    case = _flow_case(F, 8, 152)
    flow = build_flow(case["cfg"])
    flow.latent._dim = case["cfg"]["D"]
    fv = case["variables"]
    c_dev = phi.apply(pv, L.DeviceArray.from_numpy(x), L.DeviceArray.from_numpy(off))
    assert isinstance(c_dev, L.DeviceArray)
    rep = nn.segment_repeat(c_dev, repeats=5)
    assert isinstance(rep, L.DeviceArray) and rep.shape == (5 * (len(off) - 1), F)
    y = flow.apply(fv, rep, seed=0, method="sample")
    assert isinstance(y, L.DeviceArray)
    want = flow.apply(fv, np.repeat(c_dev.numpy(), 5, axis=0), seed=0, method="sample")
    assert y.shape == want.shape == (5 * (len(off) - 1), 2)
    assert np.array_equal(y.numpy(), want, equal_nan=True) and np.isfinite(want).any()


# ---- rejections ------------------------------------------------------------------------------------------
def test_rejections():
    from zenflow_amd import _lib as L
    from zenflow_amd import nn

    net, v = _net(3, 2, seed=199)
    x, off, rows = _batch(2, 198)
    S = len(off) - 1
    ct_ = nn.ConditionTrainer(net, v, 2, rows, sets_max=S)
    gc = np.zeros((S, 3), F32)
    with pytest.raises(ValueError, match="pending"):
        ct_.backward(gc, input_grad=True)
    with pytest.raises(ValueError, match="pending"):
        ct_.step(gc, input_grad=True)
    ct_.forward(x, off, train=False)  # eval mode leaves nothing pending
    with pytest.raises(ValueError, match="pending"):
        ct_.backward(gc, input_grad=True)
    ct_.forward(x, off)
    with pytest.raises(ValueError):  # the wrong shape of gc keeps the pass pending
        ct_.backward(np.zeros((S + 1, 3), F32), input_grad=True)
    g, gx = ct_.backward(gc, input_grad=True)
    assert not g.any() and not gx.any() and gx.shape == (rows, 2)
    with pytest.raises(ValueError, match="pending"):  # one reverse per forward, through either entry
        ct_.backward(gc)
    ct_.forward(x, off)
    ct_.backward(gc)
    with pytest.raises(ValueError, match="pending"):
        ct_.backward(gc, input_grad=True)
    # the C entry itself
    lib = L.load_library()
    xd, od = L.DeviceArray.from_numpy(x), L.DeviceArray.from_numpy(off)
    out, gcd = L.DeviceArray((S, 3)), L.DeviceArray.from_numpy(gc)
    gxd = L.DeviceArray((rows, 2))
    assert lib.zf_condnet_backward_input(ct_.handle, gcd.ptr, None, gxd.ptr, L.stream()) == -1
    assert b"no forward pending" in lib.zf_last_error()
    assert lib.zf_condnet_forward(ct_.handle, xd.ptr, rows, od.ptr, S, 0, 0, 0, out.ptr, L.stream()) == 0
    assert lib.zf_condnet_backward_input(ct_.handle, gcd.ptr, None, gxd.ptr, L.stream()) == -1  # after an eval forward
    assert lib.zf_condnet_forward(ct_.handle, xd.ptr, rows, od.ptr, S, 1, 1, 0, out.ptr, L.stream()) == 0
    assert lib.zf_condnet_backward_input(ct_.handle, gcd.ptr, None, None, L.stream()) == -1  # NULL gx_out
    assert b"gx_out" in lib.zf_last_error()
    assert lib.zf_condnet_backward_input(ct_.handle, None, None, gxd.ptr, L.stream()) == -1  # NULL gc
    # ... and the pass is still pending: a following backward succeeds, once
    assert lib.zf_condnet_backward(ct_.handle, gcd.ptr, None, L.stream()) == 0
    assert lib.zf_condnet_backward(ct_.handle, gcd.ptr, None, L.stream()) == -1
    assert lib.zf_condnet_forward(ct_.handle, xd.ptr, rows, od.ptr, S, 1, 1, 0, out.ptr, L.stream()) == 0
    assert lib.zf_condnet_backward_input(ct_.handle, gcd.ptr, None, None, L.stream()) == -1
    assert lib.zf_condnet_backward_input(ct_.handle, gcd.ptr, None, gxd.ptr, L.stream()) == 0
    assert lib.zf_condnet_backward_input(ct_.handle, gcd.ptr, None, gxd.ptr, L.stream()) == -1
    L.synchronize()
