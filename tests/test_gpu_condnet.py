"""Conditioning networks on the GPU (zenflow_amd/nn.py, zf_condnet_*,
zf_segment_*): the standalone segment sum / broadcast, dropout, forward and
gradient parity against the float64 / float32 oracle of
tests/condnet_oracle.py, the joint gradient through a conditional flow, the
optimiser trajectory, the module protocol and the rejections.

Set lengths of every batch: 1, 0, 63, 64, 65, the kernel's chunk length - 1,
the chunk length, the chunk length + 1, one set longer than two chunks, and
trailing padding rows that belong to no set.

The parity rule is the project's own (tests/test_gpu_train.py::
test_train_gradient_per_parameter), per tensor:
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

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
F32 = np.float32
ACTS = ["swish", "relu", "tanh", "sigmoid", "gelu", "softplus", "elu", "leaky_relu"]


def _chunk():
    from zenflow_amd import _lib as L

    return L.ZF_SEG_CHUNK


def _lengths():
    k = _chunk()
    return [1, 0, 63, 64, 65, k - 1, k, k + 1, 2 * k + 76]


PAD = 37  # trailing rows in no set


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


# ---- the standalone entries ----------------------------------------------------------
def _segment_sum(h, off, rate=0.0, seed=0, want_index=False):
    """zf_segment_sum on device copies of h (rows, F) and off (any int64s)."""
    from zenflow_amd import _lib as L

    lib = L.load_library()
    rows, F = h.shape
    S = len(off) - 1
    hd = L.DeviceArray.from_numpy(np.ascontiguousarray(h, F32))
    od = L.DeviceArray.from_numpy(np.ascontiguousarray(off, np.int64))
    out = L.DeviceArray((S, F))
    idx = L.DeviceArray((rows,), np.int32) if want_index else None
    ws = L.DeviceArray((lib.zf_segment_workspace_bytes(rows, S, F),), np.uint8)
    L.check(lib.zf_segment_sum(hd.ptr, rows, F, od.ptr, S, rate, seed, out.ptr, None if idx is None else idx.ptr,
                               ws.ptr, L.stream()), "zf_segment_sum")
    return (out.numpy(), idx.numpy()) if want_index else out.numpy()


def _segment_bcast(gc, idx, F, rate=0.0, seed=0):
    from zenflow_amd import _lib as L

    rows, S = len(idx), len(gc)
    gd = L.DeviceArray.from_numpy(np.ascontiguousarray(gc, F32))
    idd = L.DeviceArray.from_numpy(np.ascontiguousarray(idx, np.int32))
    out = L.DeviceArray((rows, F))
    L.check(L.load_library().zf_segment_bcast(gd.ptr, idd.ptr, rows, F, S, rate, seed, out.ptr, L.stream()),
            "zf_segment_bcast")
    return out.numpy()


@pytest.mark.parametrize("F", [3, 8])
def test_segment_sum_against_float64(F):
    """Every element within the worst-case bound of ANY fp32 summation order,
    |s - s64| <= (n - 1) 2^-24 sum|h_i| (Jeannerod & Rump 2013: no higher-order
    term), times (1 + 2^-20) for the float64 reference's own rounding: derived,
    not measured.  Empty sets are zero rows; the row index is the host's."""
    rng = np.random.default_rng(10 + F)
    lengths = _lengths()
    off = _offsets(lengths)
    rows = int(off[-1]) + PAD
    h = (rng.standard_normal((rows, F)) * np.exp(rng.standard_normal((rows, 1)))).astype(F32)
    got, idx = _segment_sum(h, off, want_index=True)
    assert got.dtype == F32 and got.shape == (len(lengths), F)
    h64 = h.astype(np.float64)
    for s, n in enumerate(lengths):
        seg = h64[off[s]:off[s + 1]]
        bound = max(n - 1, 0) * 2.0**-24 * np.abs(seg).sum(axis=0) * (1 + 2.0**-20)
        err = np.abs(got[s].astype(np.float64) - seg.sum(axis=0))
        assert (err <= bound).all(), (s, n, err, bound)
    assert not got[1].any() and np.array_equal(got[0], h[0])
    assert np.array_equal(idx, CO.ids_of(off, rows).astype(np.int32))
    # the whole call again: the same bits
    assert np.array_equal(_segment_sum(h, off), got)
    # the broadcast is the host's gather, exactly; rows in no set get zeros
    gc = rng.standard_normal((len(lengths), F)).astype(F32)
    want = np.where(idx[:, None] >= 0, gc[np.maximum(idx, 0)], F32(0))
    assert np.array_equal(_segment_bcast(gc, idx, F), want)
    assert not _segment_bcast(gc, idx, F)[-PAD:].any()


@pytest.mark.parametrize("F", [3, 8])
def test_segment_sum_order_depends_on_the_set_alone(F):
    """A set summed alone, first, last and between other sets (other S, other
    grid, other row alignment) gives the same bits."""
    rng = np.random.default_rng(20 + F)
    k = _chunk()
    for n in (65, k + 1, 2 * k + 76):
        mine = rng.standard_normal((n, F)).astype(F32)
        others = [rng.standard_normal((m, F)).astype(F32) for m in (7, k + 3, 1, 130)]
        alone = _segment_sum(mine, _offsets([n]))[0]
        layouts = {"first": [mine] + others, "last": others + [mine], "between": others[:2] + [mine] + others[2:]}
        for name, parts in layouts.items():
            at = [p is mine for p in parts].index(True)
            out = _segment_sum(np.concatenate(parts + [np.zeros((PAD, F), F32)]), _offsets([len(p) for p in parts]))
            assert np.array_equal(out[at], alone), (n, name)


def test_segment_sum_three_levels():
    """A set of more than chunk^2 rows: its chunk sums are summed by chunks
    again, and those once more (three levels from 2^18 rows on).  The bound of
    test_segment_sum_against_float64 holds, the small sets beside it have the
    bits they have in a batch of one level, and so has the long set alone."""
    rng = np.random.default_rng(35)
    k, F = _chunk(), 3
    n = k * k + 2 * k + 88
    small = [rng.standard_normal((m, F)).astype(F32) for m in (65, 1, k + 1)]
    big = rng.standard_normal((n, F)).astype(F32)
    parts = small[:2] + [big] + small[2:]
    out = _segment_sum(np.concatenate(parts + [np.zeros((PAD, F), F32)]), _offsets([len(p) for p in parts]))
    b64 = big.astype(np.float64)
    bound = (n - 1) * 2.0**-24 * np.abs(b64).sum(axis=0) * (1 + 2.0**-20)
    assert (np.abs(out[2] - b64.sum(axis=0)) <= bound).all()
    assert np.array_equal(out[2], _segment_sum(big, _offsets([n]))[0])
    for at, p in ((0, small[0]), (1, small[1]), (3, small[2])):
        assert np.array_equal(out[at], _segment_sum(p, _offsets([len(p)]))[0]), at


def test_segment_sum_clamps_bad_device_offsets():
    """Offsets given on the device skip the host validation; out-of-range and
    decreasing entries give finite results equal to those of the clamped
    offsets (the kernel never indexes outside h: a value check)."""
    from zenflow_amd import nn

    rng = np.random.default_rng(31)
    rows, F = 700, 3
    h = rng.standard_normal((rows, F)).astype(F32)
    for bad in ([5, -3, 70, 40, 10**12, 200], [-(2**62), 2**62, 0, 10], [900, 800, 100], [0, 650, 2**40],
                [3, 3, 3, 2, 699, 701]):
        got = _segment_sum(h, np.asarray(bad, np.int64))
        want = _segment_sum(h, nn.clamp_offsets(bad, rows))
        assert np.isfinite(got).all() and np.array_equal(got, want), bad
        o = nn.clamp_offsets(bad, rows)
        ref = np.stack([h[o[s]:o[s + 1]].astype(np.float64).sum(axis=0) for s in range(len(o) - 1)])
        assert np.abs(got - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())
    # an index array with entries outside [0, S) reads no gc row
    gc = rng.standard_normal((4, F)).astype(F32)
    idx = np.array([0, 3, -1, 4, 2**31 - 1, -(2**31), 1], np.int32)
    out = _segment_bcast(gc, idx, F)
    assert np.array_equal(out[[0, 1, 6]], gc[[0, 3, 1]]) and not out[[2, 3, 4, 5]].any()


# ---- networks ---------------------------------------------------------------------------
def _net(F, in_dim, layers=(32, 32), act="swish", batch_norm=True, dropout=0.0, pool="sum", seed=0):
    """(net, float32 variables with non-trivial BatchNorm parameters, statistics and biases)."""
    from zenflow_amd import nn

    rng = np.random.default_rng(1000 + seed)
    net = nn.ConditionNet(F, layers=layers, act=act, batch_norm=batch_norm, dropout=dropout, pool=pool)
    x0 = np.zeros((4, in_dim), F32)
    v = net.init(seed, x0, np.array([0, 4])) if pool == "sum" else net.init(seed, x0)
    for d in v["params"]["NNBlock_0"].values():
        d["bias"] = (0.3 * rng.standard_normal(d["bias"].shape)).astype(F32)
    if batch_norm:
        v["params"]["BatchNorm_0"] = {"scale": (1 + 0.2 * rng.standard_normal(in_dim)).astype(F32),
                                      "bias": (0.2 * rng.standard_normal(in_dim)).astype(F32)}
        v["batch_stats"]["BatchNorm_0"] = {"mean": (0.2 * rng.standard_normal(in_dim)).astype(F32),
                                           "var": (1 + 0.5 * rng.random(in_dim)).astype(F32)}
    return net, v


def _cfg(net):
    from zenflow_amd.activations import act_code, act_name

    return {"layers": list(net.layers), "features": net.features, "act": act_name(act_code(net.act)),
            "batch_norm": net.batch_norm, "dropout": net.dropout, "pool": net.pool}


def _batch(in_dim, seed, extra_sets=()):
    rng = np.random.default_rng(2000 + seed)
    lengths = _lengths() + list(extra_sets)
    off = _offsets(lengths)
    rows = int(off[-1]) + PAD
    x = (rng.standard_normal((rows, in_dim)) * (1 + 0.5 * np.arange(in_dim)) + 0.3).astype(F32)
    x[-PAD:] = 0  # the notebook pads with zeros
    return x, off, rows


def _oracle(net, variables, x, off, mode="net", train=True, **extra):
    """The oracle's result for one job, from its CPU-only child process."""
    rows = len(x)
    S = len(off) - 1
    with tempfile.TemporaryDirectory() as d:
        job, out = Path(d) / "job.npz", Path(d) / "out.npz"
        CO.pack_job(job, _cfg(net), variables, x, CO.ids_of(off, rows), S, mode=mode, train=train, **extra)
        subprocess.run([sys.executable, "-m", "tests.condnet_oracle", str(job), str(out)], cwd=ROOT, check=True,
                       timeout=600)
        return dict(np.load(out))


def _check(ref, name, key, got, bad, rec):
    """The parity rule of the module docstring for one tensor."""
    r64 = ref[f"{name}64{key}"]
    got = np.asarray(got, np.float64)
    assert got.shape == r64.shape, (name, key, got.shape, r64.shape)
    scale = max(np.abs(r64).max(), 1e-30)
    e32 = max(np.abs(ref[f"{name}32_{k}{key}"] - r64).max() for k in range(3))
    cond = max(np.abs(ref[f"{name}64p_{k}{key}"] - r64).max() for k in range(2))
    e = np.abs(got - r64)
    ok = e <= 1e-5 * scale + 2 * max(e32, cond)
    rec[f"{name}{key}"] = (float(e.max() / scale), float(e32 / scale), float(cond / scale))
    print(f"{name}{key}: gpu {e.max() / scale:.3g}  fp32 oracle {e32 / scale:.3g}  conditioning {cond / scale:.3g}")
    if not ok.all():
        bad.append(f"{name}{key}: {np.sum(~ok)} of {ok.size} over, max rel {e.max() / scale:.3g} "
                   f"(fp32 oracle {e32 / scale:.3g}, conditioning {cond / scale:.3g})")


def _record(rec):
    from tests.test_gpu_flow import _append_record

    _append_record("condnet_parity.jsonl", rec)


def _leaves(tree):
    return dict(CO._flat(tree))


FORWARD_CASES = [(3, 2, a) for a in ACTS] + [(3, 5, "swish"), (8, 2, "swish"), (8, 5, "swish")]


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("F,in_dim,act", FORWARD_CASES)
def test_forward_parity(F, in_dim, act, train):
    """c, and in train mode the updated batch_stats, against the oracle: all
    eight activations at one shape and swish at all shapes, pooled, with
    dropout in train mode (the mask restated on the host)."""
    from zenflow_amd import nn

    net, v = _net(F, in_dim, act=act, dropout=0.3, seed=F + in_dim)
    x, off, rows = _batch(in_dim, F)
    seed = 77
    keep = nn.dropout_keep(seed, rows, F, net.dropout) if train else None
    ref = _oracle(net, v, x, off, train=train, keep=keep)
    ct_ = nn.ConditionTrainer(net, v, in_dim, rows)
    c = ct_.forward(x, off, train=train, seed=seed)
    assert c.dtype == F32 and c.shape == (len(off) - 1, F)
    bad, rec = [], {"what": "forward", "F": F, "in_dim": in_dim, "act": act, "train": train}
    _check(ref, "c", "", c, bad, rec)
    stats = ct_.variables()["batch_stats"]["BatchNorm_0"]
    if train:
        for k in ("mean", "var"):
            _check(ref, "stats", f":BatchNorm_0/{k}", stats[k], bad, rec)
    else:  # eval mode moves nothing
        assert np.array_equal(stats["mean"], v["batch_stats"]["BatchNorm_0"]["mean"])
        assert np.array_equal(stats["var"], v["batch_stats"]["BatchNorm_0"]["var"])
        # and the module's own eval apply is the same pass
        assert np.array_equal(net.apply(v, x, off), c)
    _record(rec)
    assert not bad, bad


GRAD_CASES = [(3, 5, 0.3, True, "sum"), (8, 2, 0.0, True, "sum"), (3, 2, 0.3, False, "sum"), (8, 5, 0.0, False, "sum"),
              (8, 2, 0.3, True, None), (3, 5, 0.0, True, None), (8, 5, 0.3, False, None), (3, 2, 0.0, False, None)]


@pytest.mark.parametrize("F,in_dim,dropout,batch_norm,pool", GRAD_CASES)
def test_parameter_gradients(F, in_dim, dropout, batch_norm, pool):
    """ConditionTrainer.backward(gc) for a random cotangent against float64
    autograd, every element of every tensor: dropout on and off, BatchNorm on
    and off, pooled and per-row."""
    from zenflow_amd import nn

    net, v = _net(F, in_dim, dropout=dropout, batch_norm=batch_norm, pool=pool, seed=10 * F + in_dim)
    x, off, rows = _batch(in_dim, 3 * F + in_dim)
    seed = 2**40 + 5
    n_out = len(off) - 1 if pool == "sum" else rows
    gc = np.random.default_rng(5).standard_normal((n_out, F)).astype(F32)
    keep = nn.dropout_keep(seed, rows, F, dropout) if dropout else None
    ref = _oracle(net, v, x, off, keep=keep, gc=gc)
    ct_ = nn.ConditionTrainer(net, v, in_dim, rows)
    c = ct_.forward(x, off if pool == "sum" else None, seed=seed)
    g = ct_.backward(gc)
    assert g.dtype == F32 and g.shape == (ct_.layout.size,)
    assert not g[ct_.layout.param_mask == 0].any()  # statistics and padding
    bad, rec = [], {"what": "gradient", "F": F, "in_dim": in_dim, "dropout": dropout, "batch_norm": batch_norm,
                    "pool": pool}
    _check(ref, "c", "", c, bad, rec)
    tree = _leaves(ct_.grad_tree(g))
    assert set("g64:" + k for k in tree) == set(k for k in ref if k.startswith("g64:"))
    for k, a in tree.items():
        _check(ref, "g", ":" + k, a, bad, rec)
    _record(rec)
    assert not bad, bad
    # the same pass again: the same bits
    ct_.forward(x, off if pool == "sum" else None, seed=seed)
    assert np.array_equal(ct_.backward(gc), g)


# ---- dropout --------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0.3, 0.5])
def test_dropout_is_the_host_rule(rate):
    """A network that is the identity up to dropout (no BatchNorm, one Dense
    with the unit matrix): the train-mode output is the host restatement of
    the mask rule exactly; same seed, same bits; another seed, another mask;
    eval mode ignores the seed.  The standalone entries apply the same rule."""
    from zenflow_amd import nn

    F, rows = 8, 1500
    rng = np.random.default_rng(41)
    x = rng.standard_normal((rows, F)).astype(F32)
    net = nn.ConditionNet(F, layers=(), batch_norm=False, dropout=rate, pool=None)
    v = {"params": {"NNBlock_0": {"Dense_0": {"kernel": np.eye(F, dtype=F32), "bias": np.zeros(F, F32)}}}}
    ct_ = nn.ConditionTrainer(net, v, F, rows)
    kp = F32(1) - F32(rate)

    def host(seed):
        return np.where(nn.dropout_keep(seed, rows, F, rate), x / kp, F32(0)).astype(F32)

    a = ct_.forward(x, seed=11)
    assert np.array_equal(a, host(11))
    assert np.array_equal(ct_.forward(x, seed=11), a)
    b = ct_.forward(x, seed=12)
    assert np.array_equal(b, host(12)) and 0.2 < ((a == 0) != (b == 0)).mean() < 0.8
    big = 2**63 + 12345  # all 64 bits of the seed are key bits
    assert np.array_equal(ct_.forward(x, seed=big), host(big))
    assert np.array_equal(ct_.forward(x, train=False, seed=11), x)
    assert np.array_equal(ct_.forward(x, train=False, seed=12), x)
    # its reverse recomputes the mask: g = gc * keep / (1 - rate) feeds the Dense layer's gradient
    gc = rng.standard_normal((rows, F)).astype(F32)
    ct_.forward(x, seed=11)
    g = ct_.grad_tree(ct_.backward(gc))["NNBlock_0"]["Dense_0"]
    gl = np.where(nn.dropout_keep(11, rows, F, rate), gc / kp, F32(0)).astype(np.float64)
    assert np.abs(g["bias"] - gl.sum(axis=0)).max() <= 1e-5 * np.abs(gl).sum(axis=0).max()
    assert np.abs(g["kernel"] - x.astype(np.float64).T @ gl).max() <= 1e-5 * (np.abs(x).T @ np.abs(gl)).max()
    # standalone: every row its own set
    off = np.arange(rows + 1, dtype=np.int64)
    out, idx = _segment_sum(x, off, rate=rate, seed=11, want_index=True)
    assert np.array_equal(out, host(11))
    assert np.array_equal(_segment_bcast(gc, idx, F, rate=rate, seed=11), gl.astype(F32))


# ---- the joint gradient through a conditional flow ----------------------------------------------
def _flow_case(C, N, seed):
    """A 2-D conditional flow, rolling_spline_coupling(2, knots=8, layers=(32, 32)), as a tests/flowcases case."""
    from oracle import zf_oracle as O
    from tests.flowcases import make_variables

    cfg = dict(D=2, C=C, K=8, layers=(32, 32), latent="beta")
    rng = np.random.default_rng(seed)
    spec, variables = make_variables(cfg, rng)
    xs = rng.standard_normal((512, 2)).astype(F32)
    _, _, sb = O.shift_bounds_forward(spec["bijectors"][0], {}, xs, train=True)
    variables["batch_stats"]["bijector"]["bijectors_0"] = {k: np.asarray(v, F32) for k, v in sb.items()}
    y = rng.standard_normal((N, 2)).astype(F32)
    return {"cfg": cfg, "model": {"bijector": spec, "latent": {"type": "beta"}}, "variables": variables, "x": y}


@pytest.mark.parametrize("F", [3, 8])
def test_joint_gradient(F):
    """loss_fn_2: the flow's train-mode loss on c = phi(x).  tr.loss_grad(Y, c,
    cond_grad=True) then ct.backward(gc) against float64 autograd of the
    composed loss with respect to the network's parameters; the flow's own
    loss and gradient have the bits they have with c as a plain array."""
    from tests.flowcases import _trainer
    from zenflow_amd import _lib as L
    from zenflow_amd import nn

    in_dim = 2
    net, v = _net(F, in_dim, dropout=0.3, seed=50 + F)
    x, off, rows = _batch(in_dim, 60 + F, extra_sets=[5, 9, 2, 31] * 6)
    S = len(off) - 1
    case = _flow_case(F, S, 70 + F)
    seed = 9
    keep = nn.dropout_keep(seed, rows, F, net.dropout)
    ref = _oracle(net, v, x, off, mode="joint", keep=keep, model=case["model"], flow_variables=case["variables"],
                  y=case["x"])
    ct_ = nn.ConditionTrainer(net, v, in_dim, rows, sets_max=S)
    tr = _trainer(case, S)
    c = ct_.forward(L.DeviceArray.from_numpy(x), L.DeviceArray.from_numpy(off), seed=seed)
    assert isinstance(c, L.DeviceArray) and c.shape == (S, F)
    yd = L.DeviceArray.from_numpy(case["x"])
    loss, gflow, gc = tr.loss_grad(yd, c, cond_grad=True)
    assert isinstance(gc, L.DeviceArray)
    g = ct_.backward(gc)
    assert isinstance(g, L.DeviceArray)
    loss_plain, gflow_plain = _trainer(case, S).loss_grad(case["x"], c.numpy())
    assert loss == loss_plain and np.array_equal(gflow, gflow_plain)
    assert loss == pytest.approx(float(ref["loss64"]), rel=2e-5, abs=2e-5)
    bad, rec = [], {"what": "joint gradient", "F": F}
    for k, a in _leaves(ct_.grad_tree(g.numpy())).items():
        _check(ref, "g", ":" + k, a, bad, rec)
    _record(rec)
    assert not bad, bad


def test_joint_loop_lowers_the_loss():
    """The loop of the documentation as written, c and gc never leaving the
    device, with sets whose length the condition has to carry."""
    from tests.flowcases import _trainer
    from zenflow_amd import _lib as L
    from zenflow_amd import nn

    rng = np.random.default_rng(81)
    S, F = 200, 4
    n = rng.integers(1, 40, S)
    off = _offsets(n)
    rows = int(off[-1]) + PAD
    X = np.concatenate([rng.standard_normal((int(off[-1]), 2)), np.zeros((PAD, 2))]).astype(F32)
    Y = (np.sqrt(n)[:, None] * 0.3 + 0.2 * rng.standard_normal((S, 2))).astype(F32)
    net = nn.ConditionNet(F, layers=(32, 32), dropout=0.1, pool="sum")
    v = net.init(3, X, off)
    ct_ = nn.ConditionTrainer(net, v, 2, rows, sets_max=S)
    case = _flow_case(F, S, 82)
    tr = _trainer(case, S)
    Xd, off_d, Yd = L.DeviceArray.from_numpy(X), L.DeviceArray.from_numpy(off), L.DeviceArray.from_numpy(Y)
    losses = []
    for epoch in range(40):
        c = ct_.forward(Xd, off_d, seed=epoch)
        gc = tr.step(Yd, c, cond_grad=True)
        ct_.step(gc)
        losses.append(tr.last_loss())
    assert np.isfinite(losses).all() and np.mean(losses[-5:]) < np.mean(losses[:5]), losses
    moved = _leaves(ct_.variables()["params"])
    assert any(not np.array_equal(moved[k], a) for k, a in _leaves(v["params"]).items())


# ---- the optimiser --------------------------------------------------------------------------------
def test_optimiser_trajectory():
    """Twenty ConditionTrainer.step calls on a fixed sequence of gc, optim.adamw
    behind clip_by_global_norm, against tests/optim_ref.py::chain_reference in
    float64 driven by the float64 gradients.  The allowance is measured, not
    fixed: the float32 CPU restatement (chain_kernel_f32 on float32 autograd)
    free-running on the same sequence ends d32 = max|theta32 - theta64| away;
    the GPU may end twice that away (another, equally valid fp32 order) plus
    1e-6 max|theta|."""
    from zenflow_amd import nn, optim

    F, in_dim, T = 3, 2, 20
    net, v = _net(F, in_dim, dropout=0.3, seed=90)
    x, off, rows = _batch(in_dim, 91)
    S = len(off) - 1
    gcs = np.random.default_rng(92).standard_normal((T, S, F)).astype(F32)
    keeps = np.stack([nn.dropout_keep(t, rows, F, net.dropout) for t in range(T)])
    opt = {"max_norm": 1.0, "learning_rate": 1e-3, "weight_decay": 1e-4}
    ref = _oracle(net, v, x, off, mode="traj", gcs=gcs, keeps=keeps, opt=opt)
    chain = optim.chain(optim.clip_by_global_norm(opt["max_norm"]),
                        optim.adamw(opt["learning_rate"], weight_decay=opt["weight_decay"]))
    ct_ = nn.ConditionTrainer(net, v, in_dim, rows, optimizer=chain)
    for t in range(T):
        ct_.forward(x, off, seed=t)
        ct_.step(gcs[t])
    got = _leaves(ct_.variables()["params"])
    start = _leaves(v["params"])
    d32 = max(np.abs(ref["theta32:" + k] - ref["theta64:" + k]).max() for k in got)
    dgpu = max(np.abs(got[k].astype(np.float64) - ref["theta64:" + k]).max() for k in got)
    tmax = max(np.abs(ref["theta64:" + k]).max() for k in got)
    moved = max(np.abs(ref["theta64:" + k] - start[k]).max() for k in got)
    from tests.test_gpu_flow import _append_record

    _append_record("condnet_trajectory.jsonl", {
        "steps": T, "rows": rows, "sets": S, "chain": "clip_by_global_norm(1.0), adamw(1e-3, weight_decay=1e-4)",
        "fp32_restatement_max_abs_dist_from_fp64": float(d32), "gpu_max_abs_dist_from_fp64": float(dgpu),
        "max_abs_theta": float(tmax), "max_abs_change_over_trajectory": float(moved)})
    print(f"trajectory: fp32 restatement {d32:.3g}, gpu {dgpu:.3g}, max|theta| {tmax:.3g}, moved {moved:.3g}")
    assert moved > 5e-3  # twenty steps of 1e-3
    assert dgpu <= 2 * d32 + 1e-6 * tmax, (dgpu, d32, tmax)


def test_optimizer_forms():
    """The default (n)adamw and a masked weight decay; apply_gradient takes a tree."""
    from zenflow_amd import nn, optim
    from zenflow_amd.train import adamw

    net, v = _net(3, 2, seed=95)
    x, off, rows = _batch(2, 96)
    gc = np.random.default_rng(97).standard_normal((len(off) - 1, 3)).astype(F32)

    def mask(p):  # weight decay on the Dense kernels alone
        return {"BatchNorm_0": {"scale": False, "bias": False},
                "NNBlock_0": {k: {"kernel": True, "bias": False} for k in p["NNBlock_0"]}}

    ends = []
    for opt in (None, adamw(1e-2), optim.adamw(1e-2, weight_decay=0.5, mask=mask), optim.sgd(1e-2)):
        ct_ = nn.ConditionTrainer(net, v, 2, rows, optimizer=opt)
        ct_.forward(x, off)
        g = ct_.backward(gc)
        ct_.apply_gradient(ct_.grad_tree(g))
        ends.append(_leaves(ct_.variables()["params"]))
    start = _leaves(v["params"])
    for e in ends:
        assert all(np.isfinite(a).all() for a in e.values())
        assert not np.array_equal(e["NNBlock_0/Dense_1/kernel"], start["NNBlock_0/Dense_1/kernel"])
    k = "NNBlock_0/Dense_1/kernel"
    # a decay of 0.5 on the kernels alone: they differ from plain adamw(1e-2), the biases do not
    assert not np.array_equal(ends[2][k], ends[1][k])
    # (the biases differ by the unmasked chain's own decay, 1e-2 * 1e-4 * |bias|)
    assert np.abs(ends[2]["NNBlock_0/Dense_1/bias"] - ends[1]["NNBlock_0/Dense_1/bias"]).max() <= 5e-6
    g64 = g.astype(np.float64)
    sgd = start[k] - 1e-2 * _leaves(ct_.grad_tree(g64))[k]
    assert np.abs(ends[3][k] - sgd).max() <= 1e-6 * max(1.0, np.abs(sgd).max())


# ---- the module protocol -----------------------------------------------------------------------
def test_module_protocol():
    """DeepSetFlow as the notebook writes it, with phi a ConditionNet: init,
    train-mode apply with mutable batch_stats, eval apply equal to the two
    parts called separately, sample; a params tree in the notebook's layout
    loads."""
    import zenflow_amd as zf
    from tests.test_condnet_host import NOTEBOOK_PHI, _shapes
    from zenflow_amd import nn
    from zenflow_amd.bijectors import rolling_spline_coupling

    class DeepSetFlow(zf.Module):
        def __init__(self, bijectors):
            self.bijectors = bijectors

        def setup(self):
            self.phi = nn.ConditionNet(8, layers=(128,) * 3, dropout=0.3, pool="sum")
            self.flow = zf.Flow(self.bijectors)

        def __call__(self, x, offsets, y, train: bool = False, seed: int = 0):
            c = self.phi(x, offsets, train=train, seed=seed)
            return self.flow(y, c, train=train)

        def sample(self, x, offsets, sizes, seed):
            c = self.phi(x, offsets)
            return self.flow.sample(np.repeat(c, sizes, axis=0), seed=seed)

    rng = np.random.default_rng(7)
    n = [1, 0, 63, 64, 65, 9, 30, 4]
    off = _offsets(n)
    rows = int(off[-1]) + PAD
    X = np.concatenate([rng.standard_normal((int(off[-1]), 2)), np.zeros((PAD, 2))]).astype(F32)
    Y = rng.standard_normal((len(n), 2)).astype(F32)
    m = DeepSetFlow(rolling_spline_coupling(2, knots=8, layers=(32, 32)))
    v = m.init(zf.PRNGKey(0), X, off, Y)
    assert _shapes(v["params"]["phi"]) == NOTEBOOK_PHI
    with pytest.raises(RuntimeError, match="mutable"):
        m.apply(v, X, off, Y, train=True)
    lp_t, upd = m.apply(v, X, off, Y, train=True, seed=3, mutable=["batch_stats"])
    assert lp_t.shape == (len(n),) and np.isfinite(lp_t).all()
    new = upd["batch_stats"]
    assert set(new) == {"phi", "flow"}
    mean = new["phi"]["BatchNorm_0"]["mean"]
    assert np.abs(mean - 0.01 * X.mean(axis=0)).max() <= 1e-6  # 0.99 * 0 + 0.01 * the batch mean, padding rows included
    v2 = {"params": v["params"], "batch_stats": new}
    lp = m.apply(v2, X, off, Y)
    c = m.phi.apply({"params": v2["params"]["phi"], "batch_stats": new["phi"]}, X, off)
    lp_parts = m.flow.apply({"params": v2["params"]["flow"], "batch_stats": new["flow"]}, Y, c)
    assert c.shape == (len(n), 8) and np.array_equal(lp, lp_parts, equal_nan=True) and np.isfinite(lp).any()
    xs = m.apply(v2, X, off, 3, 5, method="sample")
    assert xs.shape == (3 * len(n), 2) and np.isfinite(xs).all()
    # a tree in the notebook's layout (float64 leaves, as np.load gives them) loads
    tree = {"params": {k: ({kk: {n_: rng.standard_normal(s) * 0.1 for n_, s in d.items()} for kk, d in t.items()}
                           if k == "NNBlock_0" else {n_: np.ones(s) for n_, s in t.items()})
                       for k, t in NOTEBOOK_PHI.items()},
            "batch_stats": {"BatchNorm_0": {"mean": np.zeros(2), "var": np.ones(2)}}}
    out = nn.ConditionNet(8, layers=(128,) * 3, dropout=0.3, pool="sum").apply(tree, X, off)
    assert out.shape == (len(n), 8) and np.isfinite(out).all() and not out[1].any()  # the empty set: a zero row
    # device in, device out
    from zenflow_amd import _lib as L

    outd = m.phi.apply({"params": v2["params"]["phi"], "batch_stats": new["phi"]}, L.DeviceArray.from_numpy(X),
                       L.DeviceArray.from_numpy(off))
    assert isinstance(outd, L.DeviceArray) and np.array_equal(outd.numpy(), c)


# ---- rejections -----------------------------------------------------------------------------------
def test_rejections():
    """Each raises the documented error before any launch."""
    from tests.flowcases import _trainer
    from zenflow_amd import _lib as L
    from zenflow_amd import nn

    # features + D - D // 2 > 64 conditioner inputs at the flow's trainer
    with pytest.raises(NotImplementedError, match="64 conditioner inputs"):
        _trainer(_flow_case(64, 8, 1), 8)
    with pytest.raises(NotImplementedError):
        nn.ConditionNet(8, layers=(4,)).init(0, np.zeros((3, 65), F32))
    with pytest.raises(NotImplementedError):
        nn.ConditionNet(8, layers=(4097,))
    with pytest.raises(NotImplementedError):
        nn.ConditionNet(8, layers=(8,) * 17)
    net, v = _net(3, 2, seed=99)
    x, off, rows = _batch(2, 98)
    ct_ = nn.ConditionTrainer(net, v, 2, rows, sets_max=len(off) - 1)
    with pytest.raises(ValueError, match="pending"):
        ct_.backward(np.zeros((len(off) - 1, 3), F32))
    with pytest.raises(ValueError, match="rows_max"):
        ct_.forward(np.zeros((rows + 1, 2), F32), off)
    with pytest.raises(ValueError, match="sets_max"):
        ct_.forward(x, np.concatenate([off, [off[-1]]]))
    with pytest.raises(ValueError):
        ct_.forward(x, off, train=False, update_stats=True)
    ct_.forward(x, off, train=False)  # eval mode leaves nothing pending
    with pytest.raises(ValueError, match="pending"):
        ct_.backward(np.zeros((len(off) - 1, 3), F32))
    ct_.forward(x, off)
    with pytest.raises(ValueError):  # the wrong shape of gc keeps the pass pending
        ct_.backward(np.zeros((len(off), 3), F32))
    g = ct_.backward(np.zeros((len(off) - 1, 3), F32))
    assert not g.any()
    with pytest.raises(ValueError, match="pending"):  # one backward per forward
        ct_.backward(np.zeros((len(off) - 1, 3), F32))
    # the C entries themselves (the Python checks aside)
    lib = L.load_library()
    xd, od = L.DeviceArray.from_numpy(x), L.DeviceArray.from_numpy(off)
    out = L.DeviceArray((len(off) - 1, 3))
    S = len(off) - 1
    assert lib.zf_condnet_backward(ct_.handle, out.ptr, None, L.stream()) == -1
    assert b"no forward pending" in lib.zf_last_error()
    assert lib.zf_condnet_forward(ct_.handle, xd.ptr, rows + 1, od.ptr, S, 1, 1, 0, out.ptr, L.stream()) == -1
    assert lib.zf_condnet_forward(ct_.handle, xd.ptr, rows, od.ptr, S + 1, 1, 1, 0, out.ptr, L.stream()) == -1
    assert lib.zf_condnet_forward(ct_.handle, xd.ptr, rows, None, S, 1, 1, 0, out.ptr, L.stream()) == -1
    assert lib.zf_condnet_forward(ct_.handle, xd.ptr, rows, od.ptr, S, 0, 1, 0, out.ptr, L.stream()) == -1
    assert lib.zf_condnet_forward(ct_.handle, xd.ptr, rows, od.ptr, S, 0, 0, 0, out.ptr, L.stream()) == 0
    assert lib.zf_condnet_backward(ct_.handle, out.ptr, None, L.stream()) == -1  # after an eval-mode forward
    from zenflow_amd import optim

    with pytest.raises(NotImplementedError, match="clip_by_global_norm"):
        nn.ConditionTrainer(net, v, 2, rows, optimizer=optim.chain(optim.scale(1.0), optim.clip_by_global_norm(1.0)))
