"""Mean and max over ragged sets on the GPU (zf_segment_pool,
zf_segment_pool_bcast, ``ConditionNet(pool="max")``): the standalone entries
against exact host restatements, and networks with the max pooling against the
float64 / float32 oracle of tests/pool_oracle.py.

The batches are tests/test_gpu_condnet.py's: set lengths 1, 0, 63, 64, 65,
chunk - 1, chunk, chunk + 1, 2 chunk + 76, and 37 trailing rows in no set;
F = 3 (no divisor of 64) and F = 8.

Standalone.  The maximum, the counts and both reverses are exact, so they are
compared under ``==``; the mean is the device's own zf_segment_sum divided on
the host by float32(n_s), bit for bit.  The dropped values are formed on the
host from ``nn.dropout_keep`` and one float32 division.

Networks.  The parity rule is the project's own, per tensor (quoted in
tests/test_gpu_condnet.py):
    |v_gpu - v64| <= 1e-5 max|v64| + 2 max(|v32 - v64|, |v64' - v64|)
with v32 the float32 oracle over three row orders and v64' float64 at inputs
and parameters jittered by 2^-22 relative.  For the max, each case first
asserts, in the float64 oracle, that over every (set, column) the largest and
the second-largest distinct value of d are at least 1e-4 max|d| apart (exact
zero ties from dropout are ties in every precision), so that no fp32
evaluation picks another row; the seeds below were chosen on the CPU so that
the oracle alone meets it."""

import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

from tests import condnet_oracle as CO
from tests.test_gpu_condnet import (PAD, _batch, _cfg, _check, _chunk, _flow_case, _leaves, _lengths, _net, _offsets,
                                    _segment_bcast, _segment_sum)

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
F32 = np.float32
BAD_OFFSETS = ([5, -3, 70, 40, 10**12, 200], [-(2**62), 2**62, 0, 10], [900, 800, 100], [0, 650, 2**40],
               [3, 3, 3, 2, 699, 701])


def _code(pool):
    from zenflow_amd import _lib as L

    return {"sum": L.ZF_POOL_SUM, "mean": L.ZF_POOL_MEAN, "max": L.ZF_POOL_MAX}[pool]


# ---- the standalone entries ----------------------------------------------------------
def _pool(h, off, pool, rate=0.0, seed=0):
    """zf_segment_pool on device copies of h (rows, F) and off (any int64s):
    (out, set index, count); the count buffer starts as -7 everywhere."""
    from zenflow_amd import _lib as L

    lib = L.load_library()
    rows, F = h.shape
    S = len(off) - 1
    hd = L.DeviceArray.from_numpy(np.ascontiguousarray(h, F32))
    od = L.DeviceArray.from_numpy(np.ascontiguousarray(off, np.int64))
    out, idx = L.DeviceArray((S, F)), L.DeviceArray((rows,), np.int32)
    cnt = L.DeviceArray.from_numpy(np.full((S, F), -7, np.int32))
    ws = L.DeviceArray((max(1, lib.zf_segment_pool_workspace_bytes(rows, S, F, _code(pool))),), np.uint8)
    L.check(lib.zf_segment_pool(hd.ptr, rows, F, od.ptr, S, _code(pool), rate, seed, out.ptr, idx.ptr, cnt.ptr, ws.ptr,
                                L.stream()), "zf_segment_pool")
    return out.numpy(), idx.numpy(), cnt.numpy()


def _pool_bcast(gc, idx, pool, h, out, count, rate=0.0, seed=0):
    from zenflow_amd import _lib as L

    rows, F = h.shape
    dev = [L.DeviceArray.from_numpy(np.ascontiguousarray(a, t))
           for a, t in ((gc, F32), (idx, np.int32), (h, F32), (out, F32), (count, np.int32))]
    g = L.DeviceArray((rows, F))
    L.check(L.load_library().zf_segment_pool_bcast(dev[0].ptr, dev[1].ptr, rows, F, len(gc), _code(pool), rate, seed,
                                                   dev[2].ptr, dev[3].ptr, dev[4].ptr, g.ptr, L.stream()),
            "zf_segment_pool_bcast")
    return g.numpy()


def _dropped(h, rate, seed):
    """(d, keep, keep_prob): d = keep ? h / (float32(1) - rate) : 0 in float32."""
    from zenflow_amd import nn

    if not rate:
        return h, np.ones(h.shape, bool), F32(1)
    kp = F32(1) - F32(rate)
    keep = nn.dropout_keep(seed, h.shape[0], h.shape[1], rate)
    with np.errstate(invalid="ignore"):
        return np.where(keep, h / kp, F32(0)).astype(F32), keep, kp


def _host_max(d, o):
    with np.errstate(invalid="ignore"):
        return np.stack([d[o[s]:o[s + 1]].max(axis=0) if o[s + 1] > o[s] else np.zeros(d.shape[1], F32)
                         for s in range(len(o) - 1)])


def _host_ties(d, c, ids):
    """tie[i, f]: row i is in a set and d[i, f] is its (set, column)'s maximum (NaN entries for a NaN maximum)."""
    cs = c[np.maximum(ids, 0)]
    return (ids[:, None] >= 0) & ((d == cs) | (np.isnan(cs) & np.isnan(d)))


def _host_reverse(gc, ids, count, on, keep, kp):
    """g_h = (on ? gc[set] / float32(count[set]) : 0) * keep / keep_prob, each step one float32 operation."""
    s = np.maximum(ids, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        gd = np.where(on & (ids[:, None] >= 0) & (count[s] > 0), gc[s] / count[s].astype(F32), F32(0)).astype(F32)
        return np.where(keep, gd / kp, F32(0)).astype(F32) if kp != 1 else gd


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _data(F, seed):
    rng = np.random.default_rng(seed)
    lengths = _lengths()
    off = _offsets(lengths)
    rows = int(off[-1]) + PAD
    h = (rng.standard_normal((rows, F)) * np.exp(rng.standard_normal((rows, 1)))).astype(F32)
    return rng, lengths, off, rows, h


@pytest.mark.parametrize("rate", [0.0, 0.25])
@pytest.mark.parametrize("F", [3, 8])
def test_max_forward(F, rate):
    """np.max of every set's dropped values under ==; a zero row for the empty
    set; a planted NaN makes exactly its (set, column) NaN; planted +-inf are
    values; the whole call twice gives the same bits."""
    rng, lengths, off, rows, h = _data(F, 300 + F)
    seed = 2**40 + 11
    _, keep, _ = _dropped(h, rate, seed)
    k = _chunk()
    long_set = len(lengths) - 1
    # a NaN in the long set's second chunk, column 1, on an entry the mask keeps
    r_nan = int(off[long_set]) + k + int(np.flatnonzero(keep[off[long_set] + k:off[long_set] + 2 * k, 1])[0])
    h[r_nan, 1] = np.nan
    r_inf = int(off[5]) + int(np.flatnonzero(keep[off[5]:off[6], 0])[-1])  # +inf: the maximum of (set 5, column 0)
    h[r_inf, 0] = np.inf
    h[off[6]:off[7], 2] = -np.inf  # a column of -inf alone: the maximum is -inf (or a dropped 0)
    h[off[4] + 7, 2] = -np.inf  # -inf among finite values changes nothing
    h[-1, 0] = np.nan  # a row in no set takes no part
    d, keep, _ = _dropped(h, rate, seed)
    want = _host_max(d, off)
    got, idx, _ = _pool(h, off, "max", rate, seed)
    assert got.dtype == F32 and np.array_equal(got, want, equal_nan=True)
    nan_at = np.zeros_like(want, bool)
    nan_at[long_set, 1] = True
    assert np.array_equal(np.isnan(got), nan_at)
    assert got[5, 0] == np.inf and not got[1].any()
    assert got[6, 2] == (-np.inf if keep[off[6]:off[7], 2].all() else 0)
    assert np.array_equal(idx, CO.ids_of(off, rows).astype(np.int32))
    again, idx2, _ = _pool(h, off, "max", rate, seed)
    assert _same_bits(again, got) and np.array_equal(idx2, idx)
    if not rate:  # the public function is the same call
        from zenflow_amd import nn

        assert _same_bits(nn.segment_max(h, off), got)


@pytest.mark.parametrize("rate", [0.0, 0.25])
@pytest.mark.parametrize("F", [3, 8])
def test_max_counts_and_reverse(F, rate):
    """Planted exact ties (the long set's maximal row of column 0 copied to
    three more of its rows, in other chunks; a column of negative values, whose
    dropped entries all tie at 0 under dropout; a NaN maximum): the int32 tie
    counts are the host's, the reverse is the host restatement bit for bit,
    rows in no set get zeros."""
    rng, lengths, off, rows, h = _data(F, 320 + F)
    seed = 977
    k = _chunk()
    a = int(off[-2])  # first row of the long set
    top = a + int(np.argmax(h[a:a + lengths[-1], 0]))
    for r in (a + 5, a + k + 1, a + 2 * k + 70):
        h[r] = h[top]
    h[:, F - 1] = -np.abs(h[:, F - 1]) - F32(1e-3)
    h[off[4] + 3, 1] = h[off[4] + 40, 1] = np.nan  # set 4, column 1: two NaNs
    d, keep, kp = _dropped(h, rate, seed)
    ids = CO.ids_of(off, rows)
    got, idx, cnt = _pool(h, off, "max", rate, seed)
    assert np.array_equal(got, _host_max(d, off), equal_nan=True)
    ties = _host_ties(d, got, ids)
    want_cnt = np.stack([ties[off[s]:off[s + 1]].sum(axis=0) for s in range(len(lengths))]).astype(np.int32)
    assert cnt.dtype == np.int32 and np.array_equal(cnt, want_cnt)
    assert not cnt[1].any() and (np.delete(cnt, 1, axis=0) >= 1).all()
    if rate:
        assert (cnt[-1, F - 1] == (~keep[a:a + lengths[-1], F - 1]).sum()) and cnt[-1, F - 1] > 100
        if keep[[top, a + 5, a + k + 1, a + 2 * k + 70], 0].all():
            assert cnt[-1, 0] == 4
    else:
        assert cnt[-1, 0] == 4 and cnt[4, 1] == 2 and np.isnan(got[4, 1])
    gc = rng.standard_normal((len(lengths), F)).astype(F32)
    g = _pool_bcast(gc, idx, "max", h, got, cnt, rate, seed)
    want = _host_reverse(gc, ids, cnt, ties, keep, kp)
    assert _same_bits(g, want)
    assert not g[-PAD:].any() and g.any()
    assert _same_bits(_pool_bcast(gc, idx, "max", h, got, cnt, rate, seed), g)


@pytest.mark.parametrize("rate", [0.0, 0.25])
@pytest.mark.parametrize("F", [3, 8])
def test_mean(F, rate):
    """out = float32(zf_segment_sum(...) / float32(n_s)) bit for bit, a zero
    row for the empty set, count = n_s in every column; the reverse is
    gc[set] / float32(n_set), then dropout's reverse, bit for bit."""
    rng, lengths, off, rows, h = _data(F, 340 + F)
    seed = 2**63 + 5
    n = np.asarray(lengths)
    sums = _segment_sum(h, off, rate=rate, seed=seed)
    want = np.where(n[:, None] > 0, sums / np.maximum(n, 1).astype(F32)[:, None], F32(0)).astype(F32)
    got, idx, cnt = _pool(h, off, "mean", rate, seed)
    assert _same_bits(got, want) and not got[1].any()
    assert np.array_equal(cnt, np.repeat(n[:, None], F, axis=1).astype(np.int32))
    ids = CO.ids_of(off, rows)
    assert np.array_equal(idx, ids.astype(np.int32))
    _, keep, kp = _dropped(h, rate, seed)
    gc = rng.standard_normal((len(lengths), F)).astype(F32)
    g = _pool_bcast(gc, idx, "mean", h, got, cnt, rate, seed)
    assert _same_bits(g, _host_reverse(gc, ids, cnt, np.ones(h.shape, bool), keep, kp))
    assert not g[-PAD:].any()
    again, _, cnt2 = _pool(h, off, "mean", rate, seed)
    assert _same_bits(again, got) and np.array_equal(cnt2, cnt)
    if not rate:
        from zenflow_amd import nn

        assert _same_bits(nn.segment_mean(h, off), got)


@pytest.mark.parametrize("rate", [0.0, 0.25])
@pytest.mark.parametrize("F", [3, 8])
def test_sum_mode_is_segment_sum(F, rate):
    """ZF_POOL_SUM through the new entries: the bits of zf_segment_sum and
    zf_segment_bcast, the count buffer untouched."""
    rng, lengths, off, rows, h = _data(F, 360 + F)
    seed = 31
    want, widx = _segment_sum(h, off, rate=rate, seed=seed, want_index=True)
    got, idx, cnt = _pool(h, off, "sum", rate, seed)
    assert _same_bits(got, want) and np.array_equal(idx, widx) and (cnt == -7).all()
    gc = rng.standard_normal((len(lengths), F)).astype(F32)
    assert _same_bits(_pool_bcast(gc, idx, "sum", h, got, cnt, rate, seed), _segment_bcast(gc, idx, F, rate, seed))


@pytest.mark.parametrize("pool", ["max", "mean"])
def test_three_levels(pool):
    """A set of more than chunk^2 rows beside small ones: it has the bits it
    has reduced alone, and so have the small sets; the max is np.max, the tie
    count of the long set is the host's."""
    rng = np.random.default_rng(375)
    k, F = _chunk(), 3
    n = k * k + 2 * k + 88
    small = [rng.standard_normal((m, F)).astype(F32) for m in (65, 1, k + 1)]
    big = rng.standard_normal((n, F)).astype(F32)
    big[k * k + k + 7] = big[3] = big[np.argmax(big[:, 0])]  # ties across the levels
    parts = small[:2] + [big] + small[2:]
    out, _, cnt = _pool(np.concatenate(parts + [np.zeros((PAD, F), F32)]), _offsets([len(p) for p in parts]), pool)
    for at, p in enumerate(parts):
        alone, _, cnt1 = _pool(p, _offsets([len(p)]), pool)
        assert _same_bits(out[at], alone[0]) and np.array_equal(cnt[at], cnt1[0]), at
    if pool == "max":
        assert np.array_equal(out[2], big.max(axis=0))
        assert np.array_equal(cnt[2], (big == big.max(axis=0)).sum(axis=0)) and cnt[2, 0] == 3
    else:
        assert (cnt[2] == n).all()
        b64 = big.astype(np.float64)
        # the sum's bound of tests/test_gpu_condnet.py over n (float32(n) is exact), and the division's half ulp
        bsum = (n - 1) * 2.0**-24 * np.abs(b64).sum(axis=0) * (1 + 2.0**-20) / n
        bound = bsum + 2.0**-24 * (np.abs(b64.mean(axis=0)) + bsum)
        assert (np.abs(out[2] - b64.mean(axis=0)) <= bound).all()


@pytest.mark.parametrize("pool", ["max", "mean"])
def test_clamps_bad_device_offsets(pool):
    """The bad device offsets of tests/test_gpu_condnet.py::
    test_segment_sum_clamps_bad_device_offsets: finite results, equal to those
    of the clamped offsets and to the host's values for them."""
    from zenflow_amd import nn

    rng = np.random.default_rng(391)
    rows, F = 700, 3
    h = rng.standard_normal((rows, F)).astype(F32)
    for bad in BAD_OFFSETS:
        o = nn.clamp_offsets(bad, rows)
        got, idx, cnt = _pool(h, np.asarray(bad, np.int64), pool)
        want, widx, wcnt = _pool(h, o, pool)
        assert np.isfinite(got).all() and _same_bits(got, want), bad
        assert np.array_equal(idx, widx) and np.array_equal(cnt, wcnt)
        assert np.array_equal(idx, CO.ids_of(bad, rows).astype(np.int32))
        if pool == "max":
            assert np.array_equal(got, _host_max(h, o))
        else:
            ref = np.stack([h[o[s]:o[s + 1]].astype(np.float64).sum(axis=0) / max(1, o[s + 1] - o[s])
                            for s in range(len(o) - 1)])
            assert np.abs(got - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())
            assert np.array_equal(cnt[:, 0], np.diff(o))


# ---- networks ---------------------------------------------------------------------------
def _oracle(net, variables, x, off, mode="net", train=True, **extra):
    """The oracle's result for one job, from its CPU-only child process."""
    rows, S = len(x), len(off) - 1
    with tempfile.TemporaryDirectory() as d:
        job, out = Path(d) / "job.npz", Path(d) / "out.npz"
        CO.pack_job(job, _cfg(net), variables, x, CO.ids_of(off, rows), S, mode=mode, train=train, **extra)
        subprocess.run([sys.executable, "-m", "tests.pool_oracle", str(job), str(out)], cwd=ROOT, check=True,
                       timeout=600)
        return dict(np.load(out))


def _record(rec):
    from tests.test_gpu_flow import _append_record

    _append_record("pool_parity.jsonl", rec)


def _assert_gap(ref):
    """The precondition of the max cases (module docstring)."""
    gap, dmax = float(ref["gap64"]), float(ref["dmax64"])
    print(f"max: smallest top-two gap {gap:.3g}, max|d| {dmax:.3g}")
    assert gap >= 1e-4 * dmax, (gap, dmax)


IN_DIM = 3
# (pool, dropout, batch_norm, F): dropout x BatchNorm at F = 8, and F = 3 once
CASES = [("max", r, bn, 8) for r in (0.0, 0.25) for bn in (True, False)] + [("max", 0.25, True, 3)]
# the network / batch seed of each case, chosen on the CPU: the float64 oracle meets _assert_gap
CASE_SEED = {c: 0 for c in CASES}
CASE_SEED.update({("max", 0.0, True, 8): 2, ("max", 0.0, False, 8): 1, ("max", 0.25, True, 8): 2,
                  ("max", 0.25, False, 8): 1})


def _case(pool, dropout, batch_norm, F):
    s = CASE_SEED[(pool, dropout, batch_norm, F)]
    net, v = _net(F, IN_DIM, layers=(32, 32), dropout=dropout, batch_norm=batch_norm, pool=pool, seed=400 + s)
    x, off, rows = _batch(IN_DIM, 500 + s)
    return net, v, x, off, rows


@pytest.mark.parametrize("pool,dropout,batch_norm,F", CASES)
def test_network_train_parity(pool, dropout, batch_norm, F):
    """The train-mode c, the parameter gradient and backward(..., input_grad=
    True)'s gx for a random cotangent against the oracle, every element of
    every tensor; g has the same bits with and without input_grad."""
    from zenflow_amd import nn

    net, v, x, off, rows = _case(pool, dropout, batch_norm, F)
    S = len(off) - 1
    seed = 2**40 + 5
    gc = np.random.default_rng(5).standard_normal((S, F)).astype(F32)
    keep = nn.dropout_keep(seed, rows, F, dropout) if dropout else None
    ref = _oracle(net, v, x, off, keep=keep, gc=gc)
    if pool == "max":
        _assert_gap(ref)
    ct_ = nn.ConditionTrainer(net, v, IN_DIM, rows)
    c = ct_.forward(x, off, seed=seed)
    g = ct_.backward(gc)
    assert c.dtype == F32 and c.shape == (S, F) and not c[1].any()
    assert g.dtype == F32 and g.shape == (ct_.layout.size,) and not g[ct_.layout.param_mask == 0].any()
    c2 = ct_.forward(x, off, seed=seed)
    g2, gx = ct_.backward(gc, input_grad=True)
    assert np.array_equal(c2, c, equal_nan=True) and np.array_equal(g2, g) and gx.shape == (rows, IN_DIM)
    bad, rec = [], {"what": "train", "pool": pool, "dropout": dropout, "batch_norm": batch_norm, "F": F}
    _check(ref, "c", "", c, bad, rec)
    _check(ref, "gx", "", gx, bad, rec)
    tree = _leaves(ct_.grad_tree(g))
    assert set("g64:" + k for k in tree) == set(k for k in ref if k.startswith("g64:"))
    for k, a in tree.items():
        _check(ref, "g", ":" + k, a, bad, rec)
    _record(rec)
    assert not bad, bad
    if not batch_norm:
        assert not gx[-PAD:].any()  # rows in no set


@pytest.mark.parametrize("pool,dropout,batch_norm,F", CASES)
def test_network_eval_parity(pool, dropout, batch_norm, F):
    """The eval-mode c through ConditionNet.apply (no dropout, the stored
    statistics) against the oracle; the trainer's eval forward has its bits."""
    from zenflow_amd import nn

    net, v, x, off, rows = _case(pool, dropout, batch_norm, F)
    ref = _oracle(net, v, x, off, train=False)
    if pool == "max":
        _assert_gap(ref)
    c = net.apply(v, x, off)
    assert c.dtype == F32 and c.shape == (len(off) - 1, F) and not c[1].any()
    bad, rec = [], {"what": "eval", "pool": pool, "dropout": dropout, "batch_norm": batch_norm, "F": F}
    _check(ref, "c", "", c, bad, rec)
    _record(rec)
    assert not bad, bad
    assert np.array_equal(nn.ConditionTrainer(net, v, IN_DIM, rows).forward(x, off, train=False), c)


JOINT_SEED = 0


def test_joint_gradient_max():
    """pool="max", dropout 0.25, in front of a small conditional flow:
    tr.step(..., cond_grad=True) -> ct.backward(gc) against float64 autograd of
    the composed loss (the joint mode of the oracle)."""
    from tests.flowcases import _trainer
    from zenflow_amd import _lib as L
    from zenflow_amd import nn

    F, in_dim = 3, 2
    net, v = _net(F, in_dim, dropout=0.25, pool="max", seed=600 + JOINT_SEED)
    x, off, rows = _batch(in_dim, 610 + JOINT_SEED, extra_sets=[5, 9, 2, 31] * 6)
    S = len(off) - 1
    case = _flow_case(F, S, 620)
    seed = 9
    keep = nn.dropout_keep(seed, rows, F, net.dropout)
    ref = _oracle(net, v, x, off, mode="joint", keep=keep, model=case["model"], flow_variables=case["variables"],
                  y=case["x"])
    _assert_gap(ref)
    ct_ = nn.ConditionTrainer(net, v, in_dim, rows, sets_max=S)
    tr = _trainer(case, S)
    c = ct_.forward(L.DeviceArray.from_numpy(x), L.DeviceArray.from_numpy(off), seed=seed)
    assert isinstance(c, L.DeviceArray) and c.shape == (S, F)
    gc = tr.step(L.DeviceArray.from_numpy(case["x"]), c, cond_grad=True)
    assert isinstance(gc, L.DeviceArray)
    g = ct_.backward(gc)
    assert tr.last_loss() == pytest.approx(float(ref["loss64"]), rel=2e-5, abs=2e-5)
    bad, rec = [], {"what": "joint gradient", "pool": "max", "F": F}
    _check(ref, "c", "", c.numpy(), bad, rec)
    for k, a in _leaves(ct_.grad_tree(g.numpy())).items():
        _check(ref, "g", ":" + k, a, bad, rec)
    _record(rec)
    assert not bad, bad


@pytest.mark.parametrize("pool", ["max"])
def test_module_protocol(pool):
    """net.apply(v, x, off, train=True, mutable=["batch_stats"], seed=3)
    returns (c, updates) with the bits of ConditionTrainer.forward and of its
    statistics; host in, host out; DeviceArray in, DeviceArray out."""
    from zenflow_amd import _lib as L
    from zenflow_amd import nn

    net, v = _net(8, 2, dropout=0.25, pool=pool, seed=700)
    x, off, rows = _batch(2, 701)
    with pytest.raises(RuntimeError, match="mutable"):
        net.apply(v, x, off, train=True, seed=3)
    with pytest.raises(ValueError, match="offsets"):
        net.apply(v, x)
    c, upd = net.apply(v, x, off, train=True, mutable=["batch_stats"], seed=3)
    ct_ = nn.ConditionTrainer(net, v, 2, rows)
    want = ct_.forward(x, off, seed=3)
    assert isinstance(c, np.ndarray) and c.dtype == F32 and np.array_equal(c, want) and not c[1].any()
    stats = ct_.variables()["batch_stats"]["BatchNorm_0"]
    for k in ("mean", "var"):
        assert np.array_equal(upd["batch_stats"]["BatchNorm_0"][k], stats[k])
    cd, _ = net.apply(v, L.DeviceArray.from_numpy(x), L.DeviceArray.from_numpy(off), train=True,
                      mutable=["batch_stats"], seed=3)
    assert isinstance(cd, L.DeviceArray) and np.array_equal(cd.numpy(), c)
    ce = net.apply(v, L.DeviceArray.from_numpy(x), L.DeviceArray.from_numpy(off))
    assert isinstance(ce, L.DeviceArray) and np.array_equal(ce.numpy(), net.apply(v, x, off))
