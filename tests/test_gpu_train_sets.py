"""``zenflow_amd.train.train_sets`` on the GPU: the driver is the loop it
documents.  tests/dist_worker_sets.py writes that loop out from the older
primitives — NumPy gathers on the host and a fresh upload per batch, the
permutation, seed, metric and stopping rules of ``train()`` — and the driver,
which gathers every batch on the device out of a resident data set
(zf_segment_take), must return the same bits: a gather is exact, and the
trainers are called in the same order on the same values.

Common shapes: 96 sets of 1 - 12 elements in batches of 40 (40, 40 and a
short last batch of 16), six epochs, ``patience=1, warmup=0`` so that the
early-stopping test is live from the third epoch on."""

import os
from pathlib import Path

import numpy as np
import pytest

from tests import dist_worker_sets as W

pytestmark = pytest.mark.gpu
WORKER = str(Path(__file__).resolve().parent / "dist_worker_sets.py")
F32 = np.float32


def _assert_same(a, b, what):
    """Two packed results, bit for bit (the losses' lengths included)."""
    assert sorted(a) == sorted(b), what
    for k in a:
        u, v = np.asarray(a[k]), np.asarray(b[k])
        assert u.shape == v.shape, f"{what}: {k} {u.shape} vs {v.shape}"
        assert np.array_equal(u, v, equal_nan=True), f"{what}: {k} ({int(np.sum(u != v))} entries differ)"


@pytest.fixture(scope="module")
def data():
    return W.make_data()


@pytest.fixture(scope="module")
def default_run(data):
    """train_sets with its own initialisation and default optimisers."""
    from zenflow_amd.train import train_sets

    flow, phi = W.make_modules()
    return W.pack(train_sets(flow, phi, *data, progress=False, **W.RUN))


def test_driver_is_the_documented_loop(data, default_run):
    """(a) best_variables (every leaf), best_epoch, loss_train and loss_test."""
    flow, phi = W.make_modules()
    hand = W.pack(W.hand_loop(flow, phi, data, **W.RUN))
    assert 3 <= len(hand["loss_test"]) <= W.RUN["epochs"] and np.isfinite(hand["loss_test"]).all()
    assert any(k.startswith("v:flow/params/") for k in hand) and any(k.startswith("v:phi/batch_stats/") for k in hand)
    _assert_same(default_run, hand, "train_sets vs the hand-written loop")


def test_optimizer_chains_reach_their_trainers(data, default_run):
    """(b) optimizer= and phi_optimizer= (clip_by_global_norm + adamw chains)
    and initial_variables=: again the hand-written loop's bits, and not the
    default optimisers'."""
    from tests.test_gpu_condnet import _flow_case
    from zenflow_amd.train import train_sets

    S = len(data[1]) - 1
    flow, phi = W.make_modules()
    init = {"flow": _flow_case(3, S, 70)["variables"], "phi": phi.init(5, data[0], data[1])}
    opt, phi_opt = W.chains()
    got = W.pack(train_sets(flow, phi, *data, progress=False, optimizer=opt, phi_optimizer=phi_opt,
                            initial_variables=init, **W.RUN))
    flow, phi = W.make_modules()
    opt, phi_opt = W.chains()
    hand = W.pack(W.hand_loop(flow, phi, data, optimizer=opt, phi_optimizer=phi_opt, initial_variables=init, **W.RUN))
    _assert_same(got, hand, "chains")
    # either chain alone changes the result: each reaches its own trainer
    flow, phi = W.make_modules()
    only_flow = W.pack(train_sets(flow, phi, *data, progress=False, optimizer=W.chains()[0], initial_variables=init,
                                  **dict(W.RUN, epochs=1)))
    flow, phi = W.make_modules()
    only_phi = W.pack(train_sets(flow, phi, *data, progress=False, phi_optimizer=W.chains()[1],
                                 initial_variables=init, **dict(W.RUN, epochs=1)))
    flow, phi = W.make_modules()
    neither = W.pack(train_sets(flow, phi, *data, progress=False, initial_variables=init, **dict(W.RUN, epochs=1)))
    def kernels(run, net):
        keys = sorted(k for k in run if k.startswith(f"v:{net}/params/") and k.endswith("/kernel"))
        assert keys, sorted(run)
        return np.concatenate([run[k].ravel() for k in keys])

    assert not np.array_equal(kernels(only_flow, "flow"), kernels(neither, "flow"))
    assert not np.array_equal(kernels(only_phi, "phi"), kernels(neither, "phi"))


def test_notebook_toy_converges():
    """(c) Y ~ N(0.3 sqrt(n), 0.2) for a set of n elements (both columns, the
    second with the sign flipped): the set's size is all the condition can
    carry, through the pooled sum.  256 sets of 1 - 20 elements, 30 epochs of
    four batches."""
    from zenflow_amd import nn
    from zenflow_amd.train import nadamw, train_sets

    def split(S, seed):
        rng = np.random.default_rng(seed)
        n = rng.integers(1, 21, S)
        off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        X = rng.standard_normal((int(off[-1]), 2)).astype(F32)
        mu = 0.3 * np.sqrt(n)[:, None] * np.array([1.0, -1.0])
        return X, off, (mu + 0.2 * rng.standard_normal((S, 2))).astype(F32)

    flow, _ = W.make_modules()
    phi = nn.ConditionNet(3, layers=(16, 16), dropout=0.25, pool="sum")
    train, test = split(256, 11), split(128, 12)
    pv0 = phi.init(1, train[0], train[1])
    best, best_epoch, loss_train, loss_test = train_sets(
        flow, phi, *train, *test, epochs=30, batch_sets=64, patience=30, warmup=0, seed=0, progress=False,
        optimizer=nadamw(2e-3), phi_optimizer=nadamw(2e-3))
    print("loss_test", [round(v, 4) for v in loss_test])
    assert len(loss_test) == len(loss_train) == 30
    assert np.isfinite(loss_test).all() and np.isfinite(loss_train).all()
    assert np.mean(loss_test[-5:]) < np.mean(loss_test[:5])
    assert 0 <= best_epoch < 30 and loss_test[best_epoch] == min(loss_test)
    k0, k1 = W.leaves(pv0["params"]), W.leaves(best["phi"]["params"])
    assert sorted(k0) == sorted(k1)
    assert all(np.isfinite(k1[k]).all() for k in k1)
    assert not np.array_equal(k0["NNBlock_0/Dense_0/kernel"], k1["NNBlock_0/Dense_0/kernel"])
    assert not np.array_equal(k0["NNBlock_0/Dense_2/kernel"], k1["NNBlock_0/Dense_2/kernel"])


def test_two_ranks_agree_with_each_other_and_the_documented_loop(tmp_path, default_run):
    """(d) two ranks on one GPU (dist.HostAllgather): both return identical
    results, and those of the hand-written data-parallel loop on the same
    shards.  (One device's bits are another fixed-order sum: random ragged
    shards do not have equal element rows.)"""
    from zenflow_amd.launch import spawn

    env = dict(os.environ, ZF_DEVICE="0")
    assert spawn(2, [WORKER, str(tmp_path)], env=env, timeout=240) == 0
    ranks = [dict(np.load(tmp_path / f"rank{k}.npz")) for k in range(2)]
    runs = [{which: {k.split(":", 1)[1]: a for k, a in r.items() if k.startswith(which + ":")}
             for which in ("driver", "hand")} for r in ranks]
    assert len(runs[0]["driver"]) == len(default_run)
    _assert_same(runs[0]["driver"], runs[1]["driver"], "rank 0 vs rank 1")
    for k in range(2):
        _assert_same(runs[k]["driver"], runs[k]["hand"], f"rank {k}: train_sets vs the hand-written loop")
    assert np.isfinite(runs[0]["driver"]["loss_test"]).all() and len(runs[0]["driver"]["loss_test"]) >= 3
