"""Data-parallel ``nn.ConditionTrainer`` (zf_condnet_set_comm,
zf_condnet_forward_shard) and its optimiser state (zf_condnet_*_opt_*).

Two ranks share this box's one GPU (tests/dist_worker_condnet.py; the
all-gathers go through dist.HostAllgather, since RCCL refuses two ranks on one
device), each holding whole sets of every global batch.  BatchNorm's sums and
the weight gradients are the trainer's fixed leaf trees, whose shape depends on
the global batch only, the dropout mask is a function of the global row, and
the pooling is per set: with equal shards both ranks must end with the bits ONE
device gets on the concatenated batch — ``array_equal``, not a tolerance.  With
uneven shards the ranks still agree bit for bit with each other, and are held
to the float64 oracle by the parity rule of tests/test_gpu_condnet.py.

Shapes of the bitwise cases (global element rows): 512 is 16 leaves of 32 rows,
8 per rank, the smallest batch with a real subtree per rank, in 24 sets of
which one per rank is empty; 2,048 has a set of 600 rows on each rank (two
chunks of the segmented reduction, a second level); 65,536 is the global batch
at which the Dense GEMMs switch to 128-row tiles, so a 32,768-row shard must
switch too."""

import ctypes
import json
import os
from pathlib import Path

import numpy as np
import pytest

from tests import dist_worker_condnet as W
from tests.test_gpu_condnet import _check, _flow_case, _leaves
from tests.test_gpu_deepset import _oracle  # tests/test_gpu_condnet.py's, with the input gradient (gx64)

pytestmark = pytest.mark.gpu
WORKER = str(Path(__file__).resolve().parent / "dist_worker_condnet.py")
F32 = np.float32
COMPARED = ("grad", "grad_plain", "blob", "opt_count", "opt_lr", "opt_norm", "opt_slots")


def _spawn(mode, cfg, tmp_path, rccl=False):
    from zenflow_amd.launch import spawn

    env = dict(os.environ, ZF_TEST_CASE=json.dumps(cfg), ZF_DEVICE="0")
    if rccl:
        env.pop("ZF_DEVICE")  # one GPU per rank (LOCAL_RANK)
        env["ZF_TEST_RCCL"] = "1"
    assert spawn(2, [WORKER, mode, str(tmp_path)], env=env, timeout=240) == 0
    return [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]


def _trainer_of(case, **kw):
    from zenflow_amd import nn

    S = 1 if case["off"] is None else len(case["off"]) - 1
    return nn.ConditionTrainer(case["net"], case["v"], case["in_dim"], len(case["x"]), sets_max=S,
                               optimizer=case["optimizer"](), **kw)


def _one_device(case):
    return W.run_sequence(_trainer_of(case), case["x"], case["off"], case["gc"], case["seed"])


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _assert_ranks_match_one_device(ranks, one):
    for k, r in enumerate(ranks):
        s0, s1, r0, r1 = (int(r[n]) for n in ("s0", "s1", "r0", "r1"))
        assert _same(r["c"], one["c"][s0:s1]), f"rank {k}: c"
        assert _same(r["gx"], one["gx"][r0:r1]), f"rank {k}: {np.sum(r['gx'] != one['gx'][r0:r1])} gx entries differ"
        for name in COMPARED:
            assert _same(r[name], one[name]), f"rank {k}: {name} ({np.sum(r[name] != one[name])} entries differ)"
        assert int(r["opt_count"]) == W.STEPS


# (global rows, BatchNorm, dropout, pool, optimiser)
BITWISE = [(512, True, 0.3, "sum", "nadamw"), (512, True, 0.0, "max", "chain"), (512, False, 0.3, "sum", "nadamw"),
           (512, True, 0.3, None, "chain"), (2048, True, 0.3, "sum", "chain"), (2048, True, 0.3, "max", "nadamw"),
           (2048, False, 0.0, None, "nadamw"), (65536, True, 0.3, "sum", "nadamw")]


def _cfg(rows, bn, dropout, pool, opt, seed):
    return {"rows": rows, "bn": bn, "dropout": dropout, "pool": pool, "opt": opt, "seed": seed}


@pytest.mark.parametrize("rows,bn,dropout,pool,opt", BITWISE)
def test_two_ranks_match_one_device_bitwise(tmp_path, rows, bn, dropout, pool, opt):
    """This rank's rows of c and of gx, the gradient (with and without the
    input gradient), and after three steps the blob and the optimiser state.
    With dropout this is the row_base check: with the local row as the
    mask's index rank 1 would draw rank 0's mask."""
    cfg = _cfg(rows, bn, dropout, pool, opt, BITWISE.index((rows, bn, dropout, pool, opt)))
    ranks = _spawn("bitwise", cfg, tmp_path)
    _assert_ranks_match_one_device(ranks, _one_device(W.make_case(cfg)))


def test_rccl_two_ranks_match_one_device_bitwise(tmp_path):
    """The product path: ConditionTrainer(comm=RcclCommunicator), one rank per
    GPU, every exchange an ncclAllGather of the ranks' fp64 roots."""
    from zenflow_amd import _lib as L

    if L.device_count() < 2:
        pytest.skip("needs 2 GPUs (RCCL refuses two ranks on one device)")
    if not L.load_library().zf_rccl_available():
        pytest.skip("librccl not present on this box")
    cfg = _cfg(2048, True, 0.3, "sum", "chain", 40)
    ranks = _spawn("bitwise", cfg, tmp_path, rccl=True)
    _assert_ranks_match_one_device(ranks, _one_device(W.make_case(cfg)))


def test_joint_loop_two_ranks_match_one_device_bitwise(tmp_path):
    """The notebook's joint loop under data parallelism: phi -> Trainer(comm=)
    with cond_grad=True -> phi.step, three steps, 512 element rows in 64 sets,
    32 sets and 256 rows per rank.  Both ranks' phi blob, flow blob and losses
    are the one-device loop's."""
    from tests.flowcases import _trainer

    rng = np.random.default_rng(5)
    lengths = [int(n) for r in range(2) for n in rng.multinomial(256, np.ones(32) / 32)]
    cfg = dict(_cfg(512, True, 0.3, "sum", "nadamw", 21), lengths=lengths, flow_seed=70)
    ranks = _spawn("joint", cfg, tmp_path)
    case = W.make_case(cfg)
    S = len(case["off"]) - 1
    assert S == 64
    fc = _flow_case(case["F"], S, cfg["flow_seed"])
    one = W.joint_loop(_trainer_of(case), _trainer(fc, S), case["x"], case["off"], fc["x"], case["seed"])
    assert np.isfinite(one["losses"]).all()
    for k, r in enumerate(ranks):
        assert (int(r["s1"]) - int(r["s0"]), int(r["r1"]) - int(r["r0"])) == (32, 256)
        for name in ("losses", "blob", "flow_blob", "opt_count", "opt_slots"):
            assert _same(r[name], one[name]), f"rank {k}: {name} ({np.sum(r[name] != one[name])} entries differ)"


def test_uneven_shards(tmp_path):
    """23 sets split 12 / 11 by nn.shard_sets, 256 and 280 element rows, with
    explicit global_rows / row_base.  The ranks' gradients, stepped blobs and
    optimiser states are equal bit for bit; the concatenated c, every
    parameter gradient and gx are held to the float64 oracle on the
    concatenated batch (dropout mask over global rows) by the parity rule."""
    from tests.test_gpu_flow import _append_record
    from zenflow_amd import nn

    lengths = [1, 0, 63, 64, 65, 9, 30, 4, 7, 5, 6, 2, 40, 3, 0, 17, 80, 1, 33, 12, 64, 21, 9]
    cfg = dict(_cfg(536, True, 0.3, "sum", "nadamw", 31), lengths=lengths)
    a, b = _spawn("uneven", cfg, tmp_path)
    assert [int(a[n]) for n in ("s0", "s1", "r0", "r1")] == [0, 12, 0, 256]
    assert [int(b[n]) for n in ("s0", "s1", "r0", "r1")] == [12, 23, 256, 536]
    for name in COMPARED:
        assert _same(a[name], b[name]), name
    case = W.make_case(cfg)
    net, x, off = case["net"], case["x"], case["off"]
    keep = nn.dropout_keep(case["seed"], len(x), case["F"], net.dropout)
    ref = _oracle(net, case["v"], x, off, keep=keep, gc=case["gc"])
    bad, rec = [], {"what": "uneven shards", "sets": [12, 11], "rows": [256, 280]}
    _check(ref, "c", "", np.concatenate([a["c"], b["c"]]), bad, rec)
    _check(ref, "gx", "", np.concatenate([a["gx"], b["gx"]]), bad, rec)
    layout = net._layout(case["in_dim"])
    for k, t in _leaves(layout.to_tree(a["grad"], cols=("params",))["params"]).items():
        _check(ref, "g", ":" + k, t, bad, rec)
    _append_record("condnet_dp_parity.jsonl", rec)
    assert not bad, bad


def _resume_optimizers():
    from zenflow_amd import optim
    from zenflow_amd.train import nadamw

    return {"nadamw": lambda: nadamw(1e-3),
            "warmup_chain": lambda: optim.chain(optim.clip_by_global_norm(1.0), optim.adamw(
                optim.warmup_cosine_decay_schedule(0.0, 1e-3, 4, 20)))}


@pytest.mark.parametrize("which", ["nadamw", "warmup_chain"])
def test_resume(which):
    """Six steps straight against three steps, variables() and opt_state()
    into a new ConditionTrainer, three more: the same blob and optimiser
    state (the chain's schedule is still warming up at the hand-over)."""
    from zenflow_amd import nn

    make = _resume_optimizers()[which]
    case = W.make_case(_cfg(512, True, 0.3, "sum", "nadamw", 51))
    x, off, gc, seed = case["x"], case["off"], case["gc"], case["seed"]
    S = len(off) - 1

    def new(variables):
        return nn.ConditionTrainer(case["net"], variables, case["in_dim"], len(x), sets_max=S, optimizer=make())

    def steps(ct, t0, t1):
        for t in range(t0, t1):
            ct.forward(x, off, seed=seed + t)
            ct.step(gc)

    straight = new(case["v"])
    steps(straight, 0, 6)
    first = new(case["v"])
    steps(first, 0, 3)
    state = first.opt_state()
    assert state["count"] == 3 and len(state["slots"]) == 2
    second = new(first.variables())
    second.load_opt_state(state)
    assert second.opt_state()["count"] == 3
    steps(second, 3, 6)
    assert np.array_equal(second._h.blob(), straight._h.blob())
    a, b = W.opt_arrays(second), W.opt_arrays(straight)
    assert int(a["opt_count"]) == 6
    for name in a:
        assert _same(a[name], b[name]), name
    with pytest.raises(ValueError, match="moment arrays"):
        second.load_opt_state(dict(state, slots=state["slots"][:1]))


class _World1:
    """A communicator of one rank."""

    rank, world = 0, 1

    def trainer_comm_desc(self):
        from zenflow_amd import _lib as L

        return L.ZfCommDesc(0, 1, None, None)


def test_one_device_unchanged():
    """Without comm, with a world-1 comm, and with global_rows=rows,
    row_base=0 spelled out: the same c, gradient and gx."""
    case = W.make_case(_cfg(512, True, 0.3, "sum", "nadamw", 61))
    x, off, gc, seed = case["x"], case["off"], case["gc"], case["seed"]
    outs = []
    for kw, shard in (({}, {}), ({"comm": _World1()}, {}), ({}, {"global_rows": len(x), "row_base": 0})):
        ct = _trainer_of(case, **kw)
        c = ct.forward(x, off, seed=seed, **shard)
        g, gx = ct.backward(gc, input_grad=True)
        outs.append((c, g, gx))
    for other in outs[1:]:
        for u, w in zip(outs[0], other):
            assert np.array_equal(u, w)
    ct = _trainer_of(case)
    for bad in ({"global_rows": len(x) + 1, "row_base": 0}, {"global_rows": len(x), "row_base": 1},
                {"global_rows": len(x) - 1, "row_base": 0}, {"global_rows": len(x), "row_base": -1}):
        with pytest.raises(ValueError, match="global_rows"):
            ct.forward(x, off, seed=seed, **bad)


def test_c_entry_rejections():
    """The C entries themselves: the codes and the zf_last_error text, each before anything is enqueued."""
    from zenflow_amd import _lib as L

    lib = L.load_library()
    case = W.make_case(_cfg(512, True, 0.3, "sum", "nadamw", 71))
    x, off = case["x"], case["off"]
    rows, S = len(x), len(off) - 1
    ct = _trainer_of(case)
    h = ct.handle
    cb = L.ALLGATHER_FN(lambda ctx, send, recv, nbytes, stream: 1)  # never reached
    fn = ctypes.cast(cb, ctypes.c_void_p).value

    def set_comm(rank, world, allgather):
        return lib.zf_condnet_set_comm(h, ctypes.byref(L.ZfCommDesc(rank, world, None, allgather)))

    for rank, world in ((2, 2), (-1, 2), (0, 0), (0, -3)):
        assert set_comm(rank, world, fn) == -1 and b"bad rank" in lib.zf_last_error()
    assert set_comm(0, 2, None) == -1 and b"without allgather" in lib.zf_last_error()
    assert set_comm(0, 65, fn) == -2 and b"64 ranks" in lib.zf_last_error()
    assert lib.zf_condnet_set_comm(None, None) == -1

    xd, od, out = L.DeviceArray.from_numpy(x), L.DeviceArray.from_numpy(off), L.DeviceArray((S, case["F"]))

    def shard(global_rows, row_base, n=rows):
        return lib.zf_condnet_forward_shard(h, xd.ptr, n, global_rows, row_base, od.ptr, S, 1, 1, 0, out.ptr,
                                            L.stream())

    # world 1: the global pass is this pass
    assert shard(rows + 1, 0) == -1 and b"global_rows" in lib.zf_last_error()
    assert shard(rows, 0) == 0
    assert set_comm(0, 2, fn) == 0  # drops the pending pass
    assert lib.zf_condnet_backward(h, out.ptr, None, L.stream()) == -1 and b"no forward pending" in lib.zf_last_error()
    for global_rows, row_base in ((rows - 1, 0), (2 * rows, -1), (2 * rows, rows + 1), (rows, 1)):
        assert shard(global_rows, row_base) == -1 and b"global_rows" in lib.zf_last_error(), (global_rows, row_base)
        assert lib.zf_condnet_backward(h, out.ptr, None, L.stream()) == -1  # nothing was enqueued, nothing is pending
    assert lib.zf_condnet_set_comm(h, None) == 0  # one device again
    assert shard(rows, 0) == 0

    buf = np.zeros(ct.layout.size, F32)
    for slot in (-1, 2):
        assert lib.zf_condnet_get_opt_slot(h, slot, buf.ctypes.data) == -1 and b"optimiser slot" in lib.zf_last_error()
        assert lib.zf_condnet_set_opt_slot(h, slot, buf.ctypes.data) == -1
    assert lib.zf_condnet_get_opt_slot(h, 0, None) == -1
    assert lib.zf_condnet_get_opt_slot(h, 1, buf.ctypes.data) == 0
    assert lib.zf_condnet_set_opt_count(h, -1) == -1 and b"optimiser count" in lib.zf_last_error()
    assert lib.zf_condnet_set_opt_count(h, 2**31) == -1
