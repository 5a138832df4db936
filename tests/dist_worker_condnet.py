"""Rank program and shared cases of tests/test_gpu_condnet_dp.py: one rank of a
data-parallel ``nn.ConditionTrainer`` on its whole sets of a global batch.
Ranks share one GPU through dist.HostAllgather (as tests/dist_worker.py's
``train_dp``) or, with ZF_TEST_RCCL=1, drive one GPU each over RCCL.  Each
rank writes <outdir>/rank<r>.npz.

    python tests/dist_worker_condnet.py <mode> <outdir>     (ZF_TEST_CASE = the case as JSON)

modes: ``bitwise`` (equal shards: run_sequence), ``joint`` (phi -> flow trainer
-> phi.step), ``uneven`` (shard_sets, explicit global_rows / row_base)."""

import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

F32 = np.float32
STEPS = 3


def rank_lengths(rows, rank_seed):
    """Set lengths of one rank's ``rows`` element rows (equal shards)."""
    rng = np.random.default_rng(7000 + rank_seed)
    if rows == 256:  # 12 sets, one of them empty
        n = [1, 0, 63, 64, 65, 9, 30, 4, 7, 5, 6, 2]
    elif rows == 1024:  # one set longer than a chunk of 512: two chunks, a second level
        n = [600, 1, 63, 64, 65, 100, 131]
    else:  # 200 sets of about rows / 200 rows
        n = list(rng.multinomial(rows, np.ones(200) / 200))
    assert sum(n) == rows, (rows, sum(n))
    return [int(n[k]) for k in rng.permutation(len(n))]


def make_case(cfg):
    """The global batch of a case, the same in every process: net, variables,
    x (rows, in_dim), offsets over all sets (None without pooling), the global
    cotangent gc and the optimiser's constructor."""
    from tests.test_gpu_condnet import _net
    from zenflow_amd import optim
    from zenflow_amd.train import Optimizer

    rows, world, seed = int(cfg["rows"]), int(cfg.get("world", 2)), int(cfg["seed"])
    in_dim, F, pool = int(cfg.get("in_dim", 2)), int(cfg.get("F", 3)), cfg["pool"]
    net, v = _net(F, in_dim, layers=tuple(cfg.get("layers", (32, 32))), batch_norm=bool(cfg["bn"]),
                  dropout=float(cfg["dropout"]), pool=pool, seed=seed)
    rng = np.random.default_rng(3000 + seed)
    x = (rng.standard_normal((rows, in_dim)) * (1 + 0.5 * np.arange(in_dim)) + 0.3).astype(F32)
    off = None
    if pool is not None:
        if "lengths" in cfg:
            lengths = [int(n) for n in cfg["lengths"]]
        else:
            lengths = sum((rank_lengths(rows // world, 10 * seed + r) for r in range(world)), [])
        off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        assert off[-1] == rows
    n_out = rows if off is None else len(off) - 1
    gc = rng.standard_normal((n_out, F)).astype(F32)

    def optimizer():
        if cfg["opt"] == "nadamw":
            return Optimizer(learning_rate=1e-3)
        if cfg["opt"] == "chain":
            return optim.chain(optim.clip_by_global_norm(1.0), optim.adamw(1e-3))
        raise ValueError(cfg["opt"])

    return {"net": net, "v": v, "x": x, "off": off, "gc": gc, "optimizer": optimizer, "in_dim": in_dim, "F": F,
            "seed": 11 + seed}


def opt_arrays(ct):
    """ConditionTrainer.opt_state() as flat arrays."""
    st = ct.opt_state()
    slots = np.stack([ct.layout.to_blob({"params": t}, cols=("params",)) for t in st["slots"]])
    return {"opt_count": np.int64(st["count"]), "opt_lr": np.float64(st["learning_rate"]),
            "opt_norm": np.float64(st["grad_norm"]), "opt_slots": slots}


def run_sequence(ct, x, off, gc, seed, **shard):
    """What the bitwise tests compare, on one device or on one rank: c, the
    gradient with and without the input gradient, gx, and after STEPS steps
    the blob and the optimiser state."""
    out = {"c": ct.forward(x, off, seed=seed, **shard)}
    out["grad"], out["gx"] = ct.backward(gc, input_grad=True)
    ct.forward(x, off, seed=seed, **shard)
    out["grad_plain"] = ct.backward(gc)
    for t in range(STEPS):
        ct.forward(x, off, seed=seed + 1 + t, **shard)
        ct.step(gc)
    out["blob"] = ct._h.blob()
    out.update(opt_arrays(ct))
    return out


def local_part(case, rank, world, even=True, even_sets=False):
    """This rank's (x, offsets, gc, shard keywords, [s0, s1), [r0, r1)) of a
    case.  even: equal element rows, the defaults of ``forward``; even_sets:
    equal sets as well (the joint loop)."""
    from zenflow_amd import nn
    from zenflow_amd.dist import shard_rows

    x, off, gc = case["x"], case["off"], case["gc"]
    if off is None:
        r0, r1 = shard_rows(len(x), rank, world)
        s0, s1, loc = r0, r1, None
    elif even_sets:
        s0, s1 = shard_rows(len(off) - 1, rank, world)
        r0, r1 = int(off[s0]), int(off[s1])
        assert (r0, r1) == shard_rows(len(x), rank, world)
        loc = off[s0:s1 + 1] - off[s0]
    elif even:  # equal element rows: the offsets hold every rank's boundary
        r0, r1 = shard_rows(len(x), rank, world)
        s0, s1 = int(np.searchsorted(off, r0, "left")), int(np.searchsorted(off, r1, "left"))
        if rank == 0:
            s0 = 0
        if rank == world - 1:
            s1 = len(off) - 1
        assert off[s0] == r0 and off[s1] == r1
        loc = off[s0:s1 + 1] - off[s0]
    else:
        s0, s1, r0, r1 = nn.shard_sets(off, rank, world)
        loc = off[s0:s1 + 1] - off[s0]
    shard = {} if even else {"global_rows": len(x), "row_base": r0}
    return x[r0:r1], loc, gc[s0:s1], shard, (s0, s1), (r0, r1)


def _comm(rdzv):
    from zenflow_amd.dist import HostAllgather, RcclCommunicator

    if os.environ.get("ZF_TEST_RCCL") == "1":
        return RcclCommunicator(rdzv.rank, rdzv.world, lambda u: rdzv.broadcast_bytes(u, tag="rccl_uid"))
    return HostAllgather(rdzv)


def main(mode, outdir):
    from zenflow_amd import nn
    from zenflow_amd.launch import FileRendezvous

    rdzv = FileRendezvous.from_env(timeout=120)
    rank, world = rdzv.rank, rdzv.world
    cfg = json.loads(os.environ["ZF_TEST_CASE"])
    case = make_case(cfg)
    comm = _comm(rdzv)
    x, off, gc, shard, (s0, s1), (r0, r1) = local_part(case, rank, world, even=mode != "uneven",
                                                       even_sets=mode == "joint")
    sets_max = max(1, s1 - s0)
    ct = nn.ConditionTrainer(case["net"], case["v"], case["in_dim"], len(x), sets_max=sets_max,
                             optimizer=case["optimizer"](), comm=comm)
    if mode in ("bitwise", "uneven"):
        out = run_sequence(ct, x, off, gc, case["seed"], **shard)
    elif mode == "joint":
        from tests.flowcases import _trainer
        from tests.test_gpu_condnet import _flow_case

        S = len(case["off"]) - 1
        fc = _flow_case(case["F"], S, cfg["flow_seed"])
        tr = _trainer(fc, s1 - s0, comm=comm)
        out = joint_loop(ct, tr, x, off, fc["x"][s0:s1], case["seed"], global_sets=S)
    else:
        raise ValueError(mode)
    np.savez(Path(outdir, f"rank{rank}.npz"), s0=s0, s1=s1, r0=r0, r1=r1, **out)
    rdzv.close()
    if hasattr(comm, "comm"):
        comm.close()


def joint_loop(ct, tr, x, off, y, seed, global_sets=None):
    """The notebook's joint loop, STEPS steps: phi -> the flow's step with d loss / d c -> phi's step."""
    from tests.flowcases import _blob

    losses = []
    for t in range(STEPS):
        c = ct.forward(x, off, seed=seed + t)
        gc = tr.step(y, c, cond_grad=True, global_rows=global_sets)
        ct.step(gc)
        losses.append(tr.last_loss())
    return {"blob": ct._h.blob(), "flow_blob": _blob(tr), "losses": np.asarray(losses, np.float64), **opt_arrays(ct)}


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
