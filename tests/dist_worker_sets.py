"""Shared case, hand-written loop and rank program of
tests/test_gpu_train_sets.py: ``zenflow_amd.train.train_sets`` against the
loop it documents, written out from the primitives that were there before it
(NumPy gathers on the host, a fresh upload per batch, ``ConditionTrainer`` and
``Trainer``).  As a program it is one rank of two that share one GPU through
dist.HostAllgather (the pattern of tests/dist_worker_condnet.py): the rank runs
``train_sets(comm=)`` and then the hand-written data-parallel loop on the same
shards, and writes both results to <outdir>/rank<r>.npz.

    python tests/dist_worker_sets.py <outdir>"""

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

F32 = np.float32
CFG = dict(D=2, C=3, K=8, layers=(32, 32), latent="beta")  # the flow of tests/test_gpu_condnet.py::_flow_case
RUN = dict(epochs=6, batch_sets=40, patience=1, warmup=0, seed=3)


def make_data(S=96, longest=12, seed=0):
    """(X, offsets, Y) of a train and of a test split: S sets of 1 .. longest elements, in_dim 2."""
    out = []
    for k, n_sets in enumerate((S, S // 2)):
        rng = np.random.default_rng(100 * seed + k)
        lengths = rng.integers(1, longest + 1, n_sets)
        off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        X = (rng.standard_normal((int(off[-1]), 2)) + 0.2).astype(F32)
        Y = (rng.standard_normal((n_sets, 2)) * 0.5 + 0.1 * np.sqrt(lengths)[:, None]).astype(F32)
        out += [X, off, Y]
    return tuple(out)


def make_modules():
    from tests.flowcases import build_flow
    from zenflow_amd import nn

    return build_flow(CFG), nn.ConditionNet(3, layers=(16, 16), dropout=0.25, pool="sum")


def chains():
    """A clip_by_global_norm + adamw chain for the flow and one for phi."""
    from zenflow_amd import optim

    return (optim.chain(optim.clip_by_global_norm(1.0), optim.adamw(2e-3)),
            optim.chain(optim.clip_by_global_norm(0.5), optim.adamw(5e-4)))


def leaves(tree, prefix=""):
    """A variables tree as {path: array}."""
    out = {}
    for k, v in tree.items():
        if isinstance(v, dict):
            out.update(leaves(v, f"{prefix}{k}/"))
        else:
            out[prefix + k] = np.asarray(v)
    return out


def pack(result):
    """(best_variables, best_epoch, loss_train, loss_test) as flat arrays."""
    variables, best_epoch, loss_train, loss_test = result
    out = {"v:" + k: a for k, a in leaves(variables).items()}
    out.update(best_epoch=np.int64(best_epoch), loss_train=np.asarray(loss_train, np.float64),
               loss_test=np.asarray(loss_test, np.float64))
    return out


def metric(flow, phi, variables, X, off, Y):
    """The eval-mode metric through the modules' public API."""
    from zenflow_amd.dist import nll_from_sum

    c = phi.apply(variables["phi"], X, off)
    lp = np.asarray(flow.apply(variables["flow"], Y, c), np.float64)
    return nll_from_sum(lp.sum(), lp.shape[0])


def hand_loop(flow, phi, data, *, epochs, batch_sets, patience, warmup, seed, optimizer=None, phi_optimizer=None,
              initial_variables=None, comm=None):
    """The loop train_sets stands for ("Training a deep-set
    flow in one call"), one device or one rank of ``comm``: every batch is
    gathered by NumPy on the host and uploaded."""
    import zenflow_amd as zf
    from zenflow_amd import nn
    from zenflow_amd._lib import DeviceArray
    from zenflow_amd.dist import shard_rows
    from zenflow_amd.train import Trainer

    X, off, Y, Xt, offt, Yt = data
    S = len(off) - 1
    rank, world = (0, 1) if comm is None else (comm.rank, comm.world)
    variables = initial_variables
    if variables is None:
        variables = {"flow": flow.init(zf.PRNGKey(seed), Y[:1], np.zeros((1, phi.features), F32)),
                     "phi": phi.init(seed + 1, X, off)}
    # capacities of its own choosing: the whole data set
    tr = Trainer(flow, variables["flow"], Y.shape[1], phi.features, min(batch_sets, S), optimizer, comm=comm)
    ct = nn.ConditionTrainer(phi, variables["phi"], X.shape[1], len(X), sets_max=S, optimizer=phi_optimizer,
                             comm=comm)

    def gather(sets):
        rows = np.concatenate([np.arange(off[s], off[s + 1]) for s in sets])
        loc = np.concatenate([[0], np.cumsum(off[sets + 1] - off[sets])]).astype(np.int64)
        return X[rows], loc, Y[sets]

    loss_train, loss_test, best_epoch, best, step = [], [], 0, variables, 0
    for epoch in range(epochs):
        perm = np.random.default_rng([seed, epoch]).permutation(S)
        for first in range(0, S, batch_sets):
            batch = perm[first:first + batch_sets]
            lo, hi = shard_rows(len(batch), rank, world)
            xb, ob, yb = (DeviceArray.from_numpy(a) for a in gather(batch[lo:hi]))
            lengths = off[batch + 1] - off[batch]
            shard = {} if comm is None else {"global_rows": int(lengths.sum()), "row_base": int(lengths[:lo].sum())}
            c = ct.forward(xb, ob, seed=seed * 2**32 + step, **shard)
            gc = tr.step(yb, c, cond_grad=True, global_rows=len(batch))
            ct.step(gc)
            step += 1
        variables = {"flow": tr.variables(), "phi": ct.variables()}
        loss_train.append(metric(flow, phi, variables, *gather(batch)))
        loss_test.append(metric(flow, phi, variables, Xt, offt, Yt))
        if not np.isfinite(loss_train[-1]):
            break
        if loss_test[-1] <= loss_test[best_epoch]:
            best_epoch, best = epoch, variables
        if epoch >= warmup and epoch >= 2 * patience and epoch % patience == 0:
            if not np.min(loss_test[-patience:]) < np.min(loss_test[-2 * patience:-patience]):
                break
    return best, best_epoch, loss_train, loss_test


def main(outdir):
    from tests.dist_worker_condnet import _comm
    from zenflow_amd.launch import FileRendezvous
    from zenflow_amd.train import train_sets

    rdzv = FileRendezvous.from_env(timeout=120)
    comm = _comm(rdzv)
    data = make_data()
    flow, phi = make_modules()
    out = {"driver:" + k: a for k, a in pack(train_sets(flow, phi, *data, progress=False, comm=comm, **RUN)).items()}
    flow, phi = make_modules()
    out.update({"hand:" + k: a for k, a in pack(hand_loop(flow, phi, data, comm=comm, **RUN)).items()})
    np.savez(Path(outdir, f"rank{rdzv.rank}.npz"), **out)
    rdzv.close()
    if hasattr(comm, "comm"):
        comm.close()


if __name__ == "__main__":
    main(sys.argv[1])
