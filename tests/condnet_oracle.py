"""Oracle of the conditioning network (zenflow_amd/nn.py, zf_condnet_*) for
tests/test_condnet_host.py and tests/test_gpu_condnet.py: a torch restatement
of examples/deep_set.ipynb's ``Phi``,

    BatchNorm -> (Dense, act) x depth -> Dense -> dropout with a GIVEN mask
    -> segment sum,

in float64 and float32, composed with ``tests/input_grad_oracle.py::flow_lp``
for the joint loss of ``loss_fn_2``.  JAX is not importable here, so the FLAX
layers are restated from their published definitions (flax.linen.BatchNorm:
biased variance max(0, E[u^2] - E[u]^2), eps 1e-5, momentum 0.99; Dense:
x @ kernel + bias; Dropout: where(keep, x / (1 - rate), 0)), not pinned to
FLAX.  The dropout mask is an input: the device's Philox rule is restated in
``zenflow_amd.nn.dropout_keep`` and pinned on its own.

The sets enter as ``ids`` (the set of every row, -1 for none), so that the
rows can be permuted: the float32 evaluation runs over three row orders (the
rounding any fp32 summation is subject to), and float64 runs again at inputs
and parameters jittered by 2^-22 relative (the conditioning), as
tests/grad_oracle.py does for the flow.

Runs in its own CPU-only process (importing torch into the GPU test process
would shadow the system librccl there):

    python -m tests.condnet_oracle JOB.npz OUT.npz

JOB.npz (``pack_job``): ``cfg`` (JSON: layers, features, act, batch_norm,
dropout, pool), ``mode`` ("net" | "joint" | "traj"), ``x``, ``ids``, ``S``,
``train``, optional ``keep``, ``gc``; joint: ``model`` (JSON), ``y`` and the
flow's variables as ``fvar:<path>``; traj: ``gcs`` (T, ...), ``keeps`` (T,
rows, F), ``opt`` (JSON: max_norm, learning_rate, weight_decay).  The
network's variables are ``var:<path>``."""

import json
import os
import sys

import numpy as np

JITTER = 2.0**-22


# ---- job files and host helpers (no torch needed) --------------------------------
def _flat(tree, path=()):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _flat(tree[k], path + (k,))
    else:
        yield "/".join(path), np.asarray(tree)


def _unflat(items):
    tree = {}
    for key, val in items:
        node = tree
        parts = key.split("/")
        for k in parts[:-1]:
            node = node.setdefault(k, {})
        node[parts[-1]] = val
    return tree


def ids_of(offsets, rows):
    """set(i) of every row for CSR offsets (as the kernel clamps them): -1 for
    a row in no set."""
    o = np.maximum.accumulate(np.clip(np.asarray(offsets, np.int64), 0, rows))
    ids = np.full(rows, -1, np.int64)
    for s in range(len(o) - 1):
        ids[o[s]:o[s + 1]] = s
    return ids


def sum_matrix(offsets, rows):
    """The notebook's ``sum_matrix`` (``preprocess``), dense: one 1 per
    element row, in the row of its set; padding rows have none."""
    n = np.diff(np.asarray(offsets, np.int64))
    m = np.zeros((len(n), rows), np.int8)
    a = int(offsets[0])
    for j, b in enumerate(a + np.cumsum(n)):
        m[j, a:b] = 1
        a = int(b)
    return m


def pack_job(path, cfg, variables, x, ids, S, mode="net", train=True, **extra):
    job = {"cfg": np.array(json.dumps(cfg)), "mode": np.array(mode), "x": np.asarray(x),
           "ids": np.asarray(ids, np.int64), "S": np.array(int(S)), "train": np.array(bool(train))}
    for k, v in extra.items():
        if v is None:
            continue
        if k == "flow_variables":
            for kk, vv in _flat(v):
                job["fvar:" + kk] = vv
        elif k in ("model", "opt"):
            job[k] = np.array(json.dumps(v))
        else:
            job[k] = np.asarray(v)
    for k, v in _flat(variables):
        job["var:" + k] = v
    np.savez(path, **job)


def load_job(path):
    z = dict(np.load(path))
    job = {k: v for k, v in z.items() if not k.startswith(("var:", "fvar:"))}
    for k in ("cfg", "model", "opt"):
        if k in job:
            job[k] = json.loads(str(job[k]))
    job["mode"], job["S"], job["train"] = str(job["mode"]), int(job["S"]), bool(job["train"])
    job["variables"] = _unflat((k[4:], v) for k, v in z.items() if k.startswith("var:"))
    fv = [(k[5:], v) for k, v in z.items() if k.startswith("fvar:")]
    if fv:
        job["flow_variables"] = _unflat(fv)
    return job


# ---- the restated network ----------------------------------------------------------
def segment_sum(h, ids, S):
    """out[s] = sum of the rows of h whose id is s (torch index_add)."""
    import torch

    sel = ids >= 0
    out = torch.zeros((S, h.shape[1]), dtype=h.dtype)
    return out.index_add(0, torch.as_tensor(ids[sel]), h[torch.as_tensor(sel)])


def keep_prob(rate):
    """(float)1 - rate as the device forms it."""
    return float(np.float32(1.0) - np.float32(rate))


def net_forward(cfg, params, stats, x, ids, S, train, keep):
    """Phi.__call__: (c, new batch_stats or None)."""
    import torch

    from oracle import zf_oracle_torch as OT

    h, new = x, None
    if cfg["batch_norm"]:
        p = params["BatchNorm_0"]
        if train:
            mean = h.mean(dim=0)
            var = torch.clamp((h * h).mean(dim=0) - mean * mean, min=0)
            s = stats["BatchNorm_0"]
            new = {"BatchNorm_0": {"mean": 0.99 * s["mean"] + 0.01 * mean.detach(),
                                   "var": 0.99 * s["var"] + 0.01 * var.detach()}}
        else:
            mean, var = stats["BatchNorm_0"]["mean"], stats["BatchNorm_0"]["var"]
        h = (h - mean) / torch.sqrt(var + 1e-5) * p["scale"] + p["bias"]
    nl = len(cfg["layers"])
    blk = params["NNBlock_0"]
    for l in range(nl):
        h = OT._act(cfg["act"], h @ blk[f"Dense_{l}"]["kernel"] + blk[f"Dense_{l}"]["bias"])
    h = h @ blk[f"Dense_{nl}"]["kernel"] + blk[f"Dense_{nl}"]["bias"]
    if train and cfg["dropout"] > 0:
        h = torch.where(torch.as_tensor(keep), h / keep_prob(cfg["dropout"]), torch.zeros_like(h))
    if cfg["pool"] == "sum":
        h = segment_sum(h, ids, S)
    return h, new


def _tree(tree, dtype, grad, rng=None):
    import torch

    if isinstance(tree, dict):
        return {k: _tree(tree[k], dtype, grad, rng) for k in sorted(tree)}
    a = np.asarray(tree, np.float64)
    if rng is not None:
        a = a * (1 + JITTER * rng.standard_normal(a.shape))
    return torch.tensor(a, dtype=dtype, requires_grad=grad)


def _grads(tree):
    if isinstance(tree, dict):
        return {k: _grads(v) for k, v in tree.items()}
    return np.zeros(tuple(tree.shape)) if tree.grad is None else tree.grad.detach().numpy().astype(np.float64)


def _np(t):
    return t.detach().numpy().astype(np.float64)


def evaluate(job, dtype, perm=None, jitter_rng=None, variables=None, gc=None, keep=None):
    """One evaluation: {"c", "stats" (train, BatchNorm), "g" (with a cotangent
    or a joint loss), "loss" (joint)}; rows permuted by ``perm`` going in and
    back coming out."""
    import torch

    cfg = job["cfg"]
    variables = job["variables"] if variables is None else variables
    x = np.asarray(job["x"], np.float64)
    ids = np.asarray(job["ids"], np.int64)
    keep = job.get("keep") if keep is None else keep
    gc = job.get("gc") if gc is None else gc
    if jitter_rng is not None:
        x = x * (1 + JITTER * jitter_rng.standard_normal(x.shape))
    if perm is not None:
        x, ids = x[perm], ids[perm]
        keep = None if keep is None else np.asarray(keep)[perm]
    pooled = cfg["pool"] == "sum"
    want_grad = gc is not None or job["mode"] == "joint"
    params = _tree(variables["params"], dtype, want_grad, jitter_rng)
    stats = _tree(variables.get("batch_stats", {}), dtype, False)
    c, new = net_forward(cfg, params, stats, torch.tensor(x, dtype=dtype), ids, job["S"], job["train"], keep)
    res = {}
    if job["mode"] == "joint":
        from oracle import zf_oracle_torch as OT
        from tests.input_grad_oracle import flow_lp

        fv = job["flow_variables"]
        fp = _tree(fv["params"]["bijector"], dtype, False, jitter_rng)
        y = np.asarray(job["y"], np.float64)
        if jitter_rng is not None:
            y = y * (1 + JITTER * jitter_rng.standard_normal(y.shape))
        lp = flow_lp(OT, job["model"], fp, fv.get("batch_stats", {}).get("bijector", {}), torch.tensor(y, dtype=dtype),
                     c, train=True)
        loss = -lp.mean()
        loss.backward()
        res["loss"] = float(loss.detach())
    elif gc is not None:
        g = np.asarray(gc, np.float64)
        if perm is not None and not pooled:
            g = g[perm]
        (torch.tensor(g, dtype=dtype) * c).sum().backward()
    cn = _np(c)
    if perm is not None and not pooled:
        cn = cn[np.argsort(perm)]
    res["c"] = cn
    if new is not None:
        res["stats"] = {"BatchNorm_0": {k: _np(v) for k, v in new["BatchNorm_0"].items()}}
    if want_grad:
        res["g"] = _grads(params)
    return res


def _put(out, tag, res):
    for k, v in res.items():
        if isinstance(v, dict):
            for kk, vv in _flat(v):
                out[f"{k}{tag}:{kk}"] = vv
        else:
            out[f"{k}{tag}"] = np.asarray(v, np.float64)


# ---- the optimiser trajectory ---------------------------------------------------------
def trajectory(job):
    """T steps of the chain on the gradients of sum(gc_t * c): float64
    (chain_reference on float64 autograd) and the float32 restatement
    (chain_kernel_f32 on float32 autograd), each free-running from the same
    start.  Returns the final parameter trees."""
    import torch

    from tests.optim_ref import chain_kernel_f32, chain_reference, chain_state
    from zenflow_amd import optim

    o = job["opt"]
    chain = optim.chain(optim.clip_by_global_norm(o["max_norm"]),
                        optim.adamw(o["learning_rate"], weight_decay=o["weight_decay"]))
    leaves = list(_flat(job["variables"]["params"]))
    sizes = [v.size for _, v in leaves]
    mask = np.ones(sum(sizes), bool)

    def flat(tree):
        return np.concatenate([np.asarray(v, np.float64).reshape(-1) for _, v in _flat(tree)])

    def tree_of(vec):
        items, at = [], 0
        for (k, v), n in zip(leaves, sizes):
            items.append((k, np.asarray(vec[at:at + n]).reshape(v.shape)))
            at += n
        return _unflat(items)

    T = job["gcs"].shape[0]
    out = {}
    for name, dtype in (("64", torch.float64), ("32", torch.float32)):
        theta = flat(job["variables"]["params"])
        state = chain_state(chain, mask)
        slots = [np.zeros(theta.size, np.float32) for _ in range(chain.n_slots)]
        if name == "32":
            theta = theta.astype(np.float32)
        stats = job["variables"].get("batch_stats", {})
        for t in range(T):
            v = {"params": tree_of(theta), "batch_stats": stats}
            keep = job["keeps"][t] if "keeps" in job else None
            g = flat(evaluate(job, dtype, variables=v, gc=job["gcs"][t], keep=keep)["g"])
            if name == "64":
                theta, state = chain_reference(theta, g, state, t, chain)
            else:
                theta, slots = chain_kernel_f32(theta, g.astype(np.float32), slots, t, chain, mask)
        out[name] = tree_of(np.asarray(theta, np.float64))
    return out


def main(job_path, out_path):
    import torch

    job = load_job(job_path)
    out = {}
    if job["mode"] == "traj":
        tr = trajectory(job)
        for name, tree in tr.items():
            for k, v in _flat(tree):
                out[f"theta{name}:{k}"] = v
        np.savez(out_path, **out)
        return
    rows = job["x"].shape[0]
    perms = [None, np.random.default_rng(1).permutation(rows), np.random.default_rng(2).permutation(rows)]
    _put(out, "64", evaluate(job, torch.float64))
    for r, p in enumerate(perms):
        _put(out, f"32_{r}", evaluate(job, torch.float32, perm=p))
    for r in range(2):
        _put(out, f"64p_{r}", evaluate(job, torch.float64, jitter_rng=np.random.default_rng(100 + r)))
    np.savez(out_path, **out)


if __name__ == "__main__":
    os.environ["HIP_VISIBLE_DEVICES"] = ""  # this process never touches the GPU (set before torch loads)
    main(sys.argv[1], sys.argv[2])
