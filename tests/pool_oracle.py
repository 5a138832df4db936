"""Oracle of the max pooling and of the mean over sets (zenflow_amd/nn.py,
``ConditionNet(pool="max")``, zf_segment_pool) for tests/test_pool_host.py and
tests/test_gpu_pool.py: tests/condnet_oracle.py's torch restatement of
``Phi`` up to and including dropout, then

    max   scatter_reduce(..., "amax", include_self=False) on zeros,
    mean  index_add over the row ids, divided by the set's number of rows,

which gives zero rows for empty sets, passes a NaN on and, in autograd, splits
the max's gradient evenly among ties (the convention of ``jnp.max``).  The
helpers, the job files, the three float32 row orders and the 2^-22 jitter are
condnet_oracle's; its ``evaluate`` tests ``cfg["pool"] == "sum"``, so the
evaluation is restated here, with the input gradient ``gx`` added.

For the max the float64 run also reports, over every (set, column), the
smallest gap between the largest and the second-largest DISTINCT value of d
(``gap``) and max|d| (``dmax``): where that gap is far above fp32 rounding no
float32 evaluation can pick another row as the maximum.

Runs in its own CPU-only process:

    python -m tests.pool_oracle JOB.npz OUT.npz

JOB.npz is ``condnet_oracle.pack_job``'s, modes "net" | "joint"."""

import os
import sys

import numpy as np

from tests import condnet_oracle as CO


def pool(d, ids, S, how):
    """The set reduction of the rows of d (torch) with ids >= 0."""
    import torch

    if how == "sum":
        return CO.segment_sum(d, ids, S)
    sel = ids >= 0
    idx, rows = torch.as_tensor(ids[sel]), d[torch.as_tensor(sel)]
    zeros = torch.zeros((S, d.shape[1]), dtype=d.dtype)
    if how == "mean":
        n = np.bincount(ids[sel], minlength=S)
        return zeros.index_add(0, idx, rows) / torch.as_tensor(np.maximum(n, 1), dtype=d.dtype)[:, None]
    if how == "max":
        return zeros.scatter_reduce(0, idx[:, None].expand(-1, d.shape[1]), rows, "amax", include_self=False)
    raise ValueError(how)


def net_forward(cfg, params, stats, x, ids, S, train, keep):
    """Phi.__call__ with the pooling of cfg: (c, new batch_stats or None, d)."""
    d, new = CO.net_forward({**cfg, "pool": None}, params, stats, x, ids, S, train, keep)
    return (d if cfg["pool"] is None else pool(d, ids, S, cfg["pool"])), new, d


def max_gap(d, ids, S):
    """(the smallest top-two gap between distinct values over the (set, column)s, max|d| over the rows in sets)."""
    gap, dmax = np.inf, 0.0
    for s in range(S):
        rows = d[ids == s]
        if not len(rows):
            continue
        dmax = max(dmax, float(np.abs(rows).max()))
        for f in range(rows.shape[1]):
            u = np.unique(rows[:, f])
            if len(u) > 1:
                gap = min(gap, float(u[-1] - u[-2]))
    return gap, dmax


def evaluate(job, dtype, perm=None, jitter_rng=None, variables=None, gc=None, keep=None):
    """condnet_oracle.evaluate for any pooling: {"c", "stats", "g", "gx",
    "loss"}, and for the max {"gap", "dmax"}."""
    import torch

    cfg = job["cfg"]
    variables = job["variables"] if variables is None else variables
    x = np.asarray(job["x"], np.float64)
    ids = np.asarray(job["ids"], np.int64)
    keep = job.get("keep") if keep is None else keep
    gc = job.get("gc") if gc is None else gc
    if jitter_rng is not None:
        x = x * (1 + CO.JITTER * jitter_rng.standard_normal(x.shape))
    if perm is not None:
        x, ids = x[perm], ids[perm]
        keep = None if keep is None else np.asarray(keep)[perm]
    pooled = cfg["pool"] is not None
    want_grad = gc is not None or job["mode"] == "joint"
    params = CO._tree(variables["params"], dtype, want_grad, jitter_rng)
    stats = CO._tree(variables.get("batch_stats", {}), dtype, False)
    xt = torch.tensor(x, dtype=dtype, requires_grad=want_grad)
    c, new, d = net_forward(cfg, params, stats, xt, ids, job["S"], job["train"], keep)
    res = {}
    if job["mode"] == "joint":
        from oracle import zf_oracle_torch as OT
        from tests.input_grad_oracle import flow_lp

        fv = job["flow_variables"]
        fp = CO._tree(fv["params"]["bijector"], dtype, False, jitter_rng)
        y = np.asarray(job["y"], np.float64)
        if jitter_rng is not None:
            y = y * (1 + CO.JITTER * jitter_rng.standard_normal(y.shape))
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
    cn = CO._np(c)
    back = None if perm is None else np.argsort(perm)
    if back is not None and not pooled:
        cn = cn[back]
    res["c"] = cn
    if new is not None:
        res["stats"] = {"BatchNorm_0": {k: CO._np(v) for k, v in new["BatchNorm_0"].items()}}
    if want_grad:
        res["g"] = CO._grads(params)
        gx = np.zeros(x.shape) if xt.grad is None else xt.grad.detach().numpy().astype(np.float64)
        res["gx"] = gx if back is None else gx[back]
    if cfg["pool"] == "max":
        res["gap"], res["dmax"] = max_gap(CO._np(d), ids, job["S"])
    return res


def main(job_path, out_path):
    import torch

    job = CO.load_job(job_path)
    out = {}
    rows = job["x"].shape[0]
    perms = [None, np.random.default_rng(1).permutation(rows), np.random.default_rng(2).permutation(rows)]
    CO._put(out, "64", evaluate(job, torch.float64))
    for r, p in enumerate(perms):
        CO._put(out, f"32_{r}", evaluate(job, torch.float32, perm=p))
    for r in range(2):
        CO._put(out, f"64p_{r}", evaluate(job, torch.float64, jitter_rng=np.random.default_rng(100 + r)))
    np.savez(out_path, **out)


if __name__ == "__main__":
    os.environ["HIP_VISIBLE_DEVICES"] = ""  # this process never touches the GPU (set before torch loads)
    main(sys.argv[1], sys.argv[2])
