"""Oracle of the input gradient and of stacked conditioning networks
(zenflow_amd/nn.py, zf_condnet_backward_input) for tests/test_deepset_host.py
and tests/test_gpu_deepset.py: a torch restatement of the first half of
examples/deep_set.ipynb (``class DeepSet`` / ``loss_fn``),

    x -> Phi (tests/condnet_oracle.py::net_forward) -> c -> rho (an NNBlock,
    net_forward again, per row) -> yp,

differentiated with respect to ``x`` and to both networks' parameters.  Three
modes:

    "net"    one network, ``x.requires_grad``, the value sum(gc * c);
    "stack"  phi -> rho, the value sum(gy * yp) for a given cotangent ``gy``;
    "flow"   phi -> rho -> the flow's train-mode loss -mean(log_prob(y | rho(phi(x))))
             (``tests/input_grad_oracle.py::flow_lp``, composed as
             condnet_oracle's joint mode composes it).

As in condnet_oracle, every job runs in float64, in float32 over three orders
of the element rows (per-row results are un-permuted coming out) and in float64
at inputs and parameters jittered by 2^-22 relative.  Output keys follow the
scheme ``tests/test_gpu_condnet.py::_check`` reads, ``<name><tag>[:<path>]``
with tag 64, 32_k, 64p_k: ``c`` (phi's output), ``y`` (rho's), ``gx`` (d / d
x), ``g:<path>`` (phi's parameters), ``rg:<path>`` (rho's), ``loss`` (flow).

Runs in its own CPU-only process:

    python -m tests.deepset_oracle JOB.npz OUT.npz

JOB.npz (``pack_job``): condnet_oracle's job for phi (``cfg``, ``x``, ``ids``,
``S``, ``keep``, ``var:<path>``; ``gc`` in mode "net"), and for the other modes
``rcfg`` (JSON), ``rvar:<path>``, optional ``rkeep``, ``gy`` (stack) or
``model`` / ``y`` / ``fvar:<path>`` (flow)."""

import json
import os
import sys

import numpy as np

from tests import condnet_oracle as CO

JITTER = CO.JITTER


def pack_job(path, cfg, variables, x, ids, S, mode="net", rcfg=None, rvariables=None, **extra):
    """condnet_oracle.pack_job plus the second network."""
    more = {}
    if rcfg is not None:
        more["rcfg"] = np.array(json.dumps(rcfg))
        for k, v in CO._flat(rvariables):
            more["rvar:" + k] = v
    CO.pack_job(path, cfg, variables, x, ids, S, mode=mode, train=True, **extra, **more)


def load_job(path):
    job = CO.load_job(path)
    rv = [(k[5:], job.pop(k)) for k in [k for k in job if k.startswith("rvar:")]]
    if rv:
        job["rvariables"] = CO._unflat(rv)
    if "rcfg" in job:
        job["rcfg"] = json.loads(str(job["rcfg"]))
    return job


def evaluate(job, dtype, perm=None, jitter_rng=None, x=None, variables=None, rvariables=None):
    """One evaluation in train mode: {"value", "c", "gx", "g"} and, behind a
    second network, {"y", "rg"}; "loss" in mode "flow".  The element rows are
    permuted by ``perm`` going in and back coming out.  ``x``, ``variables``
    and ``rvariables`` override the job's (central differences)."""
    import torch

    cfg, mode = job["cfg"], job["mode"]
    variables = job["variables"] if variables is None else variables
    x = np.asarray(job["x"] if x is None else x, np.float64)
    ids = np.asarray(job["ids"], np.int64)
    keep = job.get("keep")
    if jitter_rng is not None:
        x = x * (1 + JITTER * jitter_rng.standard_normal(x.shape))
    if perm is not None:
        x, ids = x[perm], ids[perm]
        keep = None if keep is None else np.asarray(keep)[perm]
    pooled = cfg["pool"] == "sum"
    rowperm = None if pooled else perm  # the order of c's rows
    back = None if perm is None else np.argsort(perm)

    def rows_in(a):
        a = np.asarray(a, np.float64)
        return a if rowperm is None else a[rowperm]

    def rows_out(a):
        return a if rowperm is None else a[np.argsort(rowperm)]

    params = CO._tree(variables["params"], dtype, True, jitter_rng)
    stats = CO._tree(variables.get("batch_stats", {}), dtype, False)
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    c, _ = CO.net_forward(cfg, params, stats, xt, ids, job["S"], True, keep)
    res = {}
    if mode == "net":
        value = (torch.tensor(rows_in(job["gc"]), dtype=dtype) * c).sum()
    else:
        rcfg = job["rcfg"]
        rvariables = job["rvariables"] if rvariables is None else rvariables
        rparams = CO._tree(rvariables["params"], dtype, True, jitter_rng)
        rstats = CO._tree(rvariables.get("batch_stats", {}), dtype, False)
        n = c.shape[0]
        rkeep = job.get("rkeep")
        if rkeep is not None:
            rkeep = rows_in(rkeep).astype(bool)
        y, _ = CO.net_forward(rcfg, rparams, rstats, c, np.arange(n), n, True, rkeep)
        if mode == "stack":
            value = (torch.tensor(rows_in(job["gy"]), dtype=dtype) * y).sum()
        elif mode == "flow":
            from oracle import zf_oracle_torch as OT
            from tests.input_grad_oracle import flow_lp

            fv = job["flow_variables"]
            fp = CO._tree(fv["params"]["bijector"], dtype, False, jitter_rng)
            yy = np.asarray(job["y"], np.float64)
            if jitter_rng is not None:
                yy = yy * (1 + JITTER * jitter_rng.standard_normal(yy.shape))
            lp = flow_lp(OT, job["model"], fp, fv.get("batch_stats", {}).get("bijector", {}),
                         torch.tensor(rows_in(yy), dtype=dtype), y, train=True)
            value = -lp.mean()
            res["loss"] = float(value.detach())
        else:
            raise ValueError(mode)
        res["y"] = rows_out(CO._np(y))
    value.backward()
    res["value"] = float(value.detach())
    res["c"] = rows_out(CO._np(c))
    gx = np.zeros(x.shape) if xt.grad is None else xt.grad.detach().numpy().astype(np.float64)
    res["gx"] = gx if back is None else gx[back]
    res["g"] = CO._grads(params)
    if mode != "net":
        res["rg"] = CO._grads(rparams)
    return res


def main(job_path, out_path):
    import torch

    job = load_job(job_path)
    rows = job["x"].shape[0]
    perms = [None, np.random.default_rng(1).permutation(rows), np.random.default_rng(2).permutation(rows)]
    out = {}
    CO._put(out, "64", evaluate(job, torch.float64))
    for r, p in enumerate(perms):
        CO._put(out, f"32_{r}", evaluate(job, torch.float32, perm=p))
    for r in range(2):
        CO._put(out, f"64p_{r}", evaluate(job, torch.float64, jitter_rng=np.random.default_rng(100 + r)))
    np.savez(out_path, **out)


if __name__ == "__main__":
    os.environ["HIP_VISIBLE_DEVICES"] = ""  # this process never touches the GPU (set before torch loads)
    main(sys.argv[1], sys.argv[2])
