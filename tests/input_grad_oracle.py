"""Input-gradient oracle worker for tests/test_gpu_input_grad.py: float64
autograd of the flow's log_prob with respect to its inputs x and c, the same
in float32 over three row orders, and in float64 at inputs and parameters
jittered by 2^-22 relative (the gradient's conditioning), into an .npz.

The reference's Flow (src/zenflow/flow.py:22-48) is a differentiable JAX
function; examples/deep_set.ipynb's ``DeepSetFlow`` / ``loss_fn_2`` cells
differentiate it with respect to the condition c = phi(x).  JAX is not
available offline, so the arithmetic is restated from
oracle/zf_oracle_torch.py's pieces (``rqs_forward``,
``_softmax_with_threshold``, ``_squareplus``, ``_act``, ``latent_log_prob``,
``_safe_log``):

* eval mode: BatchNorm on the stored mean / var, ShiftBounds on the stored
  xmin / xmax with the clamp (bijectors.py:258-273), nan_to_num's gradient
  as a row mask (flow.py:47);
* train mode (train.py:64-72): ``OT.shift_bounds`` and ``OT.nsc`` composed as
  ``OT.train_loss_and_grad`` composes them, with c (and optionally phi's
  weights, c = tanh(xin @ kernel + bias)) carrying ``requires_grad``.

tests/test_input_grad_oracle.py pins the eval restatement's float64 log_prob
against the NumPy oracle.  Runs in its own CPU-only process (importing torch
into the GPU test process would shadow the system librccl there).

    python -m tests.input_grad_oracle JOB.npz OUT.npz

JOB.npz: ``model`` (JSON), ``mode`` ("eval" | "train"), ``x``, optional ``c``,
``cot`` (eval), ``rows`` (eval: the row subset to differentiate), ``xin`` /
``phi_kernel`` / ``phi_bias`` (train: c = phi(xin)), and the variables
flattened as ``var:<path>`` (tests.input_grad_oracle.pack_job writes it)."""

import json
import math
import os
import sys

import numpy as np

JITTER = 2.0**-22


# ---- job files (no torch needed) ----------------------------------------------
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


def pack_job(path, model, variables, x, c=None, mode="eval", **extra):
    job = {"model": np.array(json.dumps(model)), "mode": np.array(mode), "x": np.asarray(x)}
    if c is not None:
        job["c"] = np.asarray(c)
    for k, v in extra.items():
        if v is not None:
            job[k] = np.asarray(v)
    for k, v in _flat(variables):
        job["var:" + k] = v
    np.savez(path, **job)


def load_job(path):
    z = dict(np.load(path))
    job = {k: v for k, v in z.items() if not k.startswith("var:")}
    job["model"] = json.loads(str(job["model"]))
    job["mode"] = str(job["mode"])
    job["variables"] = _unflat((k[4:], v) for k, v in z.items() if k.startswith("var:"))
    return job


# ---- the restated flow ----------------------------------------------------------
def _isset(v):
    return v is not None and np.isfinite(v)  # bijectors.py:426-427


def shift_bounds_eval(OT, spec, st, x):
    """bijectors.py:163-208 with train=False: stored xmin / xmax, clamp."""
    import torch

    bounds = {int(i): (a, b) for (i, a, b) in spec.get("bounds", ())}
    cols, ld = [], torch.zeros(x.shape[0], dtype=x.dtype)
    for i in range(x.shape[1]):
        xi = x[:, i]
        a, b = bounds.get(i, (None, None))
        if _isset(a) and _isset(b):
            mul = 1.0 / (float(b) - float(a))
            zi, li = (xi - float(a)) * mul, torch.full_like(xi, math.log(mul))
        else:
            ti = xi
            if _isset(a):
                ti = OT._safe_log(xi - float(a))
            elif _isset(b):
                ti = OT._safe_log(float(b) - xi)
            xmin = torch.tensor(float(np.asarray(st[f"xmin_{i}"], np.float64).reshape(-1)[0]), dtype=x.dtype)
            xmax = torch.tensor(float(np.asarray(st[f"xmax_{i}"], np.float64).reshape(-1)[0]), dtype=x.dtype)
            mul = 1 / (xmax - xmin)
            zi, li = torch.clamp((ti - xmin) * mul, 0, 1), torch.log(mul)
            if ti is not xi:
                li = li - ti
        cols.append(zi)
        ld = ld + li
    return torch.stack(cols, dim=1), ld


def nsc_eval(OT, spec, p, st, x, c):
    """bijectors.py:329-365 with train=False: BatchNorm on the stored statistics."""
    import torch

    K = spec.get("knots", 16)
    dt_ = x.shape[1] // 2
    xt, xc = x[:, :dt_], x[:, dt_:]
    u = torch.cat([xc, c], dim=1) if c is not None else xc
    bn = st["BatchNorm_0"]
    mean = torch.tensor(np.asarray(bn["mean"], np.float64), dtype=x.dtype)
    var = torch.tensor(np.asarray(bn["var"], np.float64), dtype=x.dtype)
    mul = 1 / torch.sqrt(var + 1e-5) * p["BatchNorm_0"]["scale"]
    u = (u - mean) * mul + p["BatchNorm_0"]["bias"]
    nl = len(spec.get("layers", (128, 128)))
    for li in range(nl):
        d = p[f"Dense_{li}"]
        u = OT._act(spec.get("act", "swish"), u @ d["kernel"] + d["bias"])
    d = p[f"Dense_{nl}"]
    q = (u @ d["kernel"] + d["bias"]).reshape(x.shape[0], dt_, 3 * K - 1)
    dx = OT._softmax_with_threshold(q[..., :K], OT.EPS)
    dy = OT._softmax_with_threshold(q[..., K : 2 * K], OT.EPS)
    sl = OT._squareplus(q[..., 2 * K :])
    yt, ld = OT.rqs_forward(xt, dx, dy, sl)
    return torch.cat([yt, xc], dim=1), ld


def flow_lp(OT, model, params, stats, x, c, train):
    """Flow.__call__ (flow.py:22-48) before nan_to_num."""
    import torch

    ld = torch.zeros(x.shape[0], dtype=x.dtype)
    h = x
    for i, b in enumerate(model["bijector"]["bijectors"]):
        key = f"bijectors_{i}"
        if b["type"] == "shift_bounds":
            h, l = OT.shift_bounds(b, stats.get(key, {}), h) if train else shift_bounds_eval(OT, b, stats.get(key, {}), h)
        elif b["type"] == "roll":
            h, l = torch.roll(h, b.get("shift", 1), dims=-1), None
        elif b["type"] == "nsc":
            h, l = OT.nsc(b, params[key], h, c) if train else nsc_eval(OT, b, params[key], stats[key], h, c)
        else:
            raise ValueError(b["type"])
        if l is not None:
            ld = ld + l
    return OT.latent_log_prob(model["latent"], h) + ld


def _np(t):
    return None if t is None else t.detach().numpy().astype(np.float64)


def eval_grads(job, dtype, perm=None, jitter_rng=None):
    """(lp_raw, gx, gc) of sum(cot * nan_to_num(lp)) over the job's rows."""
    import torch

    from oracle import zf_oracle_torch as OT

    x = np.asarray(job["x"], np.float64)
    c = None if "c" not in job else np.asarray(job["c"], np.float64)
    cot = np.ones(x.shape[0]) if "cot" not in job else np.asarray(job["cot"], np.float64).reshape(-1)
    if "rows" in job:
        r = np.asarray(job["rows"], np.int64)
        x, c, cot = x[r], None if c is None else c[r], cot[r]
    variables = job["variables"]
    pv = variables["params"]["bijector"]
    if jitter_rng is not None:
        pv = _jitter_tree(pv, jitter_rng)
        x = x * (1 + JITTER * jitter_rng.standard_normal(x.shape))
        if c is not None:
            c = c * (1 + JITTER * jitter_rng.standard_normal(c.shape))
    if perm is not None:
        x, c, cot = x[perm], None if c is None else c[perm], cot[perm]
    params = OT._tree(pv, dtype, False)
    stats = variables.get("batch_stats", {}).get("bijector", {})
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    ct = None if c is None else torch.tensor(c, dtype=dtype, requires_grad=True)
    lp = flow_lp(OT, job["model"], params, stats, xt, ct, train=False)
    fin = torch.isfinite(lp)
    # flow.py:47: nan_to_num passes the cotangent where lp is finite only
    total = (torch.tensor(cot, dtype=dtype) * torch.where(fin, lp, torch.zeros_like(lp))).sum()
    total.backward()
    gx = _np(xt.grad)
    gc = None if ct is None else _np(ct.grad)
    lpn = _np(lp)
    if perm is not None:
        inv = np.argsort(perm)
        gx, gc, lpn = gx[inv], None if gc is None else gc[inv], lpn[inv]
    return lpn, gx, gc


def _jitter_tree(tree, rng):
    if isinstance(tree, dict):
        return {k: _jitter_tree(tree[k], rng) for k in sorted(tree)}
    a = np.asarray(tree, np.float64)
    return a * (1 + JITTER * rng.standard_normal(a.shape))


def train_grads(job, dtype, perm=None, jitter_rng=None):
    """(loss, gc, gk, gb): d loss / d c of the train-mode loss (train.py:64-72),
    and with phi (c = tanh(xin @ kernel + bias)) d loss / d its weights."""
    import torch

    from oracle import zf_oracle_torch as OT

    x = np.asarray(job["x"], np.float64)
    phi = "phi_kernel" in job
    c = None if phi else np.asarray(job["c"], np.float64)
    xin = np.asarray(job["xin"], np.float64) if phi else None
    kern = np.asarray(job["phi_kernel"], np.float64) if phi else None
    bias = np.asarray(job["phi_bias"], np.float64) if phi else None
    variables = job["variables"]
    pv = variables["params"]["bijector"]
    if jitter_rng is not None:
        pv = _jitter_tree(pv, jitter_rng)
        x = x * (1 + JITTER * jitter_rng.standard_normal(x.shape))
        if phi:
            xin = xin * (1 + JITTER * jitter_rng.standard_normal(xin.shape))
            kern = kern * (1 + JITTER * jitter_rng.standard_normal(kern.shape))
        else:
            c = c * (1 + JITTER * jitter_rng.standard_normal(c.shape))
    if perm is not None:
        x = x[perm]
        c = None if c is None else c[perm]
        xin = None if xin is None else xin[perm]
    params = OT._tree(pv, dtype, False)
    stats = variables.get("batch_stats", {}).get("bijector", {})
    xt = torch.tensor(x, dtype=dtype)
    kt = bt = None
    if phi:
        kt = torch.tensor(kern, dtype=dtype, requires_grad=True)
        bt = torch.tensor(bias, dtype=dtype, requires_grad=True)
        ct = torch.tanh(torch.tensor(xin, dtype=dtype) @ kt + bt)
        ct.retain_grad()
    else:
        ct = torch.tensor(c, dtype=dtype, requires_grad=True)
    lp = flow_lp(OT, job["model"], params, stats, xt, ct, train=True)
    loss = -lp.mean()
    loss.backward()
    gc = _np(ct.grad)
    if perm is not None:
        gc = gc[np.argsort(perm)]
    return float(loss.detach()), gc, _np(None if kt is None else kt.grad), _np(None if bt is None else bt.grad)


def main(job_path, out):
    import torch

    job = load_job(job_path)
    N = job["x"].shape[0] if "rows" not in job else len(job["rows"])
    perms = [None, np.random.default_rng(1).permutation(N), np.random.default_rng(2).permutation(N)]
    res = {}

    def put(tag, names, vals):
        for n, v in zip(names, vals):
            if v is not None:
                res[f"{n}{tag}"] = np.asarray(v, np.float64)

    if job["mode"] == "eval":
        names = ("lp", "gx", "gc")
        put("64", names, eval_grads(job, torch.float64))
        for r, p in enumerate(perms):
            put(f"32_{r}", names, eval_grads(job, torch.float32, perm=p))
        for r in range(2):
            put(f"64p_{r}", names, eval_grads(job, torch.float64, jitter_rng=np.random.default_rng(100 + r)))
    else:
        names = ("loss", "gc", "gk", "gb")
        put("64", names, train_grads(job, torch.float64))
        for r, p in enumerate(perms):
            put(f"32_{r}", names, train_grads(job, torch.float32, perm=p))
        for r in range(2):
            put(f"64p_{r}", names, train_grads(job, torch.float64, jitter_rng=np.random.default_rng(100 + r)))
    np.savez(out, **res)


if __name__ == "__main__":
    os.environ["HIP_VISIBLE_DEVICES"] = ""  # this process never touches the GPU (set before torch loads)
    main(sys.argv[1], sys.argv[2])
