"""Sample-gradient oracle worker for tests/test_gpu_sample_grad.py: float64
autograd through the flow's inverse pass.

With the reference ``x = flow.apply(vars, c_or_n, method="sample")``
(flow.py:50-78) is a differentiable JAX function.  JAX is not available
offline, so the inverse chain is restated in torch from the reference:

* ``rqs_inverse``: ``rational_quadratic_spline_inverse`` (utils.py:144-202) —
  bins on the yk knots, the quadratic root, no clamp and no epsilons;
* ``nsc_inverse_eval``: ``NeuralSplineCoupling.inverse`` (bijectors.py:367-371),
  BatchNorm on the stored mean / var;
* ``shift_bounds_inverse``: ``ShiftBounds.inverse`` (bijectors.py:210-240) on
  the stored xmin / xmax; ``Roll.inverse``; their chain from the last op to
  the first.

``log_q`` is composed from ``tests.input_grad_oracle``'s pieces of ``flow_lp``
(``nsc_eval``, ``shift_bounds_eval``, ``OT.latent_log_prob``): the latent's
log_prob of z plus every op's forward log-det at the inverse's own
intermediate for that op — what ``flow_lp`` returns on x, up to the forward
spline's epsilons (tests/test_sample_grad_oracle.py ties the two).

Emitted, in the key scheme ``check_params`` / ``check_columns`` read: ``x64``,
``lq64`` / ``lq32_<r>`` / ``lq64p_<r>`` (log_q of every evaluation), ``lp64``
(log_q, NaN on rows whose x or log_q is not finite), the gradients of

    sum_b where(row b finite, gx_b . x_b + glq_b log_q_b, 0)

with respect to every parameter tensor (``g64:<path>``), z (``gz64``) and c
(``gc64``) in float64; in float32 over three row orders (``g32_<r>:``,
``gz32_<r>``, ``gc32_<r>``); in float64 at parameters, z and c jittered by
2^-22 relative (``g64p_<r>:`` ...); the inputs ``z``, ``cgx``, ``cglq`` and
``dropped``, the rows autograd itself loses (finite values, NaN gradient) in
any of those evaluations: they are left out of the sum, and the GPU call
gives them zero cotangents.

Runs in its own CPU-only process (importing torch into the GPU test process
would shadow the system librccl there).

    python -m tests.sample_grad_oracle NAME N SEED glq|noglq OUT.npz"""

import os
import sys

import numpy as np

from tests.input_grad_oracle import JITTER, _jitter_tree
from tests.weighted_grad_oracle import _flat


# ---- inputs (no torch needed) ---------------------------------------------------
def draw_latent(latent, N, D, seed):
    """z ~ the case's latent (distributions.py), float32."""
    rng = np.random.default_rng(3000 + seed)
    t = latent["type"]
    if t == "normal":
        z = 0.5 + 0.1 * rng.standard_normal((N, D))
    elif t == "truncated_normal":
        z = 0.5 + 0.1 * np.clip(rng.standard_normal((N, D)), -4.9, 4.9)
    elif t == "beta":
        a = float(latent.get("peakness", 12.0))
        z = rng.beta(a, a, (N, D))
    elif t == "uniform":
        z = rng.uniform(size=(N, D))
    else:
        raise ValueError(t)
    return z.astype(np.float32)


def make_inputs(case, N, seed, with_glq=True):
    """(z, gx, glq or None) of one case: z from its latent, standard-normal cotangents."""
    D = case["cfg"]["D"]
    z = draw_latent(case["model"]["latent"], N, D, seed)
    rng = np.random.default_rng(4000 + seed)
    gx = rng.standard_normal((N, D)).astype(np.float32)
    glq = rng.standard_normal(N).astype(np.float32)
    return z, gx, (glq if with_glq else None)


# ---- the restated inverse --------------------------------------------------------
def rqs_inverse(OT, y, dx, dy, sl):
    """utils.py:144-202."""
    import torch

    xk, yk = OT._knots(dx), OT._knots(dy)
    one = torch.ones_like(sl[..., :1])
    dk = torch.cat([one, sl, one], dim=-1)
    sk = dy / dx
    oob = (y < 0) | (y >= 1)
    idx = torch.sum((yk <= y[..., None]).to(torch.int64), dim=-1, keepdim=True) - 1
    idx = torch.clamp(idx, 0, yk.shape[-1] - 1)
    xk_i, yk_i, dx_i, dy_i = OT._take(xk, idx), OT._take(yk, idx), OT._take(dx, idx), OT._take(dy, idx)
    d_i, d_i1, s_i = OT._take(dk, idx), OT._take(dk, idx + 1), OT._take(sk, idx)
    a = dy_i * (s_i - d_i) + (y - yk_i) * (d_i1 + d_i - 2 * s_i)
    b = dy_i * d_i - (y - yk_i) * (d_i1 + d_i - 2 * s_i)
    c = -s_i * (y - yk_i)
    z = 2 * c / (-b - torch.sqrt(b**2 - 4 * a * c))
    x = z * dx_i + xk_i
    return torch.where(oob, y, x)


def nsc_inverse_eval(OT, spec, p, st, y, c):
    """bijectors.py:367-371: _spline_params(y, c, False), then the inverse spline."""
    import torch

    K = spec.get("knots", 16)
    dt_ = y.shape[1] // 2
    yt, yc = y[:, :dt_], y[:, dt_:]
    u = torch.cat([yc, c], dim=1) if c is not None else yc
    bn = st["BatchNorm_0"]
    mean = torch.tensor(np.asarray(bn["mean"], np.float64), dtype=y.dtype)
    var = torch.tensor(np.asarray(bn["var"], np.float64), dtype=y.dtype)
    mul = 1 / torch.sqrt(var + 1e-5) * p["BatchNorm_0"]["scale"]
    u = (u - mean) * mul + p["BatchNorm_0"]["bias"]
    nl = len(spec.get("layers", (128, 128)))
    for li in range(nl):
        d = p[f"Dense_{li}"]
        u = OT._act(spec.get("act", "swish"), u @ d["kernel"] + d["bias"])
    d = p[f"Dense_{nl}"]
    q = (u @ d["kernel"] + d["bias"]).reshape(y.shape[0], dt_, 3 * K - 1)
    dx = OT._softmax_with_threshold(q[..., :K], OT.EPS)
    dy = OT._softmax_with_threshold(q[..., K : 2 * K], OT.EPS)
    sl = OT._squareplus(q[..., 2 * K :])
    return torch.cat([rqs_inverse(OT, yt, dx, dy, sl), yc], dim=1)


def shift_bounds_inverse(spec, st, z):
    """bijectors.py:210-240."""
    import torch

    from tests.input_grad_oracle import _isset

    bounds = {int(i): (a, b) for (i, a, b) in spec.get("bounds", ())}
    cols = []
    for i in range(z.shape[1]):
        zi = z[:, i]
        a, b = bounds.get(i, (None, None))
        if _isset(a) and _isset(b):
            xi = zi * float(b) + (1 - zi) * float(a)
        else:
            xmin = torch.tensor(float(np.asarray(st[f"xmin_{i}"], np.float64).reshape(-1)[0]), dtype=z.dtype)
            xmax = torch.tensor(float(np.asarray(st[f"xmax_{i}"], np.float64).reshape(-1)[0]), dtype=z.dtype)
            ti = zi * xmax + (1 - zi) * xmin
            if _isset(a):
                xi = torch.exp(ti) + float(a)
            elif _isset(b):
                xi = float(b) - torch.exp(ti)
            else:
                xi = ti
        cols.append(xi)
    return torch.stack(cols, dim=1)


def flow_sample(OT, model, params, stats, z, c):
    """(x, log_q): the chain's inverse from the last op to the first, and the
    latent's log_prob of z plus every op's forward log-det at the inverse's
    own intermediate (the pieces of ``tests.input_grad_oracle.flow_lp``)."""
    import torch

    from tests import input_grad_oracle as IG

    ops = model["bijector"]["bijectors"]
    h = z
    ld = torch.zeros(z.shape[0], dtype=z.dtype)
    for i in range(len(ops) - 1, -1, -1):
        b, key = ops[i], f"bijectors_{i}"
        if b["type"] == "shift_bounds":
            h = shift_bounds_inverse(b, stats.get(key, {}), h)
            ld = ld + IG.shift_bounds_eval(OT, b, stats.get(key, {}), h)[1]
        elif b["type"] == "roll":
            h = torch.roll(h, -b.get("shift", 1), dims=-1)
        elif b["type"] == "nsc":
            h = nsc_inverse_eval(OT, b, params[key], stats[key], h, c)
            ld = ld + IG.nsc_eval(OT, b, params[key], stats[key], h, c)[1]
        else:
            raise ValueError(b["type"])
    return h, OT.latent_log_prob(model["latent"], z) + ld


def sample_grads(model, variables, z, c, gx, glq, dtype, keep=None):
    """x, log_q and the gradients of sum_b where(ok_b, gx_b . x_b + glq_b log_q_b, 0)
    over the rows ``keep`` (default all): (x, lq, ok, d / d params, gz, gc)."""
    import torch

    from oracle import zf_oracle_torch as OT

    N = np.asarray(z).shape[0]
    rows = np.arange(N) if keep is None else np.flatnonzero(keep)
    params = OT._tree(variables["params"]["bijector"], dtype, True)
    stats = variables.get("batch_stats", {}).get("bijector", {})
    zt = torch.tensor(np.asarray(z, np.float64)[rows], dtype=dtype, requires_grad=True)
    ct = None
    if c is not None:
        c = np.asarray(c, np.float64)
        ct = torch.tensor((c.reshape(-1, 1) if c.ndim == 1 else c)[rows], dtype=dtype, requires_grad=True)
    x, lq = flow_sample(OT, model, params, stats, zt, ct)
    ok = torch.isfinite(lq) & torch.isfinite(x).all(dim=1)
    gxt = torch.tensor(np.asarray(gx, np.float64)[rows], dtype=dtype)
    term = (gxt * torch.where(ok[:, None], x, torch.zeros_like(x))).sum(dim=1)
    if glq is not None:
        term = term + torch.tensor(np.asarray(glq, np.float64)[rows], dtype=dtype) * torch.where(ok, lq, torch.zeros_like(lq))
    term.sum().backward()

    def full(t, width=None, fill=0.0):
        out = np.full((N,) if width is None else (N, width), fill, np.float64)
        out[rows] = t.detach().numpy().astype(np.float64)
        return out

    D = zt.shape[1]
    okf = np.zeros(N, bool)
    okf[rows] = ok.numpy()
    return (full(x, D, np.nan), full(lq, None, np.nan), okf, {"bijector": OT._grads(params)}, full(zt.grad, D),
            None if ct is None else full(ct.grad, ct.shape[1]))


def main(name, N, seed, mode, out):
    import torch

    from tests.flowcases import make_case

    case = make_case(name, N=N, seed=seed)
    model, variables, c = case["model"], case["variables"], case["c"]
    z, gx, glq = make_inputs(case, N, seed, mode == "glq")
    z64 = z.astype(np.float64)
    ident = np.arange(N)
    evals = [("64", variables, z64, c, ident, torch.float64)]
    for r in range(3):
        evals.append((f"32_{r}", variables, z64, c, np.random.default_rng(r).permutation(N) if r else ident, torch.float32))
    for r in range(2):
        rng = np.random.default_rng(100 + r)
        v = dict(variables, params={"bijector": _jitter_tree(variables["params"]["bijector"], rng)})
        zp = z64 * (1 + JITTER * rng.standard_normal(z.shape))
        cp = None if c is None else np.asarray(c, np.float64) * (1 + JITTER * rng.standard_normal(np.shape(c)))
        evals.append((f"64p_{r}", v, zp, cp, ident, torch.float64))

    def run(e, keep):
        tag, v, ze, ce, p, dtype = e
        x, lq, ok, g, gz, gc = sample_grads(model, v, ze[p], None if ce is None else np.asarray(ce)[p], gx[p],
                                            None if glq is None else glq[p], dtype, None if keep is None else keep[p])
        inv = np.argsort(p)
        return x[inv], lq[inv], ok[inv], g, gz[inv], None if gc is None else gc[inv]

    res = {"z": z, "cgx": gx}
    if glq is not None:
        res["cglq"] = glq
    # the rows autograd loses: finite x and log_q, NaN gradient, in any evaluation
    dropped = np.zeros(N, bool)
    for e in evals:
        x, lq, ok, _, gz, gc = run(e, None)
        nan = ~np.isfinite(gz).all(axis=1)
        if gc is not None:
            nan |= ~np.isfinite(gc).all(axis=1)
        dropped |= nan & ok
        res["lq" + e[0]] = lq
        if e[0] == "64":
            res["x64"] = x
            res["lp64"] = np.where(ok, lq, np.nan)  # check_columns' rows that must be zero on the GPU
    assert dropped.mean() <= 0.02, f"{name}/{N}: {dropped.sum()} of {N} rows lost"
    res["dropped"] = dropped
    for e in evals:
        tag = e[0]
        _, _, _, g, gz, gc = run(e, ~dropped)
        for k, val in _flat(g):
            res[f"g{tag}:" + k] = val
        res["gz" + tag] = gz
        if gc is not None:
            res["gc" + tag] = gc
    np.savez(out, **res)


if __name__ == "__main__":
    os.environ["HIP_VISIBLE_DEVICES"] = ""  # this process never touches the GPU (set before torch loads)
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5])
