"""Host reference of the trainer over many optimiser steps, in float64 NumPy
(tests/test_train_ref_host.py, tests/test_gpu_train_trajectory.py).

The optimiser is optax's published (n)adamw, restated as in
zenflow_amd/train.py's docstring: scale_by_adam(b1, b2, eps, nesterov) ->
add_decayed_weights(wd) -> scale(-lr).  With g_t the gradient at theta_t and
t = 1, 2, ... the step number,

    m_t = b1 m_{t-1} + (1 - b1) g_t          v_t = b2 v_{t-1} + (1 - b2) g_t^2
    mhat = m_t / (1 - b1^t)                                          (adamw)
    mhat = b1 m_t / (1 - b1^(t+1)) + (1 - b1) g_t / (1 - b1^t)       (nadamw)
    vhat = v_t / (1 - b2^t)
    theta_{t+1} = theta_t - lr (mhat / (sqrt(vhat) + eps) + wd theta_t)

on the entries a mask selects (the parameters of a blob that also holds the
batch statistics).

``adam_tolerance`` bounds what an fp32 evaluation of that update
(adam_kernel in zf_train_kernels.h) may differ by, per element:

    2^-23 |theta_ref| + lr (t + 8) 2^-23 (Ahat / (sqrt(vhat) + eps) + wd |theta_t|)

A_t = b1 A_{t-1} + (1 - b1) |g_t| is the absolute-value twin of m_t and Ahat
the mhat formula with m -> A, g -> |g|: the t accumulations of m and v each
round once per step relative to their absolute sums (m itself may cancel to
nothing), the update is a handful of operations more (the 8), and the final
store rounds theta (the first term).

Run as a module it is the CPU-only free-running reference:

    python -m tests.train_ref NAME N SEED NESTEROV OUT.npz

T optimiser steps of the reference trainer on tests/flowcases case NAME from
ShiftBounds statistics reset to +inf / -inf, over ``trajectory_batches``, in
float64 and in float32 over three row orders of every batch: the gradient by
autograd of the restated loss (oracle/zf_oracle_torch.py), the running
statistics by the NumPy oracle's train-mode pass (oracle/zf_oracle.py), the
update as above.  The .npz holds the per-step losses (``L64``, ``L32_r``) and
the final parameters per leaf (``p64:path``, ``p32_r:path``).  Its own
process, as tests/grad_oracle.py: torch is never imported into a GPU test."""

from __future__ import annotations

import os
import sys
from dataclasses import dataclass

import numpy as np

U23 = 2.0**-23

# the trajectory tests' settings: every bias correction (b1^12 = 0.07, b2^12 =
# 0.54) and the decay (lr wd |theta| ~ 3e-5 |theta|) far above the tolerance
TRAJ_STEPS = 12
TRAJ_ROWS = 256  # rows of the case the batches are cut from
TRAJ_BATCH = 128  # batches alternate between TRAJ_BATCH and TRAJ_BATCH - 29 rows


@dataclass
class Opt:
    """Hyper-parameters (the attribute names of zenflow_amd.train.Optimizer)."""

    learning_rate: float = 3e-3
    b1: float = 0.8
    b2: float = 0.95
    eps: float = 1e-8
    weight_decay: float = 1e-2
    nesterov: bool = True


def trajectory_batches(N=TRAJ_ROWS, T=TRAJ_STEPS, B=TRAJ_BATCH):
    """Row ranges (lo, hi) of the T batches: B rows on even steps, B - 29 on
    odd ones, each from another offset of the N-row case."""
    out = []
    for t in range(T):
        rows = B if t % 2 == 0 else B - 29
        lo = (17 * t) % (N - B + 1)
        out.append((lo, lo + rows))
    return out


def reset_shift_bounds(variables):
    """A copy of ``variables`` whose ShiftBounds running xmin / xmax are the
    +inf / -inf that Flow.init starts from (the other leaves are shared)."""
    stats = dict(variables["batch_stats"]["bijector"])
    sb = {}
    for k, v in stats.get("bijectors_0", {}).items():
        if k.startswith("xmin_"):
            sb[k] = np.full(np.shape(v), np.inf, np.float32)
        elif k.startswith("xmax_"):
            sb[k] = np.full(np.shape(v), -np.inf, np.float32)
        else:
            sb[k] = v
    stats["bijectors_0"] = sb
    return {"params": variables["params"], "batch_stats": {"bijector": stats}}


# ---- the update ---------------------------------------------------------------
def adam_state(mask):
    """Zero moments over a flat blob; ``mask`` selects the parameter entries."""
    mask = np.asarray(mask).astype(bool)
    z = np.zeros(mask.shape, np.float64)
    return {"m": z, "v": z.copy(), "A": z.copy(), "mask": mask}


def _hats(m, v, g, t, opt):
    b1, b2 = float(opt.b1), float(opt.b2)
    if opt.nesterov:
        mhat = b1 * m / (1 - b1 ** (t + 1)) + (1 - b1) * g / (1 - b1**t)
    else:
        mhat = m / (1 - b1**t)
    return mhat, v / (1 - b2**t)


def adam_reference(theta, g, state, t, opt):
    """Step ``t`` (1-based) from ``theta`` with gradient ``g``: ``(theta_next,
    new state)`` in float64; entries outside the state's mask keep their value
    and their (zero) moments."""
    theta = np.asarray(theta, np.float64)
    g = np.where(state["mask"], np.asarray(g, np.float64), 0.0)
    b1, b2 = float(opt.b1), float(opt.b2)
    m = b1 * state["m"] + (1 - b1) * g
    v = b2 * state["v"] + (1 - b2) * g * g
    A = b1 * state["A"] + (1 - b1) * np.abs(g)
    mhat, vhat = _hats(m, v, g, t, opt)
    upd = mhat / (np.sqrt(vhat) + float(opt.eps)) + float(opt.weight_decay) * theta
    nxt = np.where(state["mask"], theta - float(opt.learning_rate) * upd, theta)
    return nxt, {"m": m, "v": v, "A": A, "mask": state["mask"]}


def adam_tolerance(theta_ref, theta, g, state, t, opt):
    """The module docstring's bound per element; ``state`` is the one
    ``adam_reference`` returned with ``theta_ref`` (moments after step t)."""
    g = np.where(state["mask"], np.abs(np.asarray(g, np.float64)), 0.0)
    ahat, vhat = _hats(state["A"], state["v"], g, t, opt)
    span = ahat / (np.sqrt(vhat) + float(opt.eps)) + float(opt.weight_decay) * np.abs(np.asarray(theta, np.float64))
    return U23 * np.abs(theta_ref) + float(opt.learning_rate) * (t + 8) * U23 * span


FAULTS = ("nesterov_b1t", "count_by_2", "m_not_carried", "decay_on_stepped")


def adam_kernel_f32(theta, g, m, v, t, opt, fault=None):
    """adam_kernel + step_update of zf_train_kernels.h operation by operation in
    float32 (bias corrections formed in double and stored as float, as there):
    ``(theta_next, m, v)``.  ``fault``: one of FAULTS, a deliberately wrong
    variant for tests/test_train_ref_host.py."""
    f = np.float32
    theta, g, m, v = (np.asarray(a, f) for a in (theta, g, m, v))
    b1, b2, eps, wd, lr = (f(getattr(opt, k)) for k in ("b1", "b2", "eps", "weight_decay", "learning_rate"))
    one = f(1)
    if fault == "count_by_2":
        t = 2 * t
    bc1 = f(1.0 - float(opt.b1) ** t)
    bc1n = f(1.0 - float(opt.b1) ** (t if fault == "nesterov_b1t" else t + 1))
    bc2 = f(1.0 - float(opt.b2) ** t)
    if fault == "m_not_carried":
        m = np.zeros_like(m)
    with np.errstate(all="ignore"):
        mi = b1 * m + (one - b1) * g
        vi = b2 * v + (one - b2) * g * g
        mhat = b1 * (mi / bc1n) + (one - b1) * (g / bc1) if opt.nesterov else mi / bc1
        vhat = vi / bc2
        if fault == "decay_on_stepped":
            nxt = theta - lr * (mhat / (np.sqrt(vhat) + eps))
            nxt = nxt - lr * (wd * nxt)
        else:
            nxt = theta - lr * (mhat / (np.sqrt(vhat) + eps) + wd * theta)
    assert nxt.dtype == f and mi.dtype == f and vi.dtype == f
    return nxt, mi, vi


# ---- the free-running reference (child process) ----------------------------------
def _leaves(tree, path=()):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _leaves(tree[k], path + (k,))
    else:
        yield path, tree


def _set(tree, path, value):
    for k in path[:-1]:
        tree = tree.setdefault(k, {})
    tree[path[-1]] = value


def _free_run(case, opt, dtype, order):
    """T steps; ``order`` permutes the rows of every batch (None: as cut)."""
    import torch

    from oracle import zf_oracle as O
    from oracle import zf_oracle_torch as OT

    npdt = np.float64 if dtype == torch.float64 else np.float32
    variables = reset_shift_bounds(case["variables"])
    params = {}
    for path, leaf in _leaves(variables["params"]):
        _set(params, path, np.asarray(leaf, npdt))
    stats = variables["batch_stats"]
    mom = {path: (np.zeros(leaf.shape, npdt), np.zeros(leaf.shape, npdt)) for path, leaf in _leaves(params)}
    state = {path: adam_state(np.ones(leaf.shape, bool)) for path, leaf in _leaves(params)}
    losses = []
    for t, (lo, hi) in enumerate(trajectory_batches(case["x"].shape[0]), start=1):
        rows = np.arange(lo, hi) if order is None else lo + np.random.default_rng([order, t]).permutation(hi - lo)
        x = case["x"][rows]
        c = None if case["c"] is None else case["c"][rows]
        v = {"params": params, "batch_stats": stats}
        loss, g = OT.train_loss_and_grad(case["model"], v, x, c, dtype)
        _, ns = O.flow_log_prob(case["model"], v, x.astype(npdt), None if c is None else c.astype(npdt), train=True,
                                dtype=npdt)
        losses.append(loss)
        new = {}
        for path, leaf in _leaves(params):
            gl = g
            for k in path:
                gl = gl[k]
            if npdt is np.float64:
                nxt, state[path] = adam_reference(leaf, gl, state[path], t, opt)
            else:
                nxt, m, vv = adam_kernel_f32(leaf, gl, mom[path][0], mom[path][1], t, opt)
                mom[path] = (m, vv)
            _set(new, path, nxt)
        params, stats = new, {"bijector": ns}
    return np.asarray(losses, np.float64), params


def main(name, N, seed, nesterov, out):
    import torch

    from tests.flowcases import make_case

    torch.set_num_threads(1)  # one summation order for the float32 runs, whatever the host
    case = make_case(name, N=N, seed=seed)
    opt = Opt(nesterov=bool(nesterov))
    res = {}
    res["L64"], p = _free_run(case, opt, torch.float64, None)
    for path, leaf in _leaves(p):
        res["p64:" + "/".join(path)] = np.asarray(leaf, np.float64)
    for r in range(3):
        res[f"L32_{r}"], p = _free_run(case, opt, torch.float32, r or None)
        for path, leaf in _leaves(p):
            res[f"p32_{r}:" + "/".join(path)] = np.asarray(leaf, np.float64)
    np.savez(out, **res)


if __name__ == "__main__":
    os.environ["HIP_VISIBLE_DEVICES"] = ""  # this process never touches the GPU
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
