"""Weighted-loss oracle worker for tests/test_gpu_train_weighted.py: float64
autograd of the weighted train-mode loss

    loss = -sum_b w_b lp_b / sum_b w_b

which a user of the reference writes around ``flow.apply(..., train=True)``
(train.py:64-72 with weights).  The chain loop of
``oracle.zf_oracle_torch.train_loss_and_grad`` is restated over the oracle's
public pieces (``shift_bounds``, ``nsc``, ``latent_log_prob``): BatchNorm and
ShiftBounds take their batch statistics over all rows, the weights enter at
the loss only.  Emitted, in the key scheme of tests/grad_oracle.py and
tests/input_grad_oracle.py:

* ``loss64``, ``lp64`` (the rows' train-mode log_prob before nan_to_num);
* ``g64:<path>``: the parameter gradient in float64;
* ``g32_<r>:<path>``: the same in float32 over three row orders, the weights
  permuted along with the rows;
* ``g64p_<r>:<path>``: float64 at parameters and x jittered by 2^-22 relative;
* conditional cases: ``gc64``, ``gc32_<r>`` and ``gc64p_<r>`` (parameters, x
  and c jittered), d loss / d c in the rows' original order.

Runs in its own CPU-only process (importing torch into the GPU test process
would shadow the system librccl there).

    python -m tests.weighted_grad_oracle NAME N SEED OUT.npz"""

import copy
import os
import sys

import numpy as np

JITTER = 2.0**-22


def make_weights(N, seed):
    """The tests' weights: exponential(1), then (from 8 rows on) N // 8 rows
    at 0 and N // 16 rows at -0.25, each set drawn without replacement."""
    rng = np.random.default_rng(1000 + seed)
    w = rng.exponential(1.0, N).astype(np.float32)
    if N >= 8:
        w[rng.choice(N, N // 8, replace=False)] = 0.0
        w[rng.choice(N, N // 16, replace=False)] = -0.25
    return w


def _flat(tree, path=()):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _flat(tree[k], path + (k,))
    else:
        yield "/".join(path), np.asarray(tree, np.float64)


def weighted_loss_and_grads(model, variables, x, c, w, dtype):
    """(loss, lp, d loss / d params, d loss / d c or None)."""
    import torch

    from oracle import zf_oracle_torch as OT

    params = OT._tree(variables["params"]["bijector"], dtype, True)
    stats = variables.get("batch_stats", {}).get("bijector", {})
    xt = torch.tensor(np.asarray(x, np.float64), dtype=dtype)
    ct = None
    if c is not None:
        c = np.asarray(c, np.float64)
        ct = torch.tensor(c.reshape(-1, 1) if c.ndim == 1 else c, dtype=dtype, requires_grad=True)
    ld = torch.zeros(xt.shape[0], dtype=dtype)
    h = xt
    for i, b in enumerate(model["bijector"]["bijectors"]):
        key = f"bijectors_{i}"
        if b["type"] == "shift_bounds":
            h, l = OT.shift_bounds(b, stats.get(key, {}), h)
        elif b["type"] == "roll":
            h, l = torch.roll(h, b.get("shift", 1), dims=-1), None
        elif b["type"] == "nsc":
            h, l = OT.nsc(b, params[key], h, ct)
        else:
            raise ValueError(b["type"])
        if l is not None:
            ld = ld + l
    lp = OT.latent_log_prob(model["latent"], h) + ld
    wt = torch.tensor(np.asarray(w, np.float64), dtype=dtype)
    # flow.py:47's nan_to_num passes the cotangent where lp is finite only
    # (the cases the tests use have no other rows)
    fin = torch.isfinite(lp)
    loss = -(wt * torch.where(fin, lp, torch.zeros_like(lp))).sum() / wt.sum()
    loss.backward()
    gc = None if ct is None else ct.grad.detach().numpy().astype(np.float64)
    return (float(loss.detach()), lp.detach().numpy().astype(np.float64), {"bijector": OT._grads(params)}, gc)


def _jitter_in_place(tree, rng):
    """tests/grad_oracle.py's jitter (dict order, in place)."""
    for k in tree:
        if isinstance(tree[k], dict):
            _jitter_in_place(tree[k], rng)
        else:
            a = np.asarray(tree[k], np.float64)
            tree[k] = a * (1 + JITTER * rng.standard_normal(a.shape))


def _jitter_sorted(tree, rng):
    """tests/input_grad_oracle.py's jitter (sorted keys, a new tree)."""
    if isinstance(tree, dict):
        return {k: _jitter_sorted(tree[k], rng) for k in sorted(tree)}
    a = np.asarray(tree, np.float64)
    return a * (1 + JITTER * rng.standard_normal(a.shape))


def main(name, N, seed, out):
    import torch

    from tests.flowcases import make_case

    case = make_case(name, N=N, seed=seed)
    model, variables, x, c = case["model"], case["variables"], case["x"], case["c"]
    w = make_weights(N, seed)
    res = {}
    loss, lp, g64, gc = weighted_loss_and_grads(model, variables, x, c, w, torch.float64)
    res["loss64"], res["lp64"] = np.float64(loss), lp
    for k, v in _flat(g64):
        res["g64:" + k] = v
    if gc is not None:
        res["gc64"] = gc
    for r in range(3):
        p = np.random.default_rng(r).permutation(N) if r else np.arange(N)
        _, _, g32, gc32 = weighted_loss_and_grads(model, variables, x[p], None if c is None else c[p], w[p],
                                                  torch.float32)
        for k, v in _flat(g32):
            res[f"g32_{r}:" + k] = v
        if gc32 is not None:
            res[f"gc32_{r}"] = gc32[np.argsort(p)]
    x64 = x.astype(np.float64)
    for r in range(2):
        # the parameter gradient's conditioning, as tests/grad_oracle.py: parameters and x
        rng = np.random.default_rng(100 + r)
        v = copy.deepcopy(variables)
        _jitter_in_place(v["params"], rng)
        xp = x64 * (1 + JITTER * rng.standard_normal(x.shape))
        _, _, gp, _ = weighted_loss_and_grads(model, v, xp, c, w, torch.float64)
        for k, val in _flat(gp):
            res[f"g64p_{r}:" + k] = val
        if c is None:
            continue
        # d loss / d c's, as tests/input_grad_oracle.py: parameters, x and c
        rng = np.random.default_rng(100 + r)
        v = dict(variables, params={"bijector": _jitter_sorted(variables["params"]["bijector"], rng)})
        xp = x64 * (1 + JITTER * rng.standard_normal(x.shape))
        cp = np.asarray(c, np.float64)
        cp = cp * (1 + JITTER * rng.standard_normal(cp.shape))
        _, _, _, gcp = weighted_loss_and_grads(model, v, xp, cp, w, torch.float64)
        res[f"gc64p_{r}"] = gcp
    np.savez(out, **res)


if __name__ == "__main__":
    os.environ["HIP_VISIBLE_DEVICES"] = ""  # this process never touches the GPU (set before torch loads)
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
