"""Custom-loss oracle worker for tests/test_gpu_custom_loss.py: float64
autograd of

    sum_b cot_b * where(isfinite(lp_b), lp_b, 0)

with respect to the flow's parameters (and c), lp the train- or eval-mode
log_prob of ``tests.input_grad_oracle.flow_lp`` — what ``jax.grad`` of a
user's loss around ``flow.apply`` (train.py:64-86, flow.py:22-48) sends back
for ``cot = d loss / d lp``.  No arithmetic of its own: the flow is
``flow_lp``'s, the parameters carry ``requires_grad``.

The cotangent is ``standard_normal(rows)`` from ``default_rng(2000 + seed)``
(mixed signs on purpose).  Emitted, in the key scheme of
tests/weighted_grad_oracle.py:

* ``lp64`` (all rows, before nan_to_num), ``lp32_<r>``, ``lp64p_<r>``, ``cot``,
  ``dropped``;
* ``g64:<path>``, ``g32_<r>:<path>`` (float32, three row orders) and
  ``g64p_<r>:<path>`` (float64 at parameters and x jittered by 2^-22);
* conditional cases: ``gc64``, ``gc32_<r>``, ``gc64p_<r>`` (parameters, x and
  c jittered), rows in their original order.

``dropped``: rows autograd itself loses — a finite log_prob whose gradient is
NaN (an eval-mode sample clipped onto a spline end runs the interior formula
on the fill-mode NaN knots in the unselected ``where`` branch, the artefact
``tests.test_gpu_input_grad.check_columns`` documents).  Eval rows are
independent, so those rows are left out of the sum (the flow runs on the other
rows only; their ``gc`` rows are zero); the GPU call gives them cotangent 0.
Rows that a float32 or jittered evaluation loses are dropped with them, as
``check_columns`` leaves them out.  At most 2% of a case's rows
(``check_columns``' cap, asserted here); train mode must lose none.

Runs in its own CPU-only process (importing torch into the GPU test process
would shadow the system librccl there).

    python -m tests.custom_loss_oracle NAME N SEED train|eval OUT.npz"""

import copy
import os
import sys

import numpy as np

from tests.weighted_grad_oracle import JITTER, _flat, _jitter_in_place, _jitter_sorted


def make_cot(N, seed):
    return np.random.default_rng(2000 + seed).standard_normal(N)


def custom_grads(model, variables, x, c, cot, train, dtype, keep=None, want_gx=False):
    """(lp before nan_to_num, d / d params, d / d c or None, d / d x or None) of
    sum(cot * where(isfinite(lp), lp, 0)) over the rows ``keep`` (default all)."""
    import torch

    from oracle import zf_oracle_torch as OT
    from tests.input_grad_oracle import flow_lp

    N = np.asarray(x).shape[0]
    rows = np.arange(N) if keep is None else np.flatnonzero(keep)
    params = OT._tree(variables["params"]["bijector"], dtype, True)
    stats = variables.get("batch_stats", {}).get("bijector", {})
    xt = torch.tensor(np.asarray(x, np.float64)[rows], dtype=dtype, requires_grad=want_gx)
    ct = None
    if c is not None:
        c = np.asarray(c, np.float64)
        ct = torch.tensor((c.reshape(-1, 1) if c.ndim == 1 else c)[rows], dtype=dtype, requires_grad=True)
    lp = flow_lp(OT, model, params, stats, xt, ct, train=train)
    fin = torch.isfinite(lp)
    total = (torch.tensor(np.asarray(cot, np.float64)[rows], dtype=dtype) * torch.where(fin, lp, torch.zeros_like(lp))).sum()
    total.backward()

    def full(t, width):
        out = np.zeros((N, width), np.float64)
        out[rows] = t.detach().numpy().astype(np.float64)
        return out

    lp_all = np.full(N, np.nan)
    lp_all[rows] = lp.detach().numpy().astype(np.float64)
    gc = None if ct is None else full(ct.grad, ct.shape[1])
    gx = full(xt.grad, xt.shape[1]) if want_gx else None
    return lp_all, {"bijector": OT._grads(params)}, gc, gx


def lost_rows(model, variables, x, c, cot, train):
    """Rows with a finite float64 log_prob whose autograd gradient is NaN."""
    import torch

    lp, _, gc, gx = custom_grads(model, variables, x, c, np.ones_like(cot), train, torch.float64, want_gx=True)
    nan = ~np.isfinite(gx).all(axis=1)
    if gc is not None:
        nan |= ~np.isfinite(gc).all(axis=1)
    return lp, nan & np.isfinite(lp)


def main(name, N, seed, mode, out):
    import torch

    from tests.flowcases import make_case

    train = {"train": True, "eval": False}[mode]
    case = make_case(name, N=N, seed=seed)
    model, variables, x, c = case["model"], case["variables"], case["x"], case["c"]
    cot = make_cot(N, seed)
    x64 = x.astype(np.float64)
    # every evaluation below: (tag, variables, x, c, row order, dtype)
    ident = np.arange(N)
    evals = [("64", variables, x, c, ident, torch.float64)]
    for r in range(3):
        evals.append((f"32_{r}", variables, x, c, np.random.default_rng(r).permutation(N) if r else ident,
                      torch.float32))
    for r in range(2):
        # the parameter gradient's conditioning, as tests/grad_oracle.py: parameters and x
        rng = np.random.default_rng(100 + r)
        v = copy.deepcopy(variables)
        _jitter_in_place(v["params"], rng)
        evals.append((f"64p_{r}", v, x64 * (1 + JITTER * rng.standard_normal(x.shape)), c, ident, torch.float64))
        if c is None:
            continue
        # d / d c's, as tests/input_grad_oracle.py: parameters, x and c
        rng = np.random.default_rng(100 + r)
        v = dict(variables, params={"bijector": _jitter_sorted(variables["params"]["bijector"], rng)})
        xp = x64 * (1 + JITTER * rng.standard_normal(x.shape))
        cp = np.asarray(c, np.float64)
        evals.append((f"c64p_{r}", v, xp, cp * (1 + JITTER * rng.standard_normal(cp.shape)), ident, torch.float64))

    def run(e, keep, **kw):
        tag, v, xe, ce, p, dtype = e
        lp, g, gc, gx = custom_grads(model, v, xe[p], None if ce is None else ce[p], cot[p], train, dtype,
                                     None if keep is None else keep[p], **kw)
        inv = np.argsort(p)
        return lp[inv], g, None if gc is None else gc[inv], None if gx is None else gx[inv]

    res = {"cot": cot}
    # the rows autograd loses: in float64, and (eval mode, where rows are
    # independent) in any of the float32 or jittered evaluations as well, so
    # that every emitted gradient is finite whichever CPU rounds the float32 passes
    dropped = np.zeros(N, bool)
    for e in evals if not train else evals[:1]:
        lp, _, gc, gx = run(e, None, want_gx=True)
        nan = ~np.isfinite(gx).all(axis=1)
        if gc is not None:
            nan |= ~np.isfinite(gc).all(axis=1)
        dropped |= nan & np.isfinite(lp)
        if e[0] in ("64", "32_0", "32_1", "32_2", "64p_0", "64p_1"):
            res["lp" + e[0]] = lp
    assert dropped.mean() <= 0.02, f"{name}/{N}/{mode}: {dropped.sum()} of {N} rows lost"
    assert not (train and dropped.any()), "train mode: the batch statistics tie the rows together"
    res["dropped"] = dropped
    keep = None if train else ~dropped
    for e in evals:
        tag = e[0]
        lp, g, gc, _ = run(e, keep)
        if train and tag != "64" and not tag.startswith("c"):
            res["lp" + tag] = lp
        if tag.startswith("c"):
            res["g" + tag] = gc
            continue
        for k, val in _flat(g):
            res[f"g{tag}:" + k] = val
        if gc is not None and not tag.startswith("64p"):
            res["gc" + tag] = gc
    np.savez(out, **res)


if __name__ == "__main__":
    os.environ["HIP_VISIBLE_DEVICES"] = ""  # this process never touches the GPU (set before torch loads)
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5])
