"""Host reference of the optimiser chains (zenflow_amd/optim.py) in float64
NumPy, the tolerance an fp32 evaluation is held to, and that fp32 evaluation
itself (tests/test_optim_ref_host.py, tests/test_gpu_optim.py).

``chain_reference`` evaluates the formulas of zenflow_amd/optim.py's
docstring (restatements of optax's published ones) at the hyper-parameters
the device holds (``Stage.p32``: the C ABI carries them as float) and at
``lr = schedule(count)`` in float64.  Next to every first-moment array it
carries the absolute-value twin, as ``adam_state`` of tests/train_ref.py
does: ``A`` for adam's ``m`` and lion's ``mu``, and a trace of ``|u|``.

``chain_tolerance`` generalises ``adam_tolerance``; per element

    2^-23 |theta_ref| + (t + 8 + 2 S) 2^-23 span

with S the number of stages and ``span`` the chain evaluated on absolute
values, the magnitudes of ``scale`` and of the learning rate included (for a
chain that ends in the learning rate this is ``|lr_t|`` times the span of what
precedes it): g -> |g|, moments -> their twins, decay adds wd |theta|, the
global-norm clip factor is unchanged, ``clip(max_delta)`` bounds the span by
max_delta, lion's sign counts as 1.  The derivation is the one of
train_ref.py's docstring: each of the t accumulations rounds once against its
absolute sum, each stage adds at most two operations, the learning rate and
the clip factor are each one float rounding of a double, and the final store
rounds theta.

Lion's sign is discontinuous: an element whose |b1 mu + (1 - b1) g| is at
most (t + 4) 2^-23 (b1 A + (1 - b1) |g|) is ambiguous (``info["lion_ambiguous"]``)
and a test accepts sign -1, 0 or +1 for it (``lion_sign=`` forces one)."""

from __future__ import annotations

import numpy as np

from zenflow_amd import _lib as L

U23 = 2.0**-23


def chain_state(chain, mask):
    """Zero moments and twins over a flat blob; ``mask``: the parameter entries."""
    mask = np.asarray(mask).astype(bool)
    z = lambda: np.zeros(mask.shape, np.float64)  # noqa: E731
    stages = []
    for s in chain.stages:
        if s.kind == L.ZF_OPT_SCALE_BY_ADAM:
            stages.append({"m": z(), "v": z(), "A": z()})
        elif s.kind == L.ZF_OPT_SCALE_BY_LION:
            stages.append({"mu": z(), "A": z()})
        elif s.kind == L.ZF_OPT_TRACE:
            stages.append({"tr": z(), "T": z()})
        else:
            stages.append({})
    return {"mask": mask, "stages": stages, "info": None}


def slots_of(state, chain):
    """The moment arrays in chain order (what Trainer.opt_state()["slots"] holds, as blobs)."""
    out = []
    for s, st in zip(chain.stages, state["stages"]):
        out += [st[k] for k in {L.ZF_OPT_SCALE_BY_ADAM: ("m", "v"), L.ZF_OPT_SCALE_BY_LION: ("mu",),
                                L.ZF_OPT_TRACE: ("tr",)}.get(s.kind, ())]
    return out


def chain_reference(theta, g, state, count, chain, decay_mask=None, lion_sign=None):
    """The update number t = count + 1 from ``theta`` with gradient ``g``:
    ``(theta_next, new state)`` in float64.  Entries outside the state's mask
    keep their value and their zero moments.  ``new_state["info"]``: ``lr``,
    ``norm``, ``clip`` (factor), ``span`` and ``lion_ambiguous``."""
    mask = state["mask"]
    theta_all = np.asarray(theta, np.float64)
    theta = np.where(mask, theta_all, 0.0)  # the statistics may hold +-inf
    g = np.where(mask, np.asarray(g, np.float64), 0.0)
    t = count + 1
    u, a = g, np.abs(g)  # the update and its absolute-value evaluation
    info = {"lr": float("nan"), "norm": float("nan"), "clip": 1.0, "lion_ambiguous": np.zeros(mask.shape, bool)}
    new = []
    for s, st in zip(chain.stages, state["stages"]):
        p = s.p32
        ns = {}
        if s.kind == L.ZF_OPT_CLIP_BY_GLOBAL_NORM:
            n = float(np.sqrt(np.sum(u * u)))
            f = 1.0 if n < p[0] else p[0] / n
            info["norm"], info["clip"] = n, f
            u, a = u * f, a * f
        elif s.kind == L.ZF_OPT_CLIP:
            u, a = np.clip(u, -p[0], p[0]), np.minimum(a, p[0])
        elif s.kind == L.ZF_OPT_SCALE_BY_ADAM:
            b1, b2, eps, eps_root = p
            m = b1 * st["m"] + (1 - b1) * u
            v = b2 * st["v"] + (1 - b2) * u * u
            A = b1 * st["A"] + (1 - b1) * a
            if s.nesterov:
                mhat = b1 * m / (1 - b1 ** (t + 1)) + (1 - b1) * u / (1 - b1**t)
                ahat = b1 * A / (1 - b1 ** (t + 1)) + (1 - b1) * a / (1 - b1**t)
            else:
                mhat, ahat = m / (1 - b1**t), A / (1 - b1**t)
            den = np.sqrt(v / (1 - b2**t) + eps_root) + eps
            with np.errstate(invalid="ignore", divide="ignore"):
                u, a = np.where(mask, mhat / den, 0.0), np.where(mask, ahat / den, 0.0)
            ns = {"m": m, "v": v, "A": A}
        elif s.kind == L.ZF_OPT_SCALE_BY_LION:
            b1, b2 = p[0], p[1]
            c = b1 * st["mu"] + (1 - b1) * u
            info["lion_ambiguous"] = mask & (np.abs(c) <= (t + 4) * U23 * (b1 * st["A"] + (1 - b1) * a))
            ns = {"mu": b2 * st["mu"] + (1 - b2) * u, "A": b2 * st["A"] + (1 - b2) * a}
            u = np.sign(c) if lion_sign is None else np.where(mask, float(lion_sign), 0.0)
            a = np.where(mask, 1.0, 0.0)
        elif s.kind == L.ZF_OPT_TRACE:
            tr = u + p[0] * st["tr"]
            T = a + p[0] * st["T"]
            u, a = (u + p[0] * tr, a + p[0] * T) if s.nesterov else (tr, T)
            ns = {"tr": tr, "T": T}
        elif s.kind == L.ZF_OPT_ADD_DECAYED_WEIGHTS:
            on = mask if s.mask is None else mask & np.asarray(decay_mask).astype(bool)
            u, a = np.where(on, u + p[0] * theta, u), np.where(on, a + abs(p[0]) * np.abs(theta), a)
        elif s.kind == L.ZF_OPT_SCALE:
            u, a = p[0] * u, abs(p[0]) * a
        elif s.kind == L.ZF_OPT_SCALE_BY_LEARNING_RATE:
            lr = s.schedule(count)
            info["lr"] = lr
            u, a = -lr * u, abs(lr) * a
        else:
            raise ValueError(s.kind)
        new.append(ns)
    info["span"] = np.where(mask, a, 0.0)
    return np.where(mask, theta + u, theta_all), {"mask": mask, "stages": new, "info": info}


def chain_tolerance(theta_ref, state, t, chain):
    """The module docstring's bound per element; ``state`` is the one
    ``chain_reference`` returned with ``theta_ref``."""
    S = len(chain.stages)
    return U23 * np.abs(theta_ref) + (t + 8 + 2 * S) * U23 * state["info"]["span"]


# ---- the kernels' arithmetic in float32 --------------------------------------------
FAULTS = ("schedule_at_count_plus_1", "clip_below_max_norm", "norm_over_statistics", "nesterov_old_trace",
          "decay_mask_ignored", "lion_moment_b1", "eps_root_outside_sqrt")


def chain_kernel_f32(theta, g, slots, count, chain, mask, decay_mask=None, fault=None):
    """sumsq_leaf_kernel + opt_prologue_kernel + chain_update_kernel of
    zf_optim.hip operation by operation: the scalars (norm, clip factor,
    learning rate, bias corrections) formed in double and stored as float,
    the stages in float32.  The generic stage loop and the specialised forms
    share their stage functions, so this is the arithmetic of every form.
    ``(theta_next, slots)``; ``fault``: one of FAULTS, a deliberately wrong
    variant for tests/test_optim_ref_host.py."""
    f = np.float32
    mask = np.asarray(mask).astype(bool)
    theta, g = np.asarray(theta, f), np.asarray(g, f)
    slots = [np.asarray(s, f) for s in slots]
    t = count + 1
    u = g
    out_slots = []
    at = 0
    one = f(1)
    with np.errstate(all="ignore"):
        for s in chain.stages:
            p = [f(v) for v in s.p]
            if s.kind == L.ZF_OPT_CLIP_BY_GLOBAL_NORM:
                sel = np.ones_like(mask) if fault == "norm_over_statistics" else mask
                n = float(np.sqrt(np.sum(np.where(sel, g.astype(np.float64), 0.0) ** 2)))
                below = n < float(p[0]) and fault != "clip_below_max_norm"
                u = u * f(1.0 if below else float(p[0]) / n)
            elif s.kind == L.ZF_OPT_CLIP:
                u = np.where(u != u, u, np.minimum(np.maximum(u, -p[0]), p[0]))
            elif s.kind == L.ZF_OPT_SCALE_BY_ADAM:
                b1, b2, eps, eps_root = p
                bc1 = f(1.0 - float(b1) ** t)
                bc1n = f(1.0 - float(b1) ** (t + 1))
                bc2 = f(1.0 - float(b2) ** t)
                mi = b1 * slots[at] + (one - b1) * u
                vi = b2 * slots[at + 1] + (one - b2) * u * u
                mhat = b1 * (mi / bc1n) + (one - b1) * (u / bc1) if s.nesterov else mi / bc1
                vhat = vi / bc2
                if fault == "eps_root_outside_sqrt":
                    u = mhat / (np.sqrt(vhat) + eps_root + eps)
                else:
                    u = mhat / (np.sqrt(vhat + eps_root) + eps)
                out_slots += [mi, vi]
                at += 2
            elif s.kind == L.ZF_OPT_SCALE_BY_LION:
                b1, b2 = p[0], p[1]
                c = b1 * slots[at] + (one - b1) * u
                bm = b1 if fault == "lion_moment_b1" else b2
                out_slots.append(bm * slots[at] + (one - bm) * u)
                u = np.where(c > 0, one, np.where(c < 0, -one, c)).astype(f)
                at += 1
            elif s.kind == L.ZF_OPT_TRACE:
                ti = u + p[0] * slots[at]
                u = (u + p[0] * (slots[at] if fault == "nesterov_old_trace" else ti)) if s.nesterov else ti
                out_slots.append(ti)
                at += 1
            elif s.kind == L.ZF_OPT_ADD_DECAYED_WEIGHTS:
                on = np.ones_like(mask) if s.mask is None or fault == "decay_mask_ignored" else \
                    np.asarray(decay_mask).astype(bool)
                u = np.where(on, u + p[0] * theta, u)
            elif s.kind == L.ZF_OPT_SCALE:
                u = p[0] * u
            elif s.kind == L.ZF_OPT_SCALE_BY_LEARNING_RATE:
                lr = f(s.schedule(count + 1 if fault == "schedule_at_count_plus_1" else count))
                u = -(lr * u)
            assert u.dtype == f, s.name
        nxt = np.where(mask, theta + u, theta)
    assert nxt.dtype == f and all(s.dtype == f for s in out_slots)
    # entries outside the mask are skipped by the kernel: their moments stay
    out_slots = [np.where(mask, new, old) for new, old in zip(out_slots, slots)]
    return nxt, out_slots


# ---- the blob layout without a device ------------------------------------------------
def host_program(cfg, variables):
    """The engine's Program for ``build_flow(cfg)`` and ``variables`` up to the
    point where it would touch the device: blob, param_mask and
    blob_to_variables (zf_flow_plan is host code)."""
    import ctypes as ct

    from tests.flowcases import build_flow
    from zenflow_amd import engine as E

    flow = build_flow(cfg)
    prog = E.Program.__new__(E.Program)
    prog.handle = None
    prog.root, prog.D, prog.C = flow.bijector, cfg["D"], cfg["C"]
    prog.ops = E.flatten(flow.bijector)
    desc = L.ZfFlowDesc()
    desc.dim, desc.cond_dim, desc.latent, desc.n_ops = prog.D, prog.C, L.ZF_LATENT_NORMAL, len(prog.ops)
    for i, op in enumerate(prog.ops):
        d = desc.ops[i]
        d.kind = op.kind
        if op.kind == L.ZF_OP_ROLL:
            d.shift = int(op.module.shift)
        elif op.kind == L.ZF_OP_NSC:
            d.knots, d.n_hidden, d.act = int(op.module.knots), len(op.module.layers), int(op.module.act_code)
            for l, w in enumerate(op.module.layers):
                d.hidden[l] = int(w)
    n = ct.c_int64()
    L.check(L.load_library().zf_flow_plan(ct.byref(desc), ct.byref(n)), "zf_flow_plan")
    prog.desc = desc
    prog.blob = np.zeros(n.value, np.float32)
    prog.param_mask = np.zeros(n.value, np.uint8)
    sub = {k: v.get("bijector", {}) for k, v in variables.items()}
    prog._fill_blob(desc, prog.blob, sub.get("params", {}), sub.get("batch_stats", {}))
    return prog


def no_decay_on_biases_and_batchnorm(params):
    """The usual weight-decay mask: Dense kernels only (a callable mask)."""
    def walk(tree, name=""):
        if isinstance(tree, dict):
            return {k: walk(v, k) for k, v in tree.items()}
        return name == "kernel"

    return walk(params)


def chain_check(got, theta, g, state, count, chain, decay_mask=None):
    """``got`` (the fp32 step's parameters) against the reference step from
    ``theta`` and ``g``: ``(error / tolerance per element (0 outside the
    mask), new state, number of ambiguous lion elements)``.  An ambiguous
    element is checked against the three sign candidates and keeps the best
    ratio; every other element against the one reference."""
    t = count + 1
    ref, new = chain_reference(theta, g, state, count, chain, decay_mask)
    mask = new["mask"]
    got = np.where(mask, np.asarray(got, np.float64), 0.0)

    def ratio_to(ref, state):
        r = np.abs(got - np.where(mask, ref, 0.0)) / np.maximum(chain_tolerance(ref, state, t, chain), 1e-300)
        return np.where(np.isnan(r), np.inf, r)  # a NaN parameter is outside every tolerance

    ratio = ratio_to(ref, new)
    amb = new["info"]["lion_ambiguous"]
    if amb.any():
        for sign in (-1.0, 0.0, 1.0):
            r2, n2 = chain_reference(theta, g, state, count, chain, decay_mask, lion_sign=sign)
            ratio = np.where(amb, np.minimum(ratio, ratio_to(r2, n2)), ratio)
    return np.where(mask, ratio, 0.0), new, int(amb.sum())
