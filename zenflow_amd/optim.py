"""Optimiser chains that run on the device (optax's gradient transformations).

The reference's ``train()`` takes any ``optax.GradientTransformation``
(src/zenflow/train.py:27, 62, 84-85); its users build
``optax.chain(optax.clip_by_global_norm(1.0), optax.adamw(schedule))`` and the
like.  This module has optax's names, argument names and defaults, and lowers
a chain to the stage list of include/zenflow_amd.h (``zf_optim_chain``), which
the trainer runs inside its step — three kernels, no host synchronisation.

optax cannot be imported here, so every formula below is a RESTATEMENT of
optax's published one (optax/_src/transform.py, clipping.py, schedule.py,
alias.py), not a call into it.  ``count`` is the number of updates already
applied (0 at the first update), ``t = count + 1``, ``u`` starts as the
gradient ``g`` and the step ends with ``theta <- theta + u``.

Transformations (one stage each):

* ``clip_by_global_norm(max_norm)``: n = sqrt(sum u^2) over all parameter
  entries; u <- u if n < max_norm else (u / n) max_norm.  On the device the
  factor max_norm / n is formed in double and applied as one float.  It must
  be the first stage (the norm is the raw gradient's), once.
* ``clip(max_delta)``: u <- clamp(u, -max_delta, max_delta).
* ``scale_by_adam(b1=0.9, b2=0.999, eps=1e-8, eps_root=0.0, nesterov=False)``:
  m <- b1 m + (1 - b1) u, v <- b2 v + (1 - b2) u^2,
  mhat = m / (1 - b1^t), or with nesterov
  b1 m / (1 - b1^(t+1)) + (1 - b1) u / (1 - b1^t); vhat = v / (1 - b2^t);
  u <- mhat / (sqrt(vhat + eps_root) + eps).  At most one per chain.
* ``scale_by_lion(b1=0.9, b2=0.99)``: u <- sign(b1 mu + (1 - b1) g), then
  mu <- b2 mu + (1 - b2) g.
* ``trace(decay, nesterov=False)``: tr <- u + decay tr; u <- u + decay tr
  with nesterov, else tr.
* ``add_decayed_weights(weight_decay, mask=None)``: u <- u + weight_decay
  theta where the mask is true (everywhere without one).  ``mask``: a pytree
  of bools shaped like ``variables["params"]``, or a callable from that tree
  to one.
* ``scale(step_size)``: u <- step_size u.
* ``scale_by_learning_rate(learning_rate)``: u <- -lr(count) u, the learning
  rate a float or a schedule.  At most one per chain.
* ``chain(*transformations)`` flattens nested chains.

Aliases (chains): ``sgd``, ``adam``, ``nadam``, ``adamw``, ``nadamw``, ``lion``.

Schedules are plain objects, called on the host as ``schedule(count)`` in
float64 — the oracle of what the device evaluates from its own counter:

* ``constant_schedule(value)``
* ``linear_schedule(init_value, end_value, transition_steps,
  transition_begin=0)``: c = clip(count - begin, 0, steps);
  (init - end) (1 - c / steps) + end.
* ``cosine_decay_schedule(init_value, decay_steps, alpha=0.0, exponent=1.0)``:
  c = min(count, decay_steps); d = 0.5 (1 + cos(pi c / decay_steps));
  init ((1 - alpha) d^exponent + alpha).
* ``exponential_decay(init_value, transition_steps, decay_rate,
  transition_begin=0, staircase=False, end_value=None)``: p = (count - begin)
  / steps, floored if staircase; init if count - begin <= 0 else init rate^p;
  bounded by end_value from below if rate < 1, from above otherwise.
* ``warmup_cosine_decay_schedule(init_value, peak_value, warmup_steps,
  decay_steps, end_value=0.0, exponent=1.0)``: linear warm-up joined at
  warmup_steps to a cosine decay over decay_steps - warmup_steps.
* ``join_schedules(schedules, boundaries)``: segment k sees count -
  boundaries[k-1]; up to 4 segments.
* ``piecewise_constant_schedule(init_value, boundaries_and_scales)``: init
  times every scale whose boundary < count; up to 3 boundaries.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Callable, Dict, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib as L

__all__ = [
    "Chain", "Stage", "Schedule", "chain", "clip_by_global_norm", "clip", "scale_by_adam", "scale_by_lion", "trace",
    "add_decayed_weights", "scale", "scale_by_learning_rate", "sgd", "adam", "nadam", "adamw", "nadamw", "lion",
    "constant_schedule", "linear_schedule", "cosine_decay_schedule", "exponential_decay",
    "warmup_cosine_decay_schedule", "join_schedules", "piecewise_constant_schedule", "lower_mask",
]


# ---- schedules -------------------------------------------------------------------
def _segment_value(kind: int, p: Sequence[float], c: float) -> float:
    """One segment at c = count - boundary, operation by operation as
    sched_segment in zf_optim.hip."""
    if kind == L.ZF_SCHED_LINEAR:
        init, end, steps, begin = p[0], p[1], p[2], p[3]
        if steps <= 0.0:
            return init
        cc = min(max(c - begin, 0.0), steps)
        return (init - end) * (1.0 - cc / steps) + end
    if kind == L.ZF_SCHED_COSINE:
        init, steps, alpha, ex = p[0], p[1], p[2], p[3]
        cc = min(c, steps)
        d = 0.5 * (1.0 + math.cos(math.pi * cc / steps))
        return init * ((1.0 - alpha) * math.pow(d, ex) + alpha)
    if kind == L.ZF_SCHED_EXPONENTIAL:
        init, steps, rate, begin = p[0], p[1], p[2], p[3]
        dc = c - begin
        if dc <= 0.0:
            return init
        q = dc / steps
        if p[4] != 0.0:
            q = math.floor(q)
        v = init * math.pow(rate, q)
        if p[6] != 0.0:
            v = max(v, p[5]) if rate < 1.0 else min(v, p[5])
        return v
    if kind == L.ZF_SCHED_PIECEWISE:
        v = p[0]
        for i in range(int(p[1])):
            if p[2 + 2 * i] < c:
                v = v * p[3 + 2 * i]
        return v
    return p[0]


class Schedule:
    """count -> value.  ``segments``: ((boundary, kind, params), ...), the
    segment of a count being the last one whose boundary it has reached."""

    def __init__(self, segments):
        self.segments = tuple((float(b), int(k), tuple(float(v) for v in p) + (0.0,) * (L.ZF_SCHED_PARAMS - len(p)))
                              for b, k, p in segments)

    def __call__(self, count) -> float:
        count = float(count)
        at = 0
        for i in range(1, len(self.segments)):
            if count >= self.segments[i][0]:
                at = i
        b, kind, p = self.segments[at]
        return float(_segment_value(kind, p, count - b if at else count))

    def lower(self) -> L.ZfSchedule:
        n = len(self.segments)
        if n > L.ZF_SCHED_MAX_SEGMENTS:
            raise NotImplementedError(f"join_schedules: {n} joined segments (at most {L.ZF_SCHED_MAX_SEGMENTS})")
        s = L.ZfSchedule()
        s.kind = self.segments[0][1] if n == 1 else L.ZF_SCHED_JOIN
        s.n_segments = n
        for i, (b, kind, p) in enumerate(self.segments):
            s.seg_kind[i] = kind
            s.boundary[i] = b
            for j, v in enumerate(p):
                s.p[i][j] = v
        return s


def constant_schedule(value: float) -> Schedule:
    return Schedule([(0, L.ZF_SCHED_CONSTANT, (value,))])


def linear_schedule(init_value: float, end_value: float, transition_steps: int, transition_begin: int = 0) -> Schedule:
    return Schedule([(0, L.ZF_SCHED_LINEAR, (init_value, end_value, transition_steps, transition_begin))])


def cosine_decay_schedule(init_value: float, decay_steps: int, alpha: float = 0.0, exponent: float = 1.0) -> Schedule:
    if not decay_steps > 0:
        raise ValueError("cosine_decay_schedule requires positive decay_steps")
    return Schedule([(0, L.ZF_SCHED_COSINE, (init_value, decay_steps, alpha, exponent))])


def exponential_decay(init_value: float, transition_steps: int, decay_rate: float, transition_begin: int = 0,
                      staircase: bool = False, end_value: Optional[float] = None) -> Schedule:
    if not transition_steps > 0:
        raise ValueError("exponential_decay requires positive transition_steps")
    return Schedule([(0, L.ZF_SCHED_EXPONENTIAL,
                      (init_value, transition_steps, decay_rate, transition_begin, 1.0 if staircase else 0.0,
                       0.0 if end_value is None else end_value, 0.0 if end_value is None else 1.0))])


def join_schedules(schedules: Sequence[Schedule], boundaries: Sequence[int]) -> Schedule:
    """Segment k (k >= 1) runs from boundaries[k-1] and sees count -
    boundaries[k-1]; a joined schedule may itself be a join."""
    if len(schedules) != len(boundaries) + 1:
        raise ValueError("join_schedules: one boundary fewer than schedules")
    segs = []
    for k, s in enumerate(schedules):
        s = _as_schedule(s)
        base = 0.0 if k == 0 else float(boundaries[k - 1])
        for b, kind, p in s.segments:
            segs.append((base + b, kind, p))
    if len(segs) > L.ZF_SCHED_MAX_SEGMENTS:
        raise NotImplementedError(f"join_schedules: {len(segs)} joined segments (at most {L.ZF_SCHED_MAX_SEGMENTS})")
    if any(segs[i][0] > segs[i + 1][0] for i in range(len(segs) - 1)):
        raise ValueError("join_schedules: boundaries must not decrease")
    return Schedule(segs)


def warmup_cosine_decay_schedule(init_value: float, peak_value: float, warmup_steps: int, decay_steps: int,
                                 end_value: float = 0.0, exponent: float = 1.0) -> Schedule:
    alpha = 0.0 if peak_value == 0.0 else end_value / peak_value
    return join_schedules([linear_schedule(init_value, peak_value, warmup_steps),
                           cosine_decay_schedule(peak_value, decay_steps - warmup_steps, alpha, exponent)],
                          [warmup_steps])


def piecewise_constant_schedule(init_value: float, boundaries_and_scales: Optional[Dict[int, float]] = None) -> Schedule:
    items = sorted((boundaries_and_scales or {}).items())
    if len(items) > 3:
        raise NotImplementedError(f"piecewise_constant_schedule: {len(items)} boundaries (at most 3)")
    p = [init_value, float(len(items))]
    for b, s in items:
        p += [b, s]
    return Schedule([(0, L.ZF_SCHED_PIECEWISE, p)])


def _as_schedule(lr) -> Schedule:
    return lr if isinstance(lr, Schedule) else constant_schedule(float(lr))


# ---- transformations ---------------------------------------------------------------
_NAMES = {
    L.ZF_OPT_CLIP_BY_GLOBAL_NORM: "clip_by_global_norm", L.ZF_OPT_CLIP: "clip",
    L.ZF_OPT_SCALE_BY_ADAM: "scale_by_adam", L.ZF_OPT_SCALE_BY_LION: "scale_by_lion", L.ZF_OPT_TRACE: "trace",
    L.ZF_OPT_ADD_DECAYED_WEIGHTS: "add_decayed_weights", L.ZF_OPT_SCALE: "scale",
    L.ZF_OPT_SCALE_BY_LEARNING_RATE: "scale_by_learning_rate",
}
_SLOTS = {L.ZF_OPT_SCALE_BY_ADAM: 2, L.ZF_OPT_SCALE_BY_LION: 1, L.ZF_OPT_TRACE: 1}


@dataclass(frozen=True)
class Stage:
    """One gradient transformation: ``kind`` (ZF_OPT_*), up to four float
    hyper-parameters ``p`` (the device holds them as float32), ``nesterov``,
    and the learning-rate stage's ``schedule`` / the decay stage's ``mask``."""

    kind: int
    p: Tuple[float, ...] = ()
    nesterov: bool = False
    schedule: Optional[Schedule] = None
    mask: Any = None

    @property
    def name(self) -> str:
        return _NAMES[self.kind]

    @property
    def n_slots(self) -> int:
        return _SLOTS.get(self.kind, 0)

    @property
    def p32(self) -> Tuple[float, ...]:
        """The hyper-parameters as the device holds them."""
        return tuple(float(np.float32(v)) for v in self.p)


class Chain:
    """``optax.chain``: stages applied in order, then theta <- theta + u."""

    def __init__(self, stages: Sequence[Stage]):
        self.stages = tuple(stages)

    def __iter__(self):
        return iter(self.stages)

    def __len__(self):
        return len(self.stages)

    def __repr__(self):
        return "chain(" + ", ".join(s.name for s in self.stages) + ")"

    @property
    def n_slots(self) -> int:
        return sum(s.n_slots for s in self.stages)

    def validate(self) -> None:
        """What zf_trainer_set_optim_chain rejects (ZF_ENOTSUP), on the host."""
        if not self.stages:
            raise ValueError("optimiser chain: no stage")
        if len(self.stages) > L.ZF_OPT_MAX_STAGES:
            raise NotImplementedError(f"optimiser chain: {len(self.stages)} stages (at most {L.ZF_OPT_MAX_STAGES}): "
                                      f"stage {L.ZF_OPT_MAX_STAGES} is {self.stages[L.ZF_OPT_MAX_STAGES].name}")
        seen: Dict[int, int] = {}
        slots = 0
        masks = []
        for k, s in enumerate(self.stages):
            seen[s.kind] = seen.get(s.kind, 0) + 1
            once = (L.ZF_OPT_CLIP_BY_GLOBAL_NORM, L.ZF_OPT_SCALE_BY_ADAM, L.ZF_OPT_SCALE_BY_LEARNING_RATE)
            if s.kind in once and seen[s.kind] > 1:
                raise NotImplementedError(f"optimiser chain: stage {k}: more than one {s.name}")
            if s.kind == L.ZF_OPT_CLIP_BY_GLOBAL_NORM and k != 0:
                raise NotImplementedError(
                    f"optimiser chain: stage {k}: clip_by_global_norm after {self.stages[k - 1].name} (it must come "
                    "before every stage that changes the update: the norm is the raw gradient's)")
            slots += s.n_slots
            if slots > L.ZF_OPT_MAX_SLOTS:
                raise NotImplementedError(f"optimiser chain: stage {k} ({s.name}) needs moment array {slots} "
                                          f"(at most {L.ZF_OPT_MAX_SLOTS})")
            if s.kind == L.ZF_OPT_ADD_DECAYED_WEIGHTS and s.mask is not None:
                masks.append(k)
            if s.schedule is not None:
                s.schedule.lower()
        if len(masks) > 1:
            raise NotImplementedError(f"optimiser chain: stage {masks[1]}: more than one masked add_decayed_weights")

    def lower(self) -> L.ZfOptimChain:
        self.validate()
        c = L.ZfOptimChain()
        c.n_stages = len(self.stages)
        for k, s in enumerate(self.stages):
            st = c.stages[k]
            st.kind = s.kind
            st.flags = (L.ZF_OPT_FLAG_NESTEROV if s.nesterov else 0) | (L.ZF_OPT_FLAG_MASKED if s.mask is not None else 0)
            for j, v in enumerate(s.p):
                st.p[j] = v
            if s.schedule is not None:
                st.sched = s.schedule.lower()
        return c

    def mask(self):
        """The mask of the masked add_decayed_weights stage, or None."""
        for s in self.stages:
            if s.kind == L.ZF_OPT_ADD_DECAYED_WEIGHTS and s.mask is not None:
                return s.mask
        return None


def chain(*transformations: Union[Stage, Chain]) -> Chain:
    stages = []
    for tr in transformations:
        if isinstance(tr, Chain):
            stages.extend(tr.stages)
        elif isinstance(tr, Stage):
            stages.append(tr)
        else:
            raise TypeError(f"chain: {tr!r} is not a transformation of zenflow_amd.optim")
    return Chain(stages)


def clip_by_global_norm(max_norm: float) -> Stage:
    return Stage(L.ZF_OPT_CLIP_BY_GLOBAL_NORM, (max_norm,))


def clip(max_delta: float) -> Stage:
    return Stage(L.ZF_OPT_CLIP, (max_delta,))


def scale_by_adam(b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, eps_root: float = 0.0,
                  nesterov: bool = False) -> Stage:
    return Stage(L.ZF_OPT_SCALE_BY_ADAM, (b1, b2, eps, eps_root), nesterov=bool(nesterov))


def scale_by_lion(b1: float = 0.9, b2: float = 0.99) -> Stage:
    return Stage(L.ZF_OPT_SCALE_BY_LION, (b1, b2))


def trace(decay: float, nesterov: bool = False) -> Stage:
    return Stage(L.ZF_OPT_TRACE, (decay,), nesterov=bool(nesterov))


def add_decayed_weights(weight_decay: float = 0.0, mask=None) -> Stage:
    return Stage(L.ZF_OPT_ADD_DECAYED_WEIGHTS, (weight_decay,), mask=mask)


def scale(step_size: float) -> Stage:
    return Stage(L.ZF_OPT_SCALE, (step_size,))


def scale_by_learning_rate(learning_rate) -> Stage:
    return Stage(L.ZF_OPT_SCALE_BY_LEARNING_RATE, (), schedule=_as_schedule(learning_rate))


# ---- aliases ---------------------------------------------------------------------------
def sgd(learning_rate, momentum: Optional[float] = None, nesterov: bool = False) -> Chain:
    if momentum is None:
        return chain(scale_by_learning_rate(learning_rate))
    return chain(trace(momentum, nesterov), scale_by_learning_rate(learning_rate))


def adam(learning_rate, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, eps_root: float = 0.0,
         nesterov: bool = False) -> Chain:
    return chain(scale_by_adam(b1, b2, eps, eps_root, nesterov), scale_by_learning_rate(learning_rate))


def nadam(learning_rate, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, eps_root: float = 0.0) -> Chain:
    return adam(learning_rate, b1, b2, eps, eps_root, nesterov=True)


def adamw(learning_rate, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, eps_root: float = 0.0,
          weight_decay: float = 1e-4, mask=None, nesterov: bool = False) -> Chain:
    return chain(scale_by_adam(b1, b2, eps, eps_root, nesterov), add_decayed_weights(weight_decay, mask),
                 scale_by_learning_rate(learning_rate))


def nadamw(learning_rate, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, eps_root: float = 0.0,
           weight_decay: float = 1e-4, mask=None) -> Chain:
    return adamw(learning_rate, b1, b2, eps, eps_root, weight_decay, mask, nesterov=True)


def lion(learning_rate, b1: float = 0.9, b2: float = 0.99, weight_decay: float = 1e-3, mask=None) -> Chain:
    return chain(scale_by_lion(b1, b2), add_decayed_weights(weight_decay, mask), scale_by_learning_rate(learning_rate))


# ---- trees <-> blob ----------------------------------------------------------------------
def _walk(tree, path=()):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _walk(tree[k], path + (k,))
    else:
        yield path, tree


def blob_index(program) -> Dict[Tuple[str, ...], np.ndarray]:
    """{path of a ``params`` leaf (below "bijector"): the blob offsets of its
    entries}, from blob_to_variables of the offsets themselves (in two float32
    halves, exact for any blob length)."""
    n = program.blob.size
    at = np.arange(n, dtype=np.int64)
    lo = program.blob_to_variables((at % 4096).astype(np.float32))["params"]
    hi = program.blob_to_variables((at // 4096).astype(np.float32))["params"]
    hi = dict(_walk(hi))
    return {p: (np.asarray(hi[p]).astype(np.int64) * 4096 + np.asarray(leaf).astype(np.int64))
            for p, leaf in _walk(lo)}


def _get(tree, path):
    for k in path:
        if not isinstance(tree, dict) or k not in tree:
            return None
        tree = tree[k]
    return tree


def tree_to_blob(program, tree, dtype=np.float32) -> np.ndarray:
    """A ``variables["params"]``-shaped tree -> blob layout (zero elsewhere)."""
    out = np.zeros(program.blob.size, dtype)
    inner = tree.get("bijector", {}) if isinstance(tree, dict) else {}
    for path, ix in blob_index(program).items():
        leaf = _get(inner, path)
        if leaf is None:
            raise ValueError(f"tree has no leaf {'/'.join(('bijector',) + path)}")
        out[ix.reshape(-1)] = np.broadcast_to(np.asarray(leaf), ix.shape).reshape(-1)
    return out


def blob_to_tree(program, blob) -> Dict[str, Any]:
    """Blob layout -> ``variables["params"]``-shaped tree."""
    return {"bijector": program.blob_to_variables(np.asarray(blob))["params"]}


def lower_mask(mask, program) -> np.ndarray:
    """optax's ``mask`` of add_decayed_weights (a tree of bools shaped like
    ``variables["params"]``, a leaf may be one bool; or a callable from the
    parameters to such a tree) -> one byte per blob entry."""
    if callable(mask):
        mask = mask(blob_to_tree(program, program.blob))
    return tree_to_blob(program, mask, np.uint8)
