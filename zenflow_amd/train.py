"""Training (zenflow.train, src/zenflow/train.py:18-138) on the GPU.

``loss_fn`` (train.py:64-72) is -mean(log_prob) of a train-mode forward —
ShiftBounds and BatchNorm on batch statistics — and ``step`` (:80-86) applies
its gradient with an optax-style (n)adamw update.  Both run in the library's
trainer (include/zenflow_amd.h, zf_trainer_*): the forward with stored
activations, the reverse pass through RQ splines, conditioner MLPs and
BatchNorm, and the optimiser, all on the device in the natural FLAX blob
layout.  ``metric_fn`` (:74-78) is the eval-mode log_prob of the fused
kernels.

Not reproducible offline (no JAX / optax here): jax.random's init and
permutation streams (seeded numpy generators stand in) and optax's exact
floating-point order; the optimiser restates optax's published update
(scale_by_adam with nesterov for nadamw -> add_decayed_weights -> scale by
-learning_rate), and any other chain of optax's transformations and schedules
comes from ``zenflow_amd.optim`` and runs on the device too.  Every gradient
element is checked against float64 autograd of the oracle's loss
(oracle/zf_oracle_torch.py,
tests/test_gpu_train.py::test_train_gradient_per_parameter)."""

from __future__ import annotations

import ctypes as ct
import warnings
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np

from . import _lib as L
from ._lib import DeviceArray, check
from .dist import shard_rows
from .optim import Chain, blob_to_tree, lower_mask, tree_to_blob
from .random import PRNGKey


@dataclass
class Optimizer:
    """optax.adamw / optax.nadamw hyper-parameters (optax defaults)."""

    learning_rate: float = 1e-3
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-8
    weight_decay: float = 1e-4
    nesterov: bool = True

    def desc(self) -> L.ZfOptimDesc:
        return L.ZfOptimDesc(self.learning_rate, self.b1, self.b2, self.eps, self.weight_decay,
                             1 if self.nesterov else 0)


def nadamw(learning_rate: float = 1e-3, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8,
           weight_decay: float = 1e-4) -> Optimizer:
    return Optimizer(learning_rate, b1, b2, eps, weight_decay, True)


def adamw(learning_rate: float = 1e-3, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8,
          weight_decay: float = 1e-4) -> Optimizer:
    return Optimizer(learning_rate, b1, b2, eps, weight_decay, False)


# |sum(lp)| from which the fp32 sum of the reference's jnp.mean is infinite
_F32_SUM_LIMIT = float(np.finfo(np.float32).max)

DEFAULT_OPTIMIZER = nadamw  # train.py:13-16 (optax.nadamw when available)


def _ptr(a: Optional[DeviceArray]) -> Optional[int]:
    return None if a is None else a.ptr


class Trainer:
    """Device-resident training state of one Flow: natural blob (params +
    batch statistics), gradient, optimiser moments, activation arena for
    batches of up to ``batch_max`` rows."""

    def __init__(self, flow, variables: Dict[str, Any], D: int, C: int, batch_max: int,
                 optimizer: Union[Optimizer, Chain, None] = None, comm=None):
        """``optimizer``: an :class:`Optimizer` ((n)adamw at a constant
        learning rate) or a chain of ``zenflow_amd.optim`` (clipping,
        schedules, sgd, adam, lion ...), run on the device either way.

        ``comm``: data parallelism — an object with ``rank``, ``world`` and
        ``trainer_comm_desc()`` (``dist.RcclCommunicator``, or
        ``dist.HostAllgather`` for ranks sharing a GPU); each rank then passes
        its shard of every global batch."""
        L.ensure_device()
        self.flow = flow
        self.D, self.C = int(D), int(C)
        self.batch_max = int(batch_max)
        self.optimizer = optimizer or DEFAULT_OPTIMIZER()
        self._open(flow._program(variables, self.D, self.C), comm)

    @classmethod
    def for_program(cls, program, batch_max: int) -> "Trainer":
        """A trainer on an existing device program's blob (the handle behind
        ``Flow.log_prob_and_grad``; it keeps no reference to the program)."""
        self = cls.__new__(cls)
        self.flow = None
        self.D, self.C = program.D, program.C
        self.batch_max = int(batch_max)
        self.optimizer = DEFAULT_OPTIMIZER()
        self._open(program, None, keep_program=False)
        return self

    def _open(self, prog, comm, keep_program: bool = True):
        self.program = prog if keep_program else None
        chain = self.optimizer if isinstance(self.optimizer, Chain) else None
        lowered = dmask = None
        if chain is not None:  # rejected chains raise here, before any handle exists
            lowered = chain.lower()
            if chain.mask() is not None:
                dmask = np.ascontiguousarray(lower_mask(chain.mask(), prog), np.uint8)
        opt = (DEFAULT_OPTIMIZER() if chain is not None else self.optimizer).desc()
        h = ct.c_void_p()
        check(L.load_library().zf_trainer_create(
            ct.byref(prog.desc), prog.blob.ctypes.data, prog.blob.size, prog.param_mask.ctypes.data,
            self.batch_max, ct.byref(opt), ct.byref(h)), "zf_trainer_create")
        self.handle = h.value
        if chain is not None:
            rc = L.load_library().zf_trainer_set_optim_chain(
                self.handle, ct.byref(lowered), None if dmask is None else dmask.ctypes.data)
            if rc:
                L.load_library().zf_trainer_destroy(ct.c_void_p(self.handle))
                self.handle = None
                check(rc, "zf_trainer_set_optim_chain")
        self._loss = DeviceArray((1,), np.float64)
        self.comm = comm
        self.world = 1
        if comm is not None and comm.world > 1:
            self._comm_desc = comm.trainer_comm_desc()  # kept alive: the C side holds its pointers
            check(L.load_library().zf_trainer_set_comm(self.handle, ct.byref(self._comm_desc)), "zf_trainer_set_comm")
            self.world = comm.world

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and L._lib is not None:
            L._lib.zf_trainer_destroy(ct.c_void_p(h))
            self.handle = None

    def _dev(self, x, cols):
        if x is None:
            return None
        if isinstance(x, DeviceArray):
            return x
        a = np.asarray(x, np.float32)
        if a.ndim == 1:
            a = a.reshape(-1, 1)
        return DeviceArray.from_numpy(np.ascontiguousarray(a))

    def _global(self, rows: int, global_rows: Optional[int]) -> int:
        return int(global_rows) if global_rows is not None else int(rows) * self.world

    def _weights(self, w, rows: int, name: str = "w") -> DeviceArray:
        """This rank's ``rows`` weights (or cotangents) on the device.  A host
        array is checked (shape, finiteness); a DeviceArray is taken as it
        is, size apart."""
        if isinstance(w, DeviceArray):
            if int(np.prod(w.shape)) != rows or w.dtype != np.float32:
                raise ValueError(f"{name} must hold {rows} float32 entries, got {w.dtype} {w.shape}")
            return w
        return DeviceArray.from_numpy(check_weights(w, rows, name))

    def loss_grad(self, x, c=None, update_stats: bool = False,
                  global_rows: Optional[int] = None, cond_grad: bool = False, w=None):
        """(loss, gradient in the natural blob layout) — loss_fn + jax.grad.
        Data parallel: ``x`` is this rank's shard of a global batch of
        ``global_rows`` rows (default: equal shards); both results are global.

        ``cond_grad=True`` returns ``(loss, grad, gc)`` with ``gc`` (rows, C) =
        d loss / d c of this rank's rows — what ``jax.grad(loss_fn_2)`` of
        examples/deep_set.ipynb sends back into ``phi`` through
        ``c = phi(x)``; a DeviceArray when ``c`` was one.  loss and grad have
        the same bits either way.

        ``w`` (rows,), a host array or a DeviceArray: per-sample weights of
        this rank's rows; the loss is ``-sum(w * lp) / sum(w)`` over the global
        batch (weights may be zero or negative, their sum must be positive).
        The batch statistics stay unweighted: the weights enter at the loss
        only."""
        xd, cd = self._dev(x, self.D), self._dev(c, self.C)
        g = DeviceArray((self.program.blob.size,))
        rows = xd.shape[0]
        wd = None if w is None else self._weights(w, rows)
        gc = self._gc_out(rows) if cond_grad else None
        self._call_loss_grad(xd.ptr, _ptr(cd), _ptr(wd), rows, self._global(rows, global_rows), update_stats, g.ptr,
                             _ptr(gc))
        loss = self._fp32_mean(float(self._loss.numpy()[0]))
        if cond_grad:
            return loss, g.numpy(), self._gc_like(gc, c)
        return loss, g.numpy()

    def _call_loss_grad(self, xptr, cptr, wptr, rows, global_rows, update_stats, gptr, gcptr) -> None:
        """The one loss_grad call (``wptr`` / ``gcptr`` None: unweighted / no gc)."""
        check(L.load_library().zf_trainer_loss_grad_weighted_shard(
            self.handle, xptr, cptr, wptr, rows, global_rows, 1 if update_stats else 0, self._loss.ptr, gptr, gcptr,
            L.stream()), "zf_trainer_loss_grad")
        self._last_rows = None if wptr is not None else global_rows

    def _call_step(self, xptr, cptr, wptr, rows, global_rows, gcptr) -> None:
        """The one step call (async); a weighted loss is the device's fp64
        value as is (``_last_rows`` None, see :meth:`_fp32_mean`)."""
        check(L.load_library().zf_trainer_step_weighted_shard(
            self.handle, xptr, cptr, wptr, rows, global_rows, self._loss.ptr, gcptr, L.stream()), "zf_trainer_step")
        self._last_rows = None if wptr is not None else global_rows

    @staticmethod
    def _gc_like(gc: DeviceArray, c):
        return gc if isinstance(c, DeviceArray) else gc.numpy()

    def _gc_out(self, rows: int) -> DeviceArray:
        if self.C == 0:
            raise ValueError("cond_grad=True needs a conditional flow (C > 0)")
        return DeviceArray((rows, self.C))

    def grad_tree(self, grad_blob: np.ndarray) -> Dict[str, Any]:
        """Gradient blob -> FLAX ``params`` tree (like jax.grad's output)."""
        return {"bijector": self.program.blob_to_variables(grad_blob)["params"]}

    def step(self, x, c=None, global_rows: Optional[int] = None, cond_grad: bool = False, w=None):
        """One optimiser step (train.py:80-86).  ``cond_grad=True`` returns
        ``gc`` (rows, C) = d loss / d c of the loss this step descended (a
        DeviceArray when ``c`` was one); the stepped parameters have the same
        bits either way.  ``w``: per-sample weights, as in :meth:`loss_grad`."""
        xd, cd = self._dev(x, self.D), self._dev(c, self.C)
        rows = xd.shape[0]
        wd = None if w is None else self._weights(w, rows)
        gc = self._gc_out(rows) if cond_grad else None
        self._call_step(xd.ptr, _ptr(cd), _ptr(wd), rows, self._global(rows, global_rows), _ptr(gc))
        return self._gc_like(gc, c) if cond_grad else None

    def log_prob_vjp(self, x: DeviceArray, c: Optional[DeviceArray] = None, cotangent: Optional[DeviceArray] = None):
        """Eval-mode ``(log_prob, dx, dc)`` at the trainer's current
        parameters and statistics (zf_trainer_log_prob_vjp): device in,
        device out; ``dc`` is None for an unconditional flow."""
        N = x.shape[0]
        if x.ndim != 2 or x.shape[1] != self.D:
            raise ValueError(f"x must have shape (N, {self.D}), got {x.shape}")
        if self.C and (c is None or c.shape != (N, self.C)):
            raise ValueError(f"this flow is conditional: c must have shape ({N}, {self.C})")
        if cotangent is not None and int(np.prod(cotangent.shape)) != N:
            raise ValueError(f"cotangent must have {N} entries, got shape {cotangent.shape}")
        lp, dx = DeviceArray((N,)), DeviceArray((N, self.D))
        dc = DeviceArray((N, self.C)) if self.C else None
        check(L.load_library().zf_trainer_log_prob_vjp(
            self.handle, x.ptr, c.ptr if self.C else None, None if cotangent is None else cotangent.ptr, lp.ptr,
            dx.ptr, None if dc is None else dc.ptr, N, L.stream()), "zf_trainer_log_prob_vjp")
        return lp, dx, dc

    # ---- custom losses: the user's loss between a forward and a backward ----
    def forward(self, x, c=None, *, train: bool = True, update_stats: Optional[bool] = None,
                global_rows: Optional[int] = None):
        """Per-row ``log_prob`` (rows,) float32 of ``flow.apply(..., train=train)``
        at the trainer's parameters, with the activations kept for one
        :meth:`backward` (zf_trainer_forward).  Any loss of these values is
        then the caller's own code, as with the reference (train.py:64-86):

            lp = tr.forward(x, c)
            g = tr.backward(dloss_dlp(lp))
            tr.apply_gradient(g)

        ``train=True``: batch statistics, and the running statistics are
        updated when ``update_stats`` (default: ``train``).  ``train=False``:
        the stored statistics, nothing updated.  Host arrays in give a host
        array out, a DeviceArray ``x`` a DeviceArray.  Data parallel: ``x`` is
        this rank's shard of ``global_rows`` rows, as in :meth:`loss_grad`."""
        train = bool(train)
        update_stats = train if update_stats is None else bool(update_stats)
        if update_stats and not train:
            raise ValueError("update_stats=True needs train=True: eval mode reads the stored statistics")
        xd, cd = self._dev(x, self.D), self._dev(c, self.C)
        rows = xd.shape[0]
        if rows > self.batch_max:
            raise ValueError(f"forward takes at most batch_max = {self.batch_max} rows, got {rows}: "
                             "micro-batch and accumulate the gradients")
        lp = DeviceArray((rows,))
        self._pending_rows = None
        check(L.load_library().zf_trainer_forward(
            self.handle, xd.ptr, _ptr(cd), rows, self._global(rows, global_rows), 1 if train else 0,
            1 if update_stats else 0, lp.ptr, L.stream()), "zf_trainer_forward")
        self._pending_rows = rows
        self._pending_device = isinstance(x, DeviceArray)
        return lp if isinstance(x, DeviceArray) else lp.numpy()

    def backward(self, cotangent, *, cond_grad: bool = False):
        """The gradient, in the natural blob layout, of
        ``sum_b cotangent[b] * lp[b]`` over the global batch of the pending
        :meth:`forward` — with ``cotangent = d loss / d lp`` the gradient of
        the caller's loss (zf_trainer_backward; :meth:`grad_tree` turns it
        into a FLAX tree).  ``cotangent`` (rows,): a host array, checked like
        :func:`check_weights` before any device call, or a float32 DeviceArray.
        ``cond_grad=True`` returns ``(g, gc)`` with ``gc`` (rows, C) the same
        sum's gradient with respect to ``c``.  The results are DeviceArrays
        when ``forward`` was given one.  Rows whose ``lp`` is not finite
        contribute zeros.  One backward per forward: ``ValueError`` without a
        pending one."""
        rows = getattr(self, "_pending_rows", None)
        if rows is None:
            raise ValueError("backward needs a pending forward (one backward per forward; step, loss_grad, "
                             "log_prob_vjp and apply_gradient drop it)")
        cot = self._weights(cotangent, rows, "cotangent")
        gc = self._gc_out(rows) if cond_grad else None
        g = DeviceArray((self.program.blob.size,))
        self._pending_rows = None
        rc = L.load_library().zf_trainer_backward(self.handle, cot.ptr, g.ptr, _ptr(gc), L.stream())
        if rc and "no forward pending" in L.load_library().zf_last_error().decode():
            raise ValueError("backward needs a pending forward: another trainer call dropped it")
        check(rc, "zf_trainer_backward")
        self._last_grad = g
        dev = self._pending_device
        if cond_grad:
            return (g, gc) if dev else (g.numpy(), gc.numpy())
        return g if dev else g.numpy()

    def apply_gradient(self, g=None) -> None:
        """The optimiser update of :meth:`step` on a given gradient
        (zf_trainer_apply_gradient): ``g`` a blob-layout host array or
        DeviceArray, a FLAX ``params`` tree as :meth:`grad_tree` returns it
        (edited, summed over micro-batches ...), or None for the gradient of
        the last :meth:`backward`.  Data parallel: every rank passes the same
        gradient, which is what ``backward`` returns."""
        n = self.program.blob.size
        if g is None:
            gd = getattr(self, "_last_grad", None)
            if gd is None:
                raise ValueError("apply_gradient() without a gradient needs an earlier backward")
        elif isinstance(g, DeviceArray):
            gd = g
        else:
            if isinstance(g, dict):
                g = tree_to_blob(self.program, g, np.float32)
            gd = DeviceArray.from_numpy(np.ascontiguousarray(np.asarray(g, np.float32).reshape(-1)))
        if int(np.prod(gd.shape)) != n or gd.dtype != np.float32:
            raise ValueError(f"the gradient must hold {n} float32 entries (blob layout), got {gd.dtype} {gd.shape}")
        self._pending_rows = None
        check(L.load_library().zf_trainer_apply_gradient(self.handle, gd.ptr, L.stream()),
              "zf_trainer_apply_gradient")

    # ---- gradients through sampling: a loss of the samples, not of log_prob ----
    def sample_forward(self, conditions_or_size, *, seed: int = 0, z=None, global_rows: Optional[int] = None):
        """``(x, log_q)``: the samples ``x = bijector.inverse(z, c)`` (rows, D)
        of ``Flow.sample`` (flow.py:50-78; eval mode, stored statistics) at the
        trainer's parameters and their log-density ``log_q`` (rows,) under the
        flow — the latent's log_prob of ``z`` plus every op's forward log-det
        at the inverse's own intermediates — with the activations kept for
        one :meth:`sample_backward` (zf_trainer_sample_forward).  A reverse-KL
        fit to a target density ``log_p`` is three calls:

            x, log_q = tr.sample_forward(n, seed=step)
            g = tr.sample_backward(-dlogp_dx(x) / n, np.full(n, 1 / n, np.float32))
            tr.apply_gradient(g)

        ``conditions_or_size``: the conditions ``c`` (rows, C) or, for an
        unconditional flow, the number of rows.  ``z=None`` draws
        ``flow.latent.sample(rows, PRNGKey(seed))`` on the device, the bits
        ``Flow.sample(..., seed=seed)`` starts from; else ``z`` (rows, D) is a
        host array or a DeviceArray.  Host arrays in give host arrays out, a
        DeviceArray ``c`` or ``z`` DeviceArrays.  ``log_q`` is not finite
        where the latent's density of ``z`` is not; such rows count for
        nothing in :meth:`sample_backward`.  Data parallel: the rows are this
        rank's shard of ``global_rows`` rows, as in :meth:`forward`."""
        if isinstance(conditions_or_size, (int, np.integer)):
            rows, c = int(conditions_or_size), None
        else:
            c = conditions_or_size
            rows = int(c.shape[0])
        if self.C and c is None:
            raise ValueError(f"this flow is conditional: pass the conditions (rows, {self.C}), not a size")
        if not self.C and c is not None:
            raise ValueError("this flow is unconditional: pass the number of rows")
        if rows < 1 or rows > self.batch_max:
            raise ValueError(f"sample_forward takes 1 to batch_max = {self.batch_max} rows, got {rows}: "
                             "micro-batch and accumulate the gradients")
        cd = self._dev(c, self.C)
        if cd is not None and tuple(cd.shape) != (rows, self.C):
            raise ValueError(f"conditions must have shape ({rows}, {self.C}), got {tuple(cd.shape)}")
        if z is None:
            zd = self._latent_draw(rows, seed)
        else:
            zd = self._dev(z, self.D)
            if tuple(zd.shape) != (rows, self.D) or zd.dtype != np.float32:
                raise ValueError(f"z must hold ({rows}, {self.D}) float32 entries, got {zd.dtype} {tuple(zd.shape)}")
        x, lq = DeviceArray((rows, self.D)), DeviceArray((rows,))
        self._pending_rows = None
        self._pending_sample = None
        check(L.load_library().zf_trainer_sample_forward(
            self.handle, zd.ptr, _ptr(cd), rows, self._global(rows, global_rows), x.ptr, lq.ptr, L.stream()),
            "zf_trainer_sample_forward")
        self._pending_sample = rows
        self._pending_device = isinstance(c, DeviceArray) or isinstance(z, DeviceArray)
        return (x, lq) if self._pending_device else (x.numpy(), lq.numpy())

    def _latent_draw(self, rows: int, seed: int) -> DeviceArray:
        """``flow.latent.sample(rows, PRNGKey(seed))``, left on the device."""
        from .engine import _latent_code
        from .random import key_to_seed

        if self.flow is None:
            raise ValueError("sample_forward(z=None) needs the trainer's flow for its latent: pass z")
        code, param = _latent_code(self.flow.latent)
        z = DeviceArray((rows, self.D))
        check(L.load_library().zf_latent_sample(code, param, key_to_seed(PRNGKey(seed)), z.ptr, rows, self.D,
                                                L.stream()), "zf_latent_sample")
        return z

    def sample_backward(self, gx, glog_q=None, *, cond_grad: bool = False, latent_grad: bool = False):
        """The gradient, in the natural blob layout, of
        ``sum_b gx[b] . x[b] + glog_q[b] * log_q[b]`` over the global batch of
        the pending :meth:`sample_forward` — with ``gx = d loss / d x`` and
        ``glog_q = d loss / d log_q`` the gradient of the caller's loss of the
        samples (zf_trainer_sample_backward; :meth:`grad_tree` and
        :meth:`apply_gradient` take it unchanged).  ``gx`` (rows, D) and
        ``glog_q`` (rows,), None for zeros: host arrays, checked for shape and
        finiteness before any device call, or float32 DeviceArrays.
        ``cond_grad=True`` / ``latent_grad=True`` also return the same sum's
        gradient with respect to ``c`` (rows, C) / ``z`` (rows, D), in that
        order after ``g``.  The results are DeviceArrays when
        ``sample_forward`` was given one.  Rows whose ``x`` or ``log_q`` is
        not finite contribute zeros and get zero ``gc`` / ``gz`` rows.  One
        backward per forward: ``ValueError`` without a pending one."""
        rows = getattr(self, "_pending_sample", None)
        if rows is None:
            raise ValueError("sample_backward needs a pending sample_forward (one backward per forward; forward, "
                             "step, loss_grad, log_prob_vjp and apply_gradient drop it)")
        if isinstance(gx, DeviceArray):
            if int(np.prod(gx.shape)) != rows * self.D or gx.dtype != np.float32:
                raise ValueError(f"gx must hold ({rows}, {self.D}) float32 entries, got {gx.dtype} {gx.shape}")
            gxd = gx
        else:
            a = np.asarray(gx)
            if a.shape != (rows, self.D):
                raise ValueError(f"gx must have shape ({rows}, {self.D}), got {a.shape}")
            a = np.ascontiguousarray(a, np.float32)
            if not np.isfinite(a).all():
                raise ValueError(f"gx holds {int((~np.isfinite(a)).sum())} non-finite values")
            gxd = DeviceArray.from_numpy(a)
        gl = None if glog_q is None else self._weights(glog_q, rows, "glog_q")
        gc = self._gc_out(rows) if cond_grad else None
        gz = DeviceArray((rows, self.D)) if latent_grad else None
        g = DeviceArray((self.program.blob.size,))
        self._pending_sample = None
        rc = L.load_library().zf_trainer_sample_backward(self.handle, gxd.ptr, _ptr(gl), g.ptr, _ptr(gz), _ptr(gc),
                                                         L.stream())
        if rc and "no forward pending" in L.load_library().zf_last_error().decode():
            raise ValueError("sample_backward needs a pending sample_forward: another trainer call dropped it")
        check(rc, "zf_trainer_sample_backward")
        self._last_grad = g
        out = [g] + ([gc] if cond_grad else []) + ([gz] if latent_grad else [])
        if not self._pending_device:
            out = [o.numpy() for o in out]
        return out[0] if len(out) == 1 else tuple(out)

    def _step_rows(self, xptr: int, cptr: Optional[int], rows: int, global_rows: Optional[int] = None,
                   wptr: Optional[int] = None) -> None:
        """One step on ``rows`` device-resident rows (raw pointers; async);
        ``wptr``: their weights (the weighted loss)."""
        self._call_step(xptr, cptr, wptr, rows, self._global(rows, global_rows), None)

    def _step_local(self, xptr: int, cptr: Optional[int], rows: int, wptr: Optional[int] = None) -> None:
        """One step on the whole batch without the cross-rank reductions:
        every rank holds the same batch, so each computes the one-device
        step itself (a batch with fewer rows than ranks)."""
        lib = L.load_library()
        if self.world > 1:
            check(lib.zf_trainer_set_comm(self.handle, None), "zf_trainer_set_comm")
        try:
            self._call_step(xptr, cptr, wptr, rows, rows, None)
        finally:
            if self.world > 1:
                check(lib.zf_trainer_set_comm(self.handle, ct.byref(self._comm_desc)), "zf_trainer_set_comm")

    def last_loss(self) -> float:
        return self._fp32_mean(float(self._loss.numpy()[0]))

    def _fp32_mean(self, loss: float) -> float:
        """The device loss is -sum(lp / B) in fp64; the reference's loss_fn
        (train.py:70-72) is jnp.mean in fp32, whose sum overflows to +-inf once
        |sum(lp)| leaves the fp32 range (two rows at finfo.min) — the same rule
        as dist.nll_from_sum, applied to the global batch of the last call.
        A weighted loss (``_last_rows`` None) is returned as it is."""
        from .dist import nll_from_sum

        B = getattr(self, "_last_rows", None)
        if B is None or loss != loss:
            return loss
        return nll_from_sum(-loss * B, B) if abs(loss * B) >= _F32_SUM_LIMIT else loss

    def variables(self) -> Dict[str, Any]:
        blob = np.empty_like(self.program.blob)
        check(L.load_library().zf_trainer_get_blob(self.handle, blob.ctypes.data), "zf_trainer_get_blob")
        v = self.program.blob_to_variables(blob)
        return {"params": {"bijector": v["params"]}, "batch_stats": {"bijector": v["batch_stats"]}}

    def _n_slots(self) -> int:
        return self.optimizer.n_slots if isinstance(self.optimizer, Chain) else 2

    def opt_state(self) -> Dict[str, Any]:
        """The optimiser's state (optax's ``opt_state``): ``count`` (updates
        applied), the ``learning_rate`` and ``grad_norm`` the last step used
        (grad_norm NaN without clip_by_global_norm), and ``slots``, the moment
        arrays as ``params``-shaped trees in chain order (scale_by_adam: mu,
        nu; scale_by_lion: mu; trace: trace; an :class:`Optimizer`: m, v).
        With :meth:`variables` it is all a run needs to resume."""
        lib = L.load_library()
        count, lr, gn = ct.c_int64(), ct.c_double(), ct.c_double()
        check(lib.zf_trainer_get_opt_scalars(self.handle, ct.byref(count), ct.byref(lr), ct.byref(gn)),
              "zf_trainer_get_opt_scalars")
        slots = []
        for k in range(self._n_slots()):
            blob = np.empty(self.program.blob.size, np.float32)
            check(lib.zf_trainer_get_opt_slot(self.handle, k, blob.ctypes.data), "zf_trainer_get_opt_slot")
            slots.append(blob_to_tree(self.program, blob))
        return {"count": int(count.value), "learning_rate": float(lr.value), "grad_norm": float(gn.value),
                "slots": slots}

    def load_opt_state(self, state: Dict[str, Any]) -> None:
        """Restore what :meth:`opt_state` returned (of a trainer with the
        same optimiser): the moments and the step counter, from which the
        bias corrections and the schedule follow."""
        lib = L.load_library()
        slots = list(state["slots"])
        if len(slots) != self._n_slots():
            raise ValueError(f"state has {len(slots)} moment arrays, this optimiser keeps {self._n_slots()}")
        for k, tree in enumerate(slots):
            blob = np.ascontiguousarray(tree_to_blob(self.program, tree, np.float32))
            check(lib.zf_trainer_set_opt_slot(self.handle, k, blob.ctypes.data), "zf_trainer_set_opt_slot")
        check(lib.zf_trainer_set_opt_count(self.handle, int(state["count"])), "zf_trainer_set_opt_count")


def check_weights(w, rows: int, name: str) -> np.ndarray:
    """``w`` as a contiguous float32 array of shape (rows,), all finite
    (ValueError otherwise); zero and negative weights are allowed."""
    a = np.asarray(w)
    if a.shape != (rows,):
        raise ValueError(f"{name} must have shape ({rows},), got {a.shape}")
    a = np.ascontiguousarray(a, np.float32)
    if not np.isfinite(a).all():
        raise ValueError(f"{name} holds {int((~np.isfinite(a)).sum())} non-finite values")
    return a


def weighted_nll(lp, w) -> float:
    """-sum(w * lp) / sum(w) in fp64: the weighted metric."""
    lp = np.asarray(lp, np.float64)
    w = np.asarray(w, np.float64)
    return float(-(w * lp).sum() / w.sum())


def _metric(flow, variables, x, c, w=None) -> float:
    """metric_fn (train.py:74-78): -mean(log_prob), eval mode; with weights
    ``w`` the weighted mean :func:`weighted_nll`."""
    from .dist import nll_from_sum

    lp = np.asarray(flow.apply(variables, x, c), np.float64)
    if w is not None:
        return weighted_nll(lp, w)
    return nll_from_sum(lp.sum(), lp.shape[0])


def train(
    flow,
    X_train,
    X_test,
    C_train=None,
    C_test=None,
    *,
    epochs: int = 1000,
    batch_size: int = 1024,
    optimizer: Union[Optimizer, Chain, None] = None,
    patience: float = 0.05,
    warmup: float = 0.2,
    seed: int = 0,
    progress: bool = True,
    initial_variables=None,
    comm=None,
    W_train=None,
    W_test=None,
) -> Tuple[Dict[str, Any], int, List[float], List[float]]:
    """Trains the normalizing flow on the provided inputs (train.py:18-138).

    Same arguments, defaults, early stopping and return value
    ``(best_variables, best_epoch, loss_train, loss_test)`` as the reference;
    ``optimizer`` is an :class:`Optimizer` (``nadamw(...)`` / ``adamw(...)``)
    or a chain of ``zenflow_amd.optim`` (``optim.chain(optim.clip_by_global_norm(1.0),
    optim.adamw(optim.warmup_cosine_decay_schedule(...)))``), where the
    reference takes an ``optax.GradientTransformation``.

    ``comm`` (data parallelism, one process per GPU, every rank calling with
    the same data and seed): each global batch of ``batch_size`` rows is cut
    into contiguous per-rank shards (``dist.shard_rows``); the trainer's
    reductions make every rank's parameters identical after every step, and
    equal to one device's when every batch splits evenly.  A batch with fewer
    rows than ranks is stepped by every rank on the whole batch, without
    reductions (the one-device step).

    ``W_train`` (n_train,), ``W_test`` (n_test,): per-sample weights — event
    weights, sWeights, importance or class-balance weights.  With the
    reference this is the user's own ``loss_fn``, ``-(w * lp).sum() / w.sum()``;
    here every step descends that loss of its batch (``Trainer.step(w=...)``:
    the batch statistics stay unweighted), ``loss_train`` is the weighted
    metric of the last batch, and ``loss_test`` is weighted by ``W_test``
    when given.  Weights may be zero or negative; every batch's weights must
    sum to a positive number (checked per epoch, ``ValueError``)."""
    if warmup < 1:
        warmup = warmup * epochs
    warmup = int(warmup)
    if patience < 1:
        patience = patience * epochs
    patience = int(patience)

    X_train = np.asarray(X_train, np.float32)
    X_test = np.asarray(X_test, np.float32)
    C_train = None if C_train is None else np.asarray(C_train, np.float32)
    C_test = None if C_test is None else np.asarray(C_test, np.float32)
    if C_train is not None and C_train.ndim == 1:
        C_train = C_train.reshape(-1, 1)
    if C_test is not None and C_test.ndim == 1:
        C_test = C_test.reshape(-1, 1)
    # the weights are checked before any device call
    if W_train is not None:
        W_train = check_weights(W_train, X_train.shape[0], "W_train")
    if W_test is not None:
        W_test = check_weights(W_test, X_test.shape[0], "W_test")
        if not W_test.astype(np.float64).sum() > 0:
            raise ValueError("W_test must sum to a positive number")

    if initial_variables is None:
        variables = flow.init(PRNGKey(seed), X_train[:1], None if C_train is None else C_train[:1])
    else:
        variables = initial_variables
    D = X_train.shape[1]
    Cd = 0 if C_train is None else C_train.shape[1]
    world = 1 if comm is None else int(comm.world)
    rank = 0 if comm is None else int(comm.rank)
    shard_max = -(-min(batch_size, X_train.shape[0]) // world)
    trainer = Trainer(flow, variables, D, Cd, shard_max, optimizer, comm=comm)

    loop = range(epochs)
    if progress:
        try:
            from tqdm import tqdm

            loop = tqdm(loop)
        except ModuleNotFoundError:  # pragma: no cover
            pass

    loss_train: List[float] = []
    loss_test: List[float] = []
    best_epoch = 0
    best_variables = variables
    X = C = None
    n = X_train.shape[0]
    for epoch in loop:
        perm = np.random.default_rng([seed, epoch]).permutation(n)
        X_perm = X_train[perm]
        C_perm = None if C_train is None else C_train[perm]
        W_perm = None if W_train is None else W_train[perm]
        if W_perm is not None:
            sums = np.add.reduceat(W_perm.astype(np.float64), np.arange(0, n, batch_size))
            if not (sums > 0).all():
                k = int(np.argmin(sums > 0))
                raise ValueError(f"epoch {epoch}: the weights of batch {k} sum to {sums[k]:.6g}, not a positive number")
        # one upload per epoch; batches are row ranges of the resident copy
        X_dev = DeviceArray.from_numpy(X_perm)
        C_dev = None if C_perm is None else DeviceArray.from_numpy(C_perm)
        W_dev = None if W_perm is None else DeviceArray.from_numpy(W_perm)
        for batch_idx in range(0, n, batch_size):
            rows = min(batch_size, n - batch_idx)
            if rows < world:
                trainer._step_local(X_dev.ptr + batch_idx * D * 4,
                                    None if C_dev is None else C_dev.ptr + batch_idx * Cd * 4, rows,
                                    None if W_dev is None else W_dev.ptr + batch_idx * 4)
                continue
            if rows % world and epoch == 0:
                warnings.warn(f"batch of {rows} rows does not split evenly over {world} ranks: ranks stay "
                              "identical but their fp64 reduction order differs from one device's", RuntimeWarning)
            lo, hi = shard_rows(rows, rank, world)
            trainer._step_rows(X_dev.ptr + (batch_idx + lo) * D * 4,
                               None if C_dev is None else C_dev.ptr + (batch_idx + lo) * Cd * 4, hi - lo, rows,
                               None if W_dev is None else W_dev.ptr + (batch_idx + lo) * 4)
        X = X_perm[batch_idx : batch_idx + batch_size]
        C = None if C_perm is None else C_perm[batch_idx : batch_idx + batch_size]
        W = None if W_perm is None else W_perm[batch_idx : batch_idx + batch_size]

        variables = trainer.variables()
        loss_train.append(_metric(flow, variables, X, C, W))  # last batch, as train.py:122
        loss_test.append(_metric(flow, variables, X_test, C_test, W_test))

        if not np.isfinite(loss_train[-1]):
            warnings.warn(f"epoch {epoch}: loss[train] not finite, abort training", RuntimeWarning)
            break

        if loss_test[-1] <= loss_test[best_epoch]:
            best_epoch = epoch
            best_variables = variables

        if epoch >= warmup and epoch >= 2 * patience and epoch % patience == 0:
            if not np.min(loss_test[-patience:]) < np.min(loss_test[-2 * patience : -patience]):
                break
    return best_variables, best_epoch, loss_train, loss_test


# ---------------------------------------------------------------------------
# Deep-set flows: ragged minibatches of a resident data set
# ---------------------------------------------------------------------------


def plan_set_batches(offsets, batch_sets: int, world: int = 1) -> Tuple[List[int], int, int]:
    """``(sizes, sets_max, rows_max)`` of an epoch of :func:`train_sets` over
    the S sets of ``offsets`` (S + 1, validated): the sets per batch
    (``batch_sets``, the last one ``S % batch_sets`` when that is not 0), and
    the capacities of one rank's trainers — a rank's shard of a batch has at
    most ``sets_max = ceil(min(batch_sets, S) / world)`` sets
    (``dist.shard_rows``), and no ``sets_max`` sets have more element rows
    than the ``sets_max`` longest ones, ``rows_max`` (at least 1): bounds no
    batch of no permutation exceeds, so nothing is re-created during a run.

    ValueError: ``batch_sets < 1``; a batch with fewer sets than ranks; and
    empty sets enough to fill the smallest shard (a shard without an element
    row is rejected up front, not handled)."""
    from .nn import check_offsets

    off = check_offsets(offsets, np.iinfo(np.int64).max)
    S, batch_sets, world = off.size - 1, int(batch_sets), int(world)
    if batch_sets < 1:
        raise ValueError(f"batch_sets must be at least 1, got {batch_sets}")
    if world < 1:
        raise ValueError(f"world must be at least 1, got {world}")
    if S < 1:
        raise ValueError("train_sets needs at least one set")
    sizes = [min(batch_sets, S - k) for k in range(0, S, batch_sets)]
    if min(sizes) < world:
        raise ValueError(f"S = {S} sets in batches of batch_sets = {batch_sets} leave a batch of {min(sizes)} sets "
                         f"for world = {world} ranks: every batch needs at least one set per rank")
    lengths = np.diff(off)
    smallest = min(sizes) // world  # the fewest sets a rank's shard can have
    empty = int((lengths == 0).sum())
    if empty >= smallest:
        raise ValueError(f"{empty} empty sets could fill a rank's shard of {smallest} sets (S = {S}, batch_sets = "
                         f"{batch_sets}, world = {world}): a shard without element rows is not supported")
    sets_max = -(-sizes[0] // world)
    rows_max = max(1, int(np.sort(lengths)[::-1][:sets_max].sum()))
    return sizes, sets_max, rows_max


def _sets_arrays(X, offsets, Y, what: str):
    """One split's (X, offsets, Y) as float32 / int64 / float32 host arrays, checked."""
    from .nn import check_offsets

    X = np.asarray(X, np.float32)
    Y = np.asarray(Y, np.float32)
    if X.ndim != 2:
        raise ValueError(f"X_{what} must be 2-D (rows, in_dim), got {X.shape}")
    if Y.ndim != 2:
        raise ValueError(f"Y_{what} must be 2-D (sets, D), got {Y.shape}")
    off = check_offsets(offsets, X.shape[0])
    if Y.shape[0] != off.size - 1:
        raise ValueError(f"Y_{what} has {Y.shape[0]} rows for the {off.size - 1} sets of offsets_{what}")
    return np.ascontiguousarray(X), off, np.ascontiguousarray(Y)


def _metric_sets(flow, phi, variables, X, off, Y) -> float:
    """metric_fn of a deep-set flow, through the modules: ``c = phi(x)`` in
    eval mode, then the float64 NLL of ``flow.apply(fv, Y, c)``."""
    c = phi.apply(variables["phi"], X, off)
    return _metric(flow, variables["flow"], Y, c)


def train_sets(
    flow,
    phi,
    X_train,
    offsets_train,
    Y_train,
    X_test,
    offsets_test,
    Y_test,
    *,
    epochs: int = 1000,
    batch_sets: int = 1024,
    optimizer: Union[Optimizer, Chain, None] = None,
    phi_optimizer: Union[Optimizer, Chain, None] = None,
    patience: float = 0.05,
    warmup: float = 0.2,
    seed: int = 0,
    progress: bool = True,
    initial_variables=None,
    comm=None,
) -> Tuple[Dict[str, Any], int, List[float], List[float]]:
    """:func:`train` for a deep-set flow (examples/deep_set.ipynb,
    ``DeepSetFlow`` / ``loss_fn_2``): ``flow`` models ``Y`` (one row per set)
    under the condition ``c = phi(x)``, ``phi`` a pooled ``nn.ConditionNet``
    over the set's element rows ``X`` (``offsets``: the S + 1 CSR offsets),
    and both are trained jointly on random minibatches of ``batch_sets`` sets.
    Returns ``(best_variables, best_epoch, loss_train, loss_test)`` with
    ``variables = {"flow": ..., "phi": ...}``; epochs, permutation
    (``default_rng([seed, epoch])``), metrics (eval mode: the last batch, the
    test sets), ``best_epoch`` and the ``warmup`` / ``patience`` early stopping
    are :func:`train`'s.

    The training data is uploaded once and stays resident; every batch is
    packed on the device (``nn.segment_take``, ``nn.take_rows``), so that a
    step is

        xb, ob = nn.segment_take(Xd, off_d, take_b, rows=rows_b)
        yb     = nn.take_rows(Yd, take_b)
        c      = ct.forward(xb, ob, seed=seed * 2**32 + step)
        gc     = tr.step(yb, c, cond_grad=True)
        ct.step(gc)

    with ``take_b`` the batch's slice of the epoch's permutation, ``rows_b``
    its element rows (from the host offsets) and ``step`` the optimiser steps
    taken so far.  One ``Trainer`` and one ``nn.ConditionTrainer`` serve the
    run, sized by :func:`plan_set_batches`.

    ``initial_variables=None``: the flow is initialised as :func:`train` does
    (with a zero ``(1, phi.features)`` condition), ``phi`` with
    ``phi.init(seed + 1, X_train, offsets_train)``.  ``optimizer`` /
    ``phi_optimizer``: the flow's / ``phi``'s, an :class:`Optimizer` or a
    ``zenflow_amd.optim`` chain each (default nadamw(1e-3)).

    ``comm`` (as :func:`train` takes it, every rank calling with the same data
    and seed): a batch's sets are cut contiguously over the ranks
    (``dist.shard_rows``), each rank gathers and passes its own sets
    (``global_rows`` / ``row_base`` of ``ConditionTrainer.forward``), and every
    rank evaluates the metrics on all of the data, so all ranks return
    identical results.  Their bits are not one device's: random ragged shards
    do not have equal element rows.

    Checked on the host before any device call (ValueError): shapes, offsets,
    one ``Y`` row per set, ``batch_sets >= 1``, a ``phi`` without pooling, a
    batch (the short last one included) with fewer sets than ranks, and
    enough empty sets to leave a rank's shard without an element row
    (rejected, not handled; see :func:`plan_set_batches`)."""
    from . import nn

    if warmup < 1:
        warmup = warmup * epochs
    warmup = int(warmup)
    if patience < 1:
        patience = patience * epochs
    patience = int(patience)

    if not isinstance(phi, nn.ConditionNet) or phi.pool is None:
        raise ValueError("phi must be a pooled nn.ConditionNet (pool='sum' or 'max'): one condition row per set")
    X_train, off_train, Y_train = _sets_arrays(X_train, offsets_train, Y_train, "train")
    X_test, off_test, Y_test = _sets_arrays(X_test, offsets_test, Y_test, "test")
    in_dim, D, Cd = X_train.shape[1], Y_train.shape[1], phi.features
    if X_test.shape[1] != in_dim or Y_test.shape[1] != D:
        raise ValueError(f"the test split has {X_test.shape[1]} element and {Y_test.shape[1]} target columns, the "
                         f"train split {in_dim} and {D}")
    world = 1 if comm is None else int(comm.world)
    rank = 0 if comm is None else int(comm.rank)
    sizes, sets_max, rows_max = plan_set_batches(off_train, batch_sets, world)
    batch_sets = int(batch_sets)
    S = off_train.size - 1

    if initial_variables is None:
        variables = {"flow": flow.init(PRNGKey(seed), Y_train[:1], np.zeros((1, Cd), np.float32)),
                     "phi": phi.init(seed + 1, X_train, off_train)}
    else:
        variables = initial_variables
    tr = Trainer(flow, variables["flow"], D, Cd, sets_max, optimizer, comm=comm)
    ct = nn.ConditionTrainer(phi, variables["phi"], in_dim, rows_max, sets_max=sets_max, optimizer=phi_optimizer,
                             comm=comm if world > 1 else None)
    Xd, off_d, Yd = DeviceArray.from_numpy(X_train), DeviceArray.from_numpy(off_train), DeviceArray.from_numpy(Y_train)
    Xt, off_t, Yt = DeviceArray.from_numpy(X_test), DeviceArray.from_numpy(off_test), DeviceArray.from_numpy(Y_test)
    lengths = np.diff(off_train)

    loop = range(epochs)
    if progress:
        try:
            from tqdm import tqdm

            loop = tqdm(loop)
        except ModuleNotFoundError:  # pragma: no cover
            pass

    loss_train: List[float] = []
    loss_test: List[float] = []
    best_epoch = 0
    best_variables = variables
    step = 0
    for epoch in loop:
        perm = np.random.default_rng([seed, epoch]).permutation(S)
        take_d = DeviceArray.from_numpy(perm.astype(np.int64))  # one upload per epoch
        first = 0
        for n in sizes:
            lo, hi = shard_rows(n, rank, world)
            len_b = lengths[perm[first : first + n]]
            take_b = take_d.rows(first + lo, first + hi)
            xb, ob = nn.segment_take(Xd, off_d, take_b, rows=int(len_b[lo:hi].sum()))
            yb = nn.take_rows(Yd, take_b)
            shard = {} if world == 1 else {"global_rows": int(len_b.sum()), "row_base": int(len_b[:lo].sum())}
            c = ct.forward(xb, ob, seed=seed * 2**32 + step, **shard)
            gc = tr.step(yb, c, global_rows=n, cond_grad=True)
            ct.step(gc)
            step += 1
            first += n
        # the last batch, all of it on every rank
        last = take_d.rows(S - sizes[-1], S)
        xb, ob = nn.segment_take(Xd, off_d, last, rows=int(lengths[perm[S - sizes[-1] :]].sum()))
        yb = nn.take_rows(Yd, last)

        variables = {"flow": tr.variables(), "phi": ct.variables()}
        loss_train.append(_metric_sets(flow, phi, variables, xb, ob, yb))  # last batch, as train.py:122
        loss_test.append(_metric_sets(flow, phi, variables, Xt, off_t, Yt))

        if not np.isfinite(loss_train[-1]):
            warnings.warn(f"epoch {epoch}: loss[train] not finite, abort training", RuntimeWarning)
            break

        if loss_test[-1] <= loss_test[best_epoch]:
            best_epoch = epoch
            best_variables = variables

        if epoch >= warmup and epoch >= 2 * patience and epoch % patience == 0:
            if not np.min(loss_test[-patience:]) < np.min(loss_test[-2 * patience : -patience]):
                break
    return best_variables, best_epoch, loss_train, loss_test
