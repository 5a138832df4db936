"""Conditioning networks on the device (include/zenflow_amd.h, zf_condnet_*).

examples/deep_set.ipynb trains a network ``Phi`` together with the flow: it
turns the elements of each set into the flow's condition,

    BatchNorm -> (Dense, act) x depth -> Dense -> Dropout -> sum over each set

(or, where a user of the reference edits that line of ``Phi.__call__`` to
``jnp.max``, the max over each set: ``pool="max"``)
(cells ``class NNBlock`` / ``class Phi`` / ``class DeepSetFlow`` /
``loss_fn_2``).  :class:`ConditionNet` is that network as a module of this
package's protocol, usable where the notebook puts ``Phi()``;
:class:`ConditionTrainer` holds it on the device for training next to a
``zenflow_amd.train.Trainer``:

    c  = ct.forward(Xd, off_d, seed=epoch)      # phi, train mode
    gc = tr.step(Yd, c, cond_grad=True)         # the flow's step, d loss / d c
    ct.step(gc)                                 # phi's gradient and update

with nothing leaving the device.  The sets are given in CSR form: ``offsets``
(S + 1 non-decreasing integers, set s owns the rows ``offsets[s]:offsets[s+1]``)
instead of the notebook's ``sum_matrix``.

The notebook's first half (``class DeepSet`` / ``loss_fn`` / ``step``) puts a
second network ``rho``, ``NNBlock(1, 3, 128)``, behind the pooled sum; it is
``ConditionNet(1, batch_norm=False, pool=None)``, and
``backward(gc, input_grad=True)`` sends its ``d loss / d x`` on as ``phi``'s
``gc``::

    c  = pt.forward(Xd, off_d, seed=epoch)      # phi
    yp = rt.forward(c)                          # rho
    pt.step(rt.step(gy, input_grad=True))       # gy = d loss / d yp

:func:`segment_repeat` is ``jnp.repeat(c, sizes, axis=0)`` of
``DeepSetFlow.sample`` on the device, :func:`segment_sum` its reverse;
:func:`segment_mean` and :func:`segment_max` are the other two poolings on
their own.  :func:`segment_take` packs the element rows of a minibatch of
sets out of a resident data set and :func:`take_rows` their per-set targets
(``zenflow_amd.train.train_sets`` is the loop over them).

No JAX is at hand here, so flax.linen's BatchNorm, Dense and Dropout are
restated from their published definitions, as the couplings' layers are;
``jax.random``'s dropout bits are not reproduced (the mask is
``u01(philox(seed, row, column)) >= rate``)."""

from __future__ import annotations

import ctypes as ct
from collections import OrderedDict
from typing import Any, Callable, Dict, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib as L
from ._lib import DeviceArray, check
from .activations import act_code, swish
from .module import Module, lecun_normal, scope_for
from .optim import Chain

__all__ = ["ConditionNet", "ConditionTrainer", "check_offsets", "check_take", "clamp_offsets", "dropout_keep",
           "segment_max", "segment_mean", "segment_repeat", "segment_sum", "segment_take", "shard_sets", "take_rows"]

_U64 = (1 << 64) - 1
_POOLS = {None: L.ZF_POOL_NONE, "sum": L.ZF_POOL_SUM, "max": L.ZF_POOL_MAX}


def check_offsets(offsets, rows: int) -> np.ndarray:
    """Host offsets as int64, validated: S + 1 >= 2 non-decreasing integers
    in [0, rows].  (Offsets already on the device are not read back: the
    kernel clamps them, see :func:`clamp_offsets`.)"""
    a = np.asarray(offsets)
    if a.ndim != 1 or a.size < 2:
        raise ValueError(f"offsets must be 1-D with at least 2 entries (S + 1), got shape {a.shape}")
    if not np.issubdtype(a.dtype, np.integer):
        if not np.all(a == np.floor(a)):
            raise ValueError("offsets must be integers")
    a = a.astype(np.int64)
    if a[0] < 0 or (a < 0).any():
        raise ValueError("offsets must not be negative")
    if (np.diff(a) < 0).any():
        raise ValueError("offsets must not decrease")
    if a[-1] > rows:
        raise ValueError(f"offsets reach row {int(a[-1])} of {rows}")
    return np.ascontiguousarray(a)


def clamp_offsets(offsets, rows: int) -> np.ndarray:
    """What the kernel makes of any offsets before use: each clamped to
    [0, rows], then the running maximum (zf_segment_sum)."""
    a = np.clip(np.asarray(offsets, np.int64), 0, int(rows))
    return np.maximum.accumulate(a)


def shard_sets(offsets, rank: int, world: int) -> Tuple[int, int, int, int]:
    """``(s0, s1, r0, r1)``: the sets ``[s0, s1)`` and the element rows
    ``[r0, r1) = [offsets[s0], offsets[s1])`` of ``rank`` when the S sets of
    ``offsets`` (S + 1, validated with :func:`check_offsets`) are split
    contiguously over ``world`` ranks as ``dist.shard_rows`` splits rows: a set
    lives on one rank, and the flow's rows are the sets, so ``[s0, s1)`` is
    also the flow trainer's shard.  The rank's own pass takes
    ``offsets[s0:s1 + 1] - offsets[s0]`` with ``row_base=r0`` and
    ``global_rows=offsets[-1]``.  With more ranks than sets the last ranks
    get none (``s0 == s1``)."""
    from .dist import shard_rows

    off = check_offsets(offsets, np.iinfo(np.int64).max)
    s0, s1 = shard_rows(off.size - 1, int(rank), int(world))
    return s0, s1, int(off[s0]), int(off[s1])


def dropout_keep(seed: int, rows, cols: int, rate: float) -> np.ndarray:
    """The dropout mask of the device (include/zenflow_amd.h, Dropout):
    ``keep[i, f] = u01_co(philox_at(seed, rows[i], f, ZF_DROPOUT_STREAM)[ZF_DROPOUT_WORD]) >= rate``
    for the element rows ``rows`` (an int or an index array) — Philox4x32-10
    restated in NumPy."""
    rows = np.arange(rows, dtype=np.int64) if np.isscalar(rows) else np.asarray(rows, np.int64)
    seed = int(seed) & _U64
    k0 = np.uint64(seed & 0xFFFFFFFF)
    k1 = np.uint64(seed >> 32)
    r = rows.astype(np.uint64)[:, None]
    f = np.arange(cols, dtype=np.uint64)[None, :]
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.broadcast_to(r & m32, (rows.size, cols)).copy(), np.broadcast_to(r >> np.uint64(32), (rows.size, cols)).copy(),
         np.broadcast_to(f, (rows.size, cols)).copy(), np.full((rows.size, cols), L.ZF_DROPOUT_STREAM, np.uint64)]
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    W0, W1 = 0x9E3779B9, 0xBB67AE85
    for rnd in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]  # 32 x 32 -> 64 bits: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & m32, p1 >> np.uint64(32), p1 & m32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = np.uint64((int(k0) + W0) & 0xFFFFFFFF)
        k1 = np.uint64((int(k1) + W1) & 0xFFFFFFFF)
    u = (c[L.ZF_DROPOUT_WORD] >> np.uint64(8)).astype(np.float32) * np.float32(2.0**-24)
    return u >= np.float32(rate)


def _shape2(a, what: str) -> Tuple[int, int]:
    """(rows, columns) of a 2-D float32 DeviceArray or of a host array, before anything is copied."""
    if isinstance(a, DeviceArray):
        if a.ndim != 2 or a.dtype != np.float32:
            raise ValueError(f"{what} must be a 2-D float32 DeviceArray, got {a.dtype} {a.shape}")
        return int(a.shape[0]), int(a.shape[1])
    shape = np.shape(a)
    if len(shape) != 2:
        raise ValueError(f"{what} must be 2-D, got {shape}")
    return int(shape[0]), int(shape[1])


def _to_device2(a) -> DeviceArray:
    return a if isinstance(a, DeviceArray) else DeviceArray.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32)))


def _segment_offsets(offsets, sets: Optional[int], rows: int):
    """Device offsets as they are (the kernel clamps them), host offsets
    validated (:func:`check_offsets`); ``sets`` (when known) fixes their
    number.  Nothing is copied to the device here."""
    if isinstance(offsets, DeviceArray):
        if offsets.ndim != 1 or offsets.dtype != np.int64 or offsets.shape[0] < 1:
            raise ValueError(f"device offsets must be 1-D int64 (S + 1 entries), got {offsets.dtype} {offsets.shape}")
        off = offsets
    else:
        off = check_offsets(offsets, rows)
    if sets is not None and off.shape[0] != sets + 1:
        raise ValueError(f"{sets} sets need {sets + 1} offsets, got {off.shape[0]}")
    return off


def repeats_to_offsets(repeats, sets: int) -> np.ndarray:
    """``repeats`` of ``np.repeat(c, repeats, axis=0)`` for ``sets`` rows (one
    non-negative int, or one per row) as the S + 1 int64 offsets of
    :func:`segment_repeat`."""
    r = np.asarray(repeats)
    if r.ndim > 1 or (r.ndim == 1 and r.shape[0] != sets):
        raise ValueError(f"repeats must be an int or {sets} ints, got shape {r.shape}")
    if not np.issubdtype(r.dtype, np.integer):
        if not np.all(r == np.floor(r)):
            raise ValueError("repeats must be integers")
    r = np.broadcast_to(r.astype(np.int64), (sets,))
    if (r < 0).any():
        raise ValueError("repeats must not be negative")
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(r, dtype=np.int64)])


def segment_repeat(c, offsets=None, *, repeats=None, rows: Optional[int] = None):
    """``jnp.repeat(c, sizes, axis=0)`` of the notebook's
    ``DeepSetFlow.sample`` on the device (zf_segment_repeat): ``c`` (S, F <=
    64) -> (rows, F) with ``out[i] = c[set(i)]`` and zeros for rows in no
    set.  The copies are given either as ``repeats`` (an int, or S
    non-negative ints; ``rows`` defaults to their sum) or as CSR ``offsets``
    (S + 1; host offsets are validated with :func:`check_offsets` and ``rows``
    defaults to the last one, device offsets (an int64 DeviceArray) are only
    clamped by the kernel and need ``rows``).  Host array in, host array out;
    DeviceArray in, DeviceArray out.  Its reverse is :func:`segment_sum`."""
    if (offsets is None) == (repeats is None):
        raise ValueError("segment_repeat takes either offsets or repeats" +
                         (", not both" if offsets is not None else ""))
    S, F = _shape2(c, "c")
    if repeats is not None:
        off = repeats_to_offsets(repeats, S)
        rows = int(off[-1]) if rows is None else int(rows)
        if rows < off[-1]:
            raise ValueError(f"repeats make {int(off[-1])} rows, rows = {rows}")
    else:
        if rows is None:
            if isinstance(offsets, DeviceArray):
                raise ValueError("device offsets are not read back: give rows")
            rows = int(np.asarray(offsets).reshape(-1)[-1]) if np.size(offsets) else 0
        rows = int(rows)
        if rows < 0:
            raise ValueError(f"rows must not be negative, got {rows}")
        off = _segment_offsets(offsets, S, rows)
    L.ensure_device()
    lib = L.load_library()
    cd, od = _to_device2(c), _device_offsets(off)
    out = DeviceArray((rows, F))
    ws = DeviceArray((max(1, lib.zf_segment_workspace_bytes(rows, S, F)),), np.uint8)
    check(lib.zf_segment_repeat(cd.ptr, S, F, od.ptr, rows, out.ptr, None, ws.ptr, L.stream()), "zf_segment_repeat")
    return out if isinstance(c, DeviceArray) else out.numpy()


def segment_sum(h, offsets):
    """The sum over each set's rows (zf_segment_sum, no dropout): ``h`` (rows,
    F <= 64) and S + 1 ``offsets`` -> (S, F); the reverse of
    :func:`segment_repeat` and the pooling of :class:`ConditionNet`, with its
    fixed order of additions.  Host offsets are validated, device offsets only
    clamped by the kernel.  Host array in, host array out; DeviceArray in,
    DeviceArray out."""
    rows, F = _shape2(h, "h")
    off = _segment_offsets(offsets, None, rows)
    S = off.shape[0] - 1
    L.ensure_device()
    lib = L.load_library()
    hd, od = _to_device2(h), _device_offsets(off)
    out = DeviceArray((S, F))
    ws = DeviceArray((max(1, lib.zf_segment_workspace_bytes(rows, S, F)),), np.uint8)
    check(lib.zf_segment_sum(hd.ptr, rows, F, od.ptr, S, 0.0, 0, out.ptr, None, ws.ptr, L.stream()), "zf_segment_sum")
    return out if isinstance(h, DeviceArray) else out.numpy()


def _segment_pool(h, offsets, pool: int):
    rows, F = _shape2(h, "h")
    off = _segment_offsets(offsets, None, rows)
    S = off.shape[0] - 1
    L.ensure_device()
    lib = L.load_library()
    hd, od = _to_device2(h), _device_offsets(off)
    out = DeviceArray((S, F))
    ws = DeviceArray((max(1, lib.zf_segment_pool_workspace_bytes(rows, S, F, pool)),), np.uint8)
    check(lib.zf_segment_pool(hd.ptr, rows, F, od.ptr, S, pool, 0.0, 0, out.ptr, None, None, ws.ptr, L.stream()),
          "zf_segment_pool")
    return out if isinstance(h, DeviceArray) else out.numpy()


def segment_mean(h, offsets):
    """The mean over each set's rows (zf_segment_pool, ZF_POOL_MEAN, no
    dropout): :func:`segment_sum`'s result divided by the set's number of rows
    in one fp32 division, a zero row for an empty set.  Arguments and
    conventions as :func:`segment_sum`'s."""
    return _segment_pool(h, offsets, L.ZF_POOL_MEAN)


def segment_max(h, offsets):
    """The maximum over each set's rows (zf_segment_pool, ZF_POOL_MAX, no
    dropout): exact, a NaN in a (set, column) gives NaN there as ``jnp.max``
    does, a zero row for an empty set.  Arguments and conventions as
    :func:`segment_sum`'s."""
    return _segment_pool(h, offsets, L.ZF_POOL_MAX)


def check_take(take, sets: int) -> np.ndarray:
    """Host set indices as int64, validated: 1-D integers, each in
    [0, sets).  (Indices already on the device are not read back: the kernel
    makes an index outside that range an empty set.)"""
    a = np.asarray(take)
    if a.ndim != 1:
        raise ValueError(f"take must be 1-D, got shape {a.shape}")
    if not np.issubdtype(a.dtype, np.integer):
        if a.dtype == object or not np.issubdtype(a.dtype, np.number) or not np.all(a == np.floor(a)):
            raise ValueError("take must be integers")
    a = a.astype(np.int64)
    if a.size and (a.min() < 0 or a.max() >= sets):
        raise ValueError(f"take must lie in [0, {sets}), got {int(a.min())} .. {int(a.max())}")
    return np.ascontiguousarray(a)


def _take_arg(take, sets: int):
    """A device ``take`` as it is (1-D int64), a host one validated."""
    if isinstance(take, DeviceArray):
        if take.ndim != 1 or take.dtype != np.int64:
            raise ValueError(f"a device take must be 1-D int64, got {take.dtype} {take.shape}")
        return take
    return check_take(take, sets)


def _take_launch(xd: DeviceArray, rows: int, F: int, od: Optional[DeviceArray], S: int, take, rows_out: int,
                 out_shape) -> Tuple[DeviceArray, DeviceArray]:
    """zf_segment_take on device buffers: (out, off_out)."""
    lib = L.load_library()
    td = take if isinstance(take, DeviceArray) else DeviceArray.from_numpy(take)
    n = int(td.shape[0])
    out, off_out = DeviceArray(out_shape), DeviceArray((n + 1,), np.int64)
    ws = DeviceArray((max(1, lib.zf_segment_take_workspace_bytes(S, n)),), np.uint8)
    check(lib.zf_segment_take(xd.ptr, rows, F, None if od is None else od.ptr, S, td.ptr, n, rows_out, out.ptr,
                              off_out.ptr, ws.ptr, L.stream()), "zf_segment_take")
    return out, off_out


def segment_take(x, offsets, take, *, rows: Optional[int] = None):
    """The sets ``take`` of a ragged batch, packed (zf_segment_take): ``x``
    (rows_x, F <= 64) and S + 1 ``offsets`` -> ``(x_out, offsets_out)`` with
    the element rows of set ``take[0]``, then of ``take[1]``, ... each in its
    own order, and their ``len(take) + 1`` CSR offsets — a minibatch of a
    deep-set data set that stays on the device.  Duplicates are allowed.

    ``x_out`` has ``rows`` rows, zeros behind the last set; ``rows`` defaults
    to the sum of the taken lengths when ``offsets`` and ``take`` are both on
    the host.  Host offsets are validated (:func:`check_offsets`), a host
    ``take`` too (1-D integers in [0, S)), and ``rows`` below the sum of their
    lengths is a ValueError.  Device ``offsets`` or a device ``take`` (int64
    DeviceArrays) are not read back: they need ``rows``, the kernel clamps the
    offsets (:func:`clamp_offsets`), takes an index outside [0, S) as an empty
    set and truncates at ``rows``.  Host array in, host arrays out; a
    DeviceArray ``x`` gives DeviceArrays (``offsets_out`` int64)."""
    rows_x, F = _shape2(x, "x")
    off = _segment_offsets(offsets, None, rows_x)
    S = off.shape[0] - 1
    take = _take_arg(take, S)
    on_host = not isinstance(off, DeviceArray) and not isinstance(take, DeviceArray)
    if rows is None and not on_host:
        raise ValueError("device offsets and a device take are not read back: give rows")
    if rows is not None and int(rows) < 0:
        raise ValueError(f"rows must not be negative, got {rows}")
    if on_host:
        need = int(np.diff(off)[take].sum())
        rows = need if rows is None else int(rows)
        if rows < need:
            raise ValueError(f"the taken sets have {need} rows, rows = {rows}")
    rows = int(rows)
    L.ensure_device()
    out, off_out = _take_launch(_to_device2(x), rows_x, F, _device_offsets(off), S, take, rows, (rows, F))
    return (out, off_out) if isinstance(x, DeviceArray) else (out.numpy(), off_out.numpy())


def take_rows(y, take):
    """``y[take]`` on the device (zf_segment_take with every row its own
    set): ``y`` (S, F <= 64), or 1-D (S,), returned 1-D — the per-set targets
    of the minibatch that :func:`segment_take` packs.  A host ``take`` is
    validated (1-D integers in [0, S)), a device one (int64 DeviceArray) made
    harmless by the kernel: an index outside [0, S) is an empty set, as in
    :func:`segment_take` — its row is left out, the rows behind it move up
    and zero rows close the result.  Host array in, host array out;
    DeviceArray in, DeviceArray out."""
    if isinstance(y, DeviceArray):
        if y.ndim not in (1, 2) or y.dtype != np.float32:
            raise ValueError(f"y must be a 1-D or 2-D float32 DeviceArray, got {y.dtype} {y.shape}")
        shape = y.shape
    else:
        shape = np.shape(y)
        if len(shape) not in (1, 2):
            raise ValueError(f"y must be 1-D or 2-D, got {shape}")
    S, F = int(shape[0]), int(shape[1]) if len(shape) == 2 else 1
    take = _take_arg(take, S)
    n = int(take.shape[0])
    L.ensure_device()
    yd = y if isinstance(y, DeviceArray) else DeviceArray.from_numpy(np.ascontiguousarray(np.asarray(y, np.float32)))
    out, _ = _take_launch(yd, S, F, None, S, take, n, (n, F) if len(shape) == 2 else (n,))
    return out if isinstance(y, DeviceArray) else out.numpy()


class _Layout:
    """The natural blob of a ConditionNet for ``in_dim`` input columns
    (zf_condnet_plan): descriptor, and blob <-> variable trees."""

    def __init__(self, net: "ConditionNet", in_dim: int):
        self.in_dim = int(in_dim)
        layers = tuple(int(w) for w in net.layers)
        if self.in_dim > 64:
            raise NotImplementedError(f"ConditionNet: {self.in_dim} input columns (at most 64)")
        if len(layers) > 16:
            raise NotImplementedError(f"ConditionNet: {len(layers)} hidden layers (at most 16)")
        d = L.ZfCondnetDesc()
        d.in_dim = self.in_dim
        d.n_hidden = len(layers)
        for l, w in enumerate(layers):
            d.hidden[l] = w
        d.out_dim = int(net.features)
        d.act = act_code(net.act)
        d.batch_norm = 1 if net.batch_norm else 0
        d.pool = _POOLS[net.pool]
        d.dropout = float(net.dropout)
        n = ct.c_int64()
        check(L.load_library().zf_condnet_plan(ct.byref(d), ct.byref(n)), "zf_condnet_plan")
        self.desc, self.size = d, int(n.value)
        # (collection, path, offset, shape) of every tensor
        self.entries = []
        if net.batch_norm:
            for j, (col, name) in enumerate((("batch_stats", "mean"), ("batch_stats", "var"), ("params", "scale"),
                                             ("params", "bias"))):
                self.entries.append((col, ("BatchNorm_0", name), int(d.off_bn) + j * self.in_dim, (self.in_dim,)))
        w_in = self.in_dim
        for l, w_out in enumerate(layers + (int(net.features),)):
            self.entries.append(("params", ("NNBlock_0", f"Dense_{l}", "kernel"), int(d.off_w[l]), (w_in, w_out)))
            self.entries.append(("params", ("NNBlock_0", f"Dense_{l}", "bias"), int(d.off_b[l]), (w_out,)))
            w_in = w_out
        self.param_mask = np.zeros(self.size, np.uint8)
        for col, _, off, shape in self.entries:
            if col == "params":
                self.param_mask[off:off + int(np.prod(shape))] = 1

    def to_blob(self, variables: Dict[str, Any], cols=("params", "batch_stats"), dtype=np.float32, strict=True):
        blob = np.zeros(self.size, dtype)
        for col, path, off, shape in self.entries:
            if col not in cols:
                continue
            node = (variables or {}).get(col, {})
            for k in path:
                node = node.get(k) if isinstance(node, dict) else None
                if node is None:
                    break
            if node is None:
                if strict:
                    raise KeyError(f"{col}/{'/'.join(path)} is missing from the variables")
                continue
            a = np.asarray(node)
            if dtype == np.uint8:  # a mask leaf may be one bool
                a = np.broadcast_to(a, shape)
            if a.shape != shape:
                raise ValueError(f"{col}/{'/'.join(path)} has shape {a.shape}, expected {shape}")
            blob[off:off + a.size] = a.reshape(-1)
        return blob

    def to_tree(self, blob, cols=("params", "batch_stats")) -> Dict[str, Any]:
        blob = np.asarray(blob)
        out: Dict[str, Any] = {}
        for col, path, off, shape in self.entries:
            if col not in cols:
                continue
            node = out.setdefault(col, {})
            for k in path[:-1]:
                node = node.setdefault(k, {})
            node[path[-1]] = blob[off:off + int(np.prod(shape))].reshape(shape).copy()
        return out


def _seed64(seed) -> int:
    return int(seed) & _U64


class _Handle:
    """One zf_condnet handle: the network on the device for passes of up to
    ``rows_max`` rows in up to ``sets_max`` sets."""

    def __init__(self, layout: _Layout, variables, rows_max: int, sets_max: int, opt_desc=None):
        L.ensure_device()
        self.layout = layout
        self.rows_max, self.sets_max = int(rows_max), int(sets_max)
        blob = layout.to_blob(variables)
        h = ct.c_void_p()
        check(L.load_library().zf_condnet_create(
            ct.byref(layout.desc), blob.ctypes.data, blob.size, layout.param_mask.ctypes.data, self.rows_max,
            self.sets_max, None if opt_desc is None else ct.byref(opt_desc), ct.byref(h)), "zf_condnet_create")
        self.ptr = h.value

    def __del__(self):
        p = getattr(self, "ptr", None)
        if p and L._lib is not None:
            L._lib.zf_condnet_destroy(ct.c_void_p(p))
            self.ptr = None

    @property
    def pooled(self) -> bool:
        return self.layout.desc.pool != L.ZF_POOL_NONE

    def forward(self, xd: DeviceArray, off: Optional[DeviceArray], train: bool, update_stats: bool, seed: int,
                global_rows: Optional[int] = None, row_base: int = 0):
        """``xd``: this rank's rows, from global row ``row_base`` on, of a pass of ``global_rows`` (None: its own) rows."""
        rows = xd.shape[0]
        sets = 0 if off is None else off.shape[0] - 1
        out = DeviceArray((sets if self.pooled else rows, self.layout.desc.out_dim))
        check(L.load_library().zf_condnet_forward_shard(
            self.ptr, xd.ptr, rows, rows if global_rows is None else int(global_rows), int(row_base),
            None if off is None else off.ptr, sets, 1 if train else 0, 1 if update_stats else 0, _seed64(seed),
            out.ptr, L.stream()), "zf_condnet_forward_shard")
        return out

    def blob(self) -> np.ndarray:
        b = np.empty(self.layout.size, np.float32)
        check(L.load_library().zf_condnet_get_blob(self.ptr, b.ctypes.data), "zf_condnet_get_blob")
        return b


def _prep_x(x, in_dim: Optional[int] = None) -> Tuple[DeviceArray, bool]:
    if isinstance(x, DeviceArray):
        if x.ndim != 2 or x.dtype != np.float32:
            raise ValueError(f"x must be a 2-D float32 DeviceArray (rows, in_dim), got {x.dtype} {x.shape}")
        xd, dev = x, True
    else:
        a = np.asarray(x, np.float32)
        if a.ndim != 2:
            raise ValueError(f"x must be 2-D (rows, in_dim), got {a.shape}")
        xd, dev = DeviceArray.from_numpy(np.ascontiguousarray(a)), False
    if in_dim is not None and xd.shape[1] != in_dim:
        raise ValueError(f"x must have {in_dim} columns, got {xd.shape[1]}")
    return xd, dev


def _check_offsets_arg(offsets, rows: int, pooled: bool):
    """The ``offsets`` argument, checked on the host before anything touches
    the device: None (no pooling), a DeviceArray as it is, or the validated
    int64 host array."""
    if not pooled:
        if offsets is not None:
            raise ValueError("offsets given to a network without pooling (pool=None)")
        return None
    if offsets is None:
        raise ValueError("a pooled network needs the sets' offsets")
    if isinstance(offsets, DeviceArray):
        if offsets.ndim != 1 or offsets.dtype != np.int64 or offsets.shape[0] < 2:
            raise ValueError(f"device offsets must be 1-D int64 with S + 1 >= 2 entries, got {offsets.dtype} "
                             f"{offsets.shape}")
        return offsets
    return check_offsets(offsets, rows)


def _device_offsets(off) -> Optional[DeviceArray]:
    return off if off is None or isinstance(off, DeviceArray) else DeviceArray.from_numpy(off)


class ConditionNet(Module):
    """``Phi`` of examples/deep_set.ipynb: BatchNorm, ``len(layers)`` Dense
    layers with ``act``, a Dense layer to ``features`` columns, Dropout, and
    with ``pool="sum"`` / ``"max"`` that reduction over each
    set's rows (an empty set gives a zero row; the max passes a NaN on as
    ``jnp.max`` does and splits its gradient evenly among ties, dropped
    entries being zeros that take part).

    ``__call__(x, offsets=None, *, train=False, seed=0)``: ``x`` (rows,
    in_dim) -> (S, features) when pooled (``offsets``: S + 1
    non-decreasing integers, host offsets are validated with ValueError,
    device offsets (an int64 DeviceArray) only clamped by the kernel) or
    (rows, features) with ``pool=None``.  Host arrays in, host arrays out;
    DeviceArray in, DeviceArray out.  ``train=True`` normalises by the
    statistics of all rows passed (padding rows included, as the notebook's
    BatchNorm sees them), draws the dropout mask from ``seed`` and needs
    ``mutable=["batch_stats"]`` when the network has a BatchNorm.

    The variables have the notebook's layout whatever the pooling, so a tree
    trained with the reference's ``Phi`` loads unchanged: ``params``: ``BatchNorm_0/{scale,
    bias}``, ``NNBlock_0/Dense_k/{kernel, bias}``; ``batch_stats``:
    ``BatchNorm_0/{mean, var}`` (no BatchNorm entries with
    ``batch_norm=False``)."""

    def __init__(self, features: int, layers: Sequence[int] = (128, 128, 128), act: Union[str, Callable] = swish,
                 batch_norm: bool = True, dropout: float = 0.0, pool: Optional[str] = None):
        if pool not in _POOLS:
            raise NotImplementedError(f'pool={pool!r}: only None, "sum" and "max" are implemented')
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"dropout rate {dropout} outside [0, 1)")
        if int(features) < 1:
            raise ValueError(f"features must be positive, got {features}")
        if int(features) > 64:
            raise NotImplementedError(f"ConditionNet: {features} output columns (at most 64)")
        layers = tuple(int(w) for w in layers)
        if any(w < 1 for w in layers):
            raise ValueError(f"layer widths must be positive, got {layers}")
        if any(w > 4096 for w in layers):
            raise NotImplementedError(f"ConditionNet: a hidden width above 4096 in {layers}")
        if len(layers) > 16:
            raise NotImplementedError(f"ConditionNet: {len(layers)} hidden layers (at most 16)")
        self.features = int(features)
        self.layers = layers
        self.act = act
        self.batch_norm = bool(batch_norm)
        self.dropout = float(dropout)
        self.pool = pool

    # -- variables ---------------------------------------------------------------
    def _layout(self, in_dim: int) -> _Layout:
        cache = self.__dict__.setdefault("_layouts", {})
        if in_dim not in cache:
            cache[in_dim] = _Layout(self, in_dim)
        return cache[in_dim]

    def _init_variables(self, gen, D, C, params, stats) -> None:
        self._layout(D)  # rejects what the kernels do not take
        if self.batch_norm:
            params["BatchNorm_0"] = {"scale": np.ones(D, np.float32), "bias": np.zeros(D, np.float32)}
            stats["BatchNorm_0"] = {"mean": np.zeros(D, np.float32), "var": np.ones(D, np.float32)}
        block: Dict[str, Any] = {}
        w_in = D
        for l, w_out in enumerate(self.layers + (self.features,)):
            block[f"Dense_{l}"] = {"kernel": lecun_normal(gen, w_in, w_out), "bias": np.zeros(w_out, np.float32)}
            w_in = w_out
        params["NNBlock_0"] = block

    # -- the forward pass -----------------------------------------------------------
    def _eval_handle(self, variables, layout: _Layout, rows: int, sets: int) -> _Handle:
        from .engine import PROGRAM_CACHE_SIZE, _digest

        key = (_digest(variables), layout.in_dim)
        cache = self.__dict__.setdefault("_handles", OrderedDict())
        h = cache.get(key)
        if h is None or h.rows_max < rows or h.sets_max < sets:
            h = _Handle(layout, variables, max(rows, 1), max(sets, 1))
            cache[key] = h
            while len(cache) > PROGRAM_CACHE_SIZE:
                cache.popitem(last=False)
        cache.move_to_end(key)
        return h

    def __call__(self, x, offsets=None, *, train: bool = False, seed: int = 0):
        scope = scope_for(self)
        shape = x.shape if isinstance(x, DeviceArray) else np.shape(x)
        if len(shape) != 2:
            raise ValueError(f"x must be 2-D (rows, in_dim), got {shape}")
        rows, in_dim = int(shape[0]), int(shape[1])
        if scope.initializing:  # inside an outer module's init: create variables only
            scope.init_module(self, in_dim, 0)
            n_out = rows
            if self.pool is not None:
                if offsets is None:
                    raise ValueError("a pooled network needs the sets' offsets")
                n_out = int((offsets.shape if isinstance(offsets, DeviceArray) else np.shape(offsets))[0]) - 1
            return np.zeros((n_out, self.features), np.float32)
        layout = self._layout(in_dim)
        off = _check_offsets_arg(offsets, rows, self.pool is not None)
        xd, x_dev = _prep_x(x)
        off = _device_offsets(off)
        sets = 0 if off is None else off.shape[0] - 1
        if train:
            update = self.batch_norm and "batch_stats" in scope.mutable
            if self.batch_norm and not update:
                raise RuntimeError("train=True updates batch_stats; pass mutable=['batch_stats']")
            h = _Handle(layout, scope.variables, max(rows, 1), max(sets, 1))  # its statistics change: never shared
            out = h.forward(xd, off, True, update, seed)
            if update:
                scope.updates["batch_stats"] = layout.to_tree(h.blob(), cols=("batch_stats",))["batch_stats"]
        else:
            out = self._eval_handle(scope.variables, layout, rows, sets).forward(xd, off, False, False, 0)
        return out if x_dev else out.numpy()


class ConditionTrainer:
    """A :class:`ConditionNet` resident on the device for training: blob
    (parameters and BatchNorm statistics), the activations of one pass of up
    to ``rows_max`` element rows in up to ``sets_max`` sets (default
    ``rows_max``), the gradient and the optimiser state.

    ``optimizer``: a ``zenflow_amd.train.Optimizer`` ((n)adamw) or any chain of
    ``zenflow_amd.optim`` (clipping, schedules, a masked weight decay whose
    mask is shaped like this network's ``params``); default nadamw(1e-3).

    The joint loop of the notebook's ``loss_fn_2`` / ``step`` next to a
    ``Trainer`` ``tr`` of the flow::

        c = ct.forward(Xd, off_d, seed=epoch)
        gc = tr.step(Yd, c, cond_grad=True)
        ct.step(gc)

    and likewise with the ``d / d c`` of ``tr.sample_backward`` or
    ``tr.log_prob_vjp``.  A network behind this one (the notebook's ``rho``
    behind ``phi``, ``class DeepSet``) is a second trainer whose
    ``backward(gy, input_grad=True)`` or ``step(gy, input_grad=True)`` returns
    the ``d loss / d x`` that is this one's ``gc``::

        c = pt.forward(Xd, off_d, seed=epoch)
        yp = rt.forward(c)
        pt.step(rt.step(gy, input_grad=True))

    ``comm``: data parallelism, as ``Trainer(comm=)`` takes it
    (``dist.RcclCommunicator``, or ``dist.HostAllgather`` for ranks sharing a
    GPU).  Every rank holds whole sets (:func:`shard_sets`) and calls
    ``forward`` / ``backward`` / ``apply_gradient`` with its own element rows,
    offsets and ``gc`` rows — under ``tr = Trainer(..., comm=comm)`` the ``gc``
    of ``tr.step(Y[s0:s1], c, cond_grad=True)`` is just that.  BatchNorm's
    batch sums (forward, and reverse when ``input_grad=True``) and the
    gradient are exchanged as the ranks' fp64 tree roots: at most three
    all-gathers a step, one for a network without BatchNorm.  Every rank ends
    with the same gradient, parameters, statistics and optimiser state, bit
    for bit, for any split of whole sets; R ranks (a power of two) with
    ``global_rows / R`` element rows each, ``global_rows`` a multiple of the
    leaf count, reproduce the bits of one device on the concatenated batch.

    :meth:`opt_state` / :meth:`load_opt_state` with :meth:`variables` are all
    a run needs to resume.

    Not provided: eval-mode input gradients (an eval forward leaves nothing
    pending), splitting one set across ranks, graph capture,
    mean pooling inside the network (:func:`segment_mean` is the reduction alone)."""

    def __init__(self, net: ConditionNet, variables: Dict[str, Any], in_dim: int, rows_max: int,
                 sets_max: Optional[int] = None, optimizer=None, comm=None):
        from .train import DEFAULT_OPTIMIZER, Optimizer

        self.net = net
        self.in_dim = int(in_dim)
        self.layout = net._layout(self.in_dim)
        self.optimizer = optimizer if optimizer is not None else DEFAULT_OPTIMIZER()
        chain = self.optimizer if isinstance(self.optimizer, Chain) else None
        if chain is None and not isinstance(self.optimizer, Optimizer):
            raise TypeError("optimizer must be a zenflow_amd.train.Optimizer or a zenflow_amd.optim chain")
        lowered = dmask = None
        if chain is not None:  # rejected chains raise here, before any handle exists
            lowered = chain.lower()
            if chain.mask() is not None:
                dmask = self._lower_mask(chain.mask(), variables)
        rows_max = int(rows_max)
        sets_max = rows_max if sets_max is None else int(sets_max)
        if rows_max < 1 or sets_max < 1:
            raise ValueError(f"rows_max and sets_max must be positive, got {rows_max}, {sets_max}")
        self._h = _Handle(self.layout, variables, rows_max, sets_max,
                          None if chain is not None else self.optimizer.desc())
        if chain is not None:
            check(L.load_library().zf_condnet_set_optim_chain(
                self._h.ptr, ct.byref(lowered), None if dmask is None else dmask.ctypes.data),
                "zf_condnet_set_optim_chain")
        self._pending: Optional[Tuple[int, bool, int]] = None  # (rows of c, device result?, rows of x)
        self._last_grad: Optional[DeviceArray] = None
        self.comm = comm
        self.rank, self.world = 0, 1
        if comm is not None:
            self._comm_desc = comm.trainer_comm_desc()  # kept alive: the C side holds its pointers
            check(L.load_library().zf_condnet_set_comm(self._h.ptr, ct.byref(self._comm_desc)), "zf_condnet_set_comm")
            self.rank, self.world = int(comm.rank), int(comm.world)

    @property
    def handle(self) -> int:
        return self._h.ptr

    @property
    def rows_max(self) -> int:
        return self._h.rows_max

    @property
    def sets_max(self) -> int:
        return self._h.sets_max

    def _lower_mask(self, mask, variables) -> np.ndarray:
        if callable(mask):
            mask = mask(variables["params"])
        return np.ascontiguousarray(self.layout.to_blob({"params": mask}, cols=("params",), dtype=np.uint8))

    def _shard(self, rows: int, global_rows: Optional[int], row_base: Optional[int]) -> Tuple[int, int]:
        """(global_rows, row_base) of a pass of ``rows`` rows on this rank:
        the equal-shard values by default, ValueError for what
        zf_condnet_forward_shard would reject."""
        if self.world > 1 and (global_rows is None) != (row_base is None):
            raise ValueError("under data parallelism global_rows and row_base go together: give both or neither")
        g = rows * self.world if global_rows is None else int(global_rows)
        b = rows * self.rank if row_base is None else int(row_base)
        if g < rows or b < 0 or b + rows > g or (self.world == 1 and g != rows):
            raise ValueError(f"rows [{b}, {b + rows}) of global_rows {g} (rows {rows}, world {self.world})")
        return g, b

    def forward(self, x, offsets=None, *, train: bool = True, update_stats: Optional[bool] = None, seed: int = 0,
                global_rows: Optional[int] = None, row_base: Optional[int] = None):
        """``c`` of ``net.apply(..., train=train)`` at the trainer's
        parameters (zf_condnet_forward_shard): (S, features) pooled, (rows,
        features) otherwise; a DeviceArray when ``x`` is one.  ``train=True``
        keeps the activations for one :meth:`backward`, normalises by batch
        statistics, draws the dropout mask from ``seed`` and moves the running
        statistics when ``update_stats`` (default: ``train``).

        Data parallel: ``x`` and ``offsets`` (local to ``x``) are this rank's
        whole sets of a global pass of ``global_rows`` element rows, of which
        this rank's first is ``row_base`` (defaults: ``rows * world`` and
        ``rank * rows``, equal shards; give both for any other split, see
        :func:`shard_sets`).  The result holds this rank's sets."""
        train = bool(train)
        update_stats = train if update_stats is None else bool(update_stats)
        if update_stats and not train:
            raise ValueError("update_stats=True needs train=True: eval mode reads the stored statistics")
        shape = x.shape if isinstance(x, DeviceArray) else np.shape(x)
        if len(shape) != 2 or shape[1] != self.in_dim:
            raise ValueError(f"x must have shape (rows, {self.in_dim}), got {tuple(shape)}")
        rows = int(shape[0])
        global_rows, row_base = self._shard(rows, global_rows, row_base)
        if rows > self.rows_max:
            raise ValueError(f"forward takes at most rows_max = {self.rows_max} rows, got {rows}")
        off = _check_offsets_arg(offsets, rows, self._h.pooled)
        if off is not None and off.shape[0] - 1 > self.sets_max:
            raise ValueError(f"forward takes at most sets_max = {self.sets_max} sets, got {off.shape[0] - 1}")
        xd, x_dev = _prep_x(x, self.in_dim)
        off = _device_offsets(off)
        self._pending = None
        out = self._h.forward(xd, off, train, update_stats, seed, global_rows, row_base)
        if train:
            self._pending = (out.shape[0], x_dev, rows)
        return out if x_dev else out.numpy()

    def backward(self, gc, *, input_grad: bool = False):
        """The gradient, in the blob layout, of the loss whose ``d loss / d c``
        is ``gc`` (the shape of the pending forward's result; a host array or
        a float32 DeviceArray) with respect to the network's parameters
        (zf_condnet_backward; :meth:`grad_tree` makes a ``params`` tree of
        it).  A DeviceArray when ``forward`` was given one.  One backward per
        train-mode forward: ValueError otherwise.

        ``input_grad=True`` returns ``(g, gx)`` with ``gx`` (rows, in_dim)
        float32 the ``d loss / d x`` of the pending pass
        (zf_condnet_backward_input), on the device or the host as ``g`` is;
        ``g`` has the same bits either way."""
        if self._pending is None:
            raise ValueError("backward needs a pending train-mode forward (one backward per forward; an eval-mode "
                             "forward and apply_gradient leave none)")
        n, dev, rows = self._pending
        F = self.net.features
        if isinstance(gc, DeviceArray):
            if gc.dtype != np.float32 or int(np.prod(gc.shape)) != n * F:
                raise ValueError(f"gc must hold ({n}, {F}) float32 entries, got {gc.dtype} {gc.shape}")
            gd = gc
        else:
            a = np.asarray(gc, np.float32)
            if a.size != n * F:
                raise ValueError(f"gc must have shape ({n}, {F}), got {a.shape}")
            gd = DeviceArray.from_numpy(np.ascontiguousarray(a.reshape(n, F)))
        g = DeviceArray((self.layout.size,))
        self._pending = None
        if not input_grad:
            check(L.load_library().zf_condnet_backward(self._h.ptr, gd.ptr, g.ptr, L.stream()), "zf_condnet_backward")
            self._last_grad = g
            return g if dev else g.numpy()
        gx = DeviceArray((rows, self.in_dim))
        check(L.load_library().zf_condnet_backward_input(self._h.ptr, gd.ptr, g.ptr, gx.ptr, L.stream()),
              "zf_condnet_backward_input")
        self._last_grad = g
        return (g, gx) if dev else (g.numpy(), gx.numpy())

    def apply_gradient(self, g=None) -> None:
        """The optimiser update on ``g`` (zf_condnet_apply_gradient): a
        blob-layout host array or DeviceArray, a ``params`` tree as
        :meth:`grad_tree` returns it, or None for the last backward's."""
        n = self.layout.size
        if g is None:
            if self._last_grad is None:
                raise ValueError("apply_gradient() without a gradient needs an earlier backward")
            gd = None
        elif isinstance(g, DeviceArray):
            gd = g
        else:
            if isinstance(g, dict):
                g = self.layout.to_blob({"params": g}, cols=("params",))
            gd = DeviceArray.from_numpy(np.ascontiguousarray(np.asarray(g, np.float32).reshape(-1)))
        if gd is not None and (int(np.prod(gd.shape)) != n or gd.dtype != np.float32):
            raise ValueError(f"the gradient must hold {n} float32 entries (blob layout), got {gd.dtype} {gd.shape}")
        self._pending = None
        check(L.load_library().zf_condnet_apply_gradient(self._h.ptr, None if gd is None else gd.ptr, L.stream()),
              "zf_condnet_apply_gradient")

    def step(self, gc, *, input_grad: bool = False):
        """:meth:`backward` then :meth:`apply_gradient`: one optimiser step on
        the gradient that ``gc`` sends back.  ``input_grad=True`` returns the
        ``gx`` of :meth:`backward`, formed before the update from the
        pre-update parameters; None otherwise."""
        if not input_grad:
            self.backward(gc)
            self.apply_gradient()
            return None
        _, gx = self.backward(gc, input_grad=True)
        self.apply_gradient()
        return gx

    def variables(self) -> Dict[str, Any]:
        """The current ``params`` and ``batch_stats`` trees."""
        return self.layout.to_tree(self._h.blob())

    def grad_tree(self, g) -> Dict[str, Any]:
        """Gradient blob -> ``params`` tree (like jax.grad's output)."""
        return self.layout.to_tree(np.asarray(g), cols=("params",))["params"]

    def _n_slots(self) -> int:
        return self.optimizer.n_slots if isinstance(self.optimizer, Chain) else 2

    def opt_state(self) -> Dict[str, Any]:
        """The optimiser's state, as ``Trainer.opt_state`` gives it:
        ``count``, the ``learning_rate`` and ``grad_norm`` the last step used
        (NaN before the first step; grad_norm NaN without
        clip_by_global_norm), and ``slots``, the moment arrays as
        ``params``-shaped trees in chain order (an ``Optimizer``: m, v)."""
        lib = L.load_library()
        count, lr, gn = ct.c_int64(), ct.c_double(), ct.c_double()
        check(lib.zf_condnet_get_opt_scalars(self._h.ptr, ct.byref(count), ct.byref(lr), ct.byref(gn)),
              "zf_condnet_get_opt_scalars")
        slots = []
        for k in range(self._n_slots()):
            blob = np.empty(self.layout.size, np.float32)
            check(lib.zf_condnet_get_opt_slot(self._h.ptr, k, blob.ctypes.data), "zf_condnet_get_opt_slot")
            slots.append(self.layout.to_tree(blob, cols=("params",))["params"])
        return {"count": int(count.value), "learning_rate": float(lr.value), "grad_norm": float(gn.value),
                "slots": slots}

    def load_opt_state(self, state: Dict[str, Any]) -> None:
        """Restore what :meth:`opt_state` returned (of a trainer with the
        same optimiser): the moments and the step counter, from which the
        bias corrections and the schedule follow."""
        slots = list(state["slots"])
        if len(slots) != self._n_slots():
            raise ValueError(f"state has {len(slots)} moment arrays, this optimiser keeps {self._n_slots()}")
        lib = L.load_library()
        for k, tree in enumerate(slots):
            blob = np.ascontiguousarray(self.layout.to_blob({"params": tree}, cols=("params",)))
            check(lib.zf_condnet_set_opt_slot(self._h.ptr, k, blob.ctypes.data), "zf_condnet_set_opt_slot")
        check(lib.zf_condnet_set_opt_count(self._h.ptr, int(state["count"])), "zf_condnet_set_opt_count")
