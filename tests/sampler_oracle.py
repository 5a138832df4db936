"""Host restatement of the device's latent sampler (zenflow_amd/csrc/zf_random.h)
in NumPy (tests/test_sampler_oracle_host.py, tests/test_gpu_sampling.py).

The device generator is fully specified: Philox4x32-10 (Salmon et al. 2011,
the Random123 constants) with counter (row lo, row hi, dim, stream) and key
(seed lo, seed hi), then

* ``u01_co`` / ``u01_oc``: the top 24 bits as a float in [0, 1) / (0, 1];
* Box-Muller ``n = sqrt(-2 log u_oc(w0)) * cos(pi * 2 u_co(w1))``;
* Uniform: stream 0, word 0.  Normal: stream 1, ``0.5 + 0.1 n``.
  TruncatedNormal: streams 1, 2, ... until ``|n| <= 5``;
* Beta(a, a) = x / (x + y) of two Marsaglia-Tsang Gamma(a, 1) draws, stream
  bases 16 and 17, trial t on stream base + 2t: ``v = 1 + c n`` with
  ``d = a - 1/3``, ``c = 1/sqrt(9 d)``; rejected when ``v <= 0``; accepted when
  ``log u_oc(w2) < n^2 / 2 + d - d v^3 + d log v^3``; the draw is ``d v^3``.

``latent_draw`` follows the device step for step in float32.  Where the device
may differ in the last bits the restatement takes the better-rounded value, so
a device deviation is bounded by the device's own error: ``cos(pi * 2u)`` is
evaluated in float64 and rounded once (the device calls ``cospif``);
``0.5 + 0.1 n`` and ``1 + c n`` are rounded once, as the device's fused
multiply-add does; ``log`` and ``sqrt`` are NumPy's float32 ones.

Rejection tests are discontinuous, so ``latent_draw`` also returns, for every
trial of every element, what the test compared: a GPU test sets aside the
elements whose comparison is a near-tie (``near_ties``) and holds every other
element to a derived bound."""

from __future__ import annotations

import numpy as np

from zenflow_amd import _lib as L

F32 = np.float32
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
MAX_TRIALS = 64


def philox4x32_10(counter, key):
    """Philox4x32-10.  counter (..., 4) and key (..., 2) as uint32 words
    (broadcast against each other over the leading axes) -> (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint32).astype(np.uint64)
    k = np.asarray(key, dtype=np.uint32).astype(np.uint64)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape) for i in range(2))
    for r in range(10):
        p0 = _M0 * c0  # 32 x 32 -> 64 bits, exact in uint64
        p1 = _M1 * c2
        kr0 = (k0 + np.uint64((_W0 * r) & 0xFFFFFFFF)) & _MASK
        kr1 = (k1 + np.uint64((_W1 * r) & 0xFFFFFFFF)) & _MASK
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ kr0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ kr1, p0 & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def philox_at(seed, rows, dim, stream):
    """The device's ``philox_at``: four words per row of ``rows`` (int64)."""
    rows = np.asarray(rows, dtype=np.int64).astype(np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.empty(rows.shape + (4,), np.uint32)
    ctr[..., 0] = (rows & _MASK).astype(np.uint32)
    ctr[..., 1] = (rows >> _S32).astype(np.uint32)
    ctr[..., 2] = np.uint32(int(dim) & 0xFFFFFFFF)
    ctr[..., 3] = np.uint32(int(stream) & 0xFFFFFFFF)
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32))


def u01_co(b):
    """[0, 1) from the top 24 bits (exact in float32)."""
    return (b >> np.uint32(8)).astype(F32) * F32(2.0**-24)


def u01_oc(b):
    """(0, 1] from the top 24 bits (exact in float32)."""
    return ((b >> np.uint32(8)).astype(np.int64) + 1).astype(F32) * F32(2.0**-24)


def normal_of(a, b):
    """Box-Muller standard normal from two words, float32."""
    r = np.sqrt(F32(-2.0) * np.log(u01_oc(a)))
    c = np.cos(np.pi * (2.0 * u01_co(b).astype(np.float64))).astype(F32)
    return (r * c).astype(F32)


def _fma32(a, b, c):
    """float32(a * b + c) rounded once: the product of two floats is exact in
    float64 and the sum's double rounding cannot matter at these magnitudes
    beyond what a test's bound already allows."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def gamma_draw(seed, rows, dim, base, alpha):
    """Marsaglia-Tsang Gamma(alpha, 1), alpha >= 1 -> (draw, trials).

    ``trials[t]`` describes trial t for the elements that ran it: ``idx``
    (positions in ``rows``), ``v`` (1 + c n, before the cube), ``margin``
    (rhs - log u; NaN where v <= 0 rejected first) and ``accepted``."""
    rows = np.asarray(rows, dtype=np.int64)
    d = F32(alpha) - F32(1.0 / 3.0)
    cc = F32(1.0 / np.sqrt(np.float64(F32(9.0) * d)))
    out = np.full(rows.shape, d, F32)  # the device's fall-through value
    taken = np.full(rows.shape, -1, np.int64)
    active = np.arange(rows.size)
    trials = []
    for t in range(MAX_TRIALS):
        if active.size == 0:
            break
        w = philox_at(seed, rows[active], dim, (base + 2 * t) & 0xFFFFFFFF)
        n = normal_of(w[:, 0], w[:, 1])
        v = _fma32(cc, n, F32(1.0))
        pos = v > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            v3 = (v * v * v).astype(F32)
            lu = np.log(u01_oc(w[:, 2]))
            rhs = (((F32(0.5) * n) * n + d) - d * v3) + d * np.log(v3)
            margin = np.where(pos, (rhs - lu).astype(F32), F32(np.nan)).astype(F32)
        acc = pos & (lu < rhs)
        out[active[acc]] = (d * v3[acc]).astype(F32)
        taken[active[acc]] = t
        trials.append({"idx": active.copy(), "v": v, "margin": margin, "accepted": acc})
        active = active[~acc]
    return out, taken, trials


def latent_draw(latent, param, seed, rows, dim):
    """z[rows, dim] of the device's ``latent_draw`` -> (z float32, info).

    info["trial"]: the index of the trial taken per element (Beta: the larger
    of its two gamma draws'); TruncatedNormal adds info["n"], the list of the
    standard normals tried per trial (``idx``, ``n``); Beta adds
    info["gamma"] = the two draws' ``trials`` lists (``gamma_draw``)."""
    rows = np.asarray(rows, dtype=np.int64)
    if latent == L.ZF_LATENT_UNIFORM:
        return u01_co(philox_at(seed, rows, dim, 0)[:, 0]), {"trial": np.zeros(rows.shape, np.int64)}
    if latent == L.ZF_LATENT_BETA:
        x, tx, trx = gamma_draw(seed, rows, dim, 16, F32(param))
        y, ty, try_ = gamma_draw(seed, rows, dim, 17, F32(param))
        z = (x / (x + y).astype(F32)).astype(F32)
        return z, {"trial": np.maximum(tx, ty), "gamma": (trx, try_)}
    if latent not in (L.ZF_LATENT_NORMAL, L.ZF_LATENT_TRUNCNORM):
        raise ValueError(f"bad latent {latent}")
    z = np.full(rows.shape, 0.5, F32)
    taken = np.full(rows.shape, -1, np.int64)
    active = np.arange(rows.size)
    tried = []
    for t in range(MAX_TRIALS):
        if active.size == 0:
            break
        w = philox_at(seed, rows[active], dim, 1 + t)
        n = normal_of(w[:, 0], w[:, 1])
        ok = np.abs(n) <= F32(5.0) if latent == L.ZF_LATENT_TRUNCNORM else np.ones(n.shape, bool)
        z[active[ok]] = _fma32(F32(0.1), n[ok], F32(0.5))
        taken[active[ok]] = t
        tried.append({"idx": active.copy(), "n": n})
        active = active[~ok]
    return z, {"trial": taken, "n": tried}


def sample(latent, param, seed, N, D):
    """(N, D) draws as zf_latent_sample lays them out -> (z, [info per dim])."""
    rows = np.arange(N, dtype=np.int64)
    cols, infos = [], []
    for d in range(D):
        z, info = latent_draw(latent, param, seed, rows, d)
        cols.append(z)
        infos.append(info)
    return np.stack(cols, axis=1), infos


def near_ties(info, n, margin_tol, v_tol):
    """Elements (bool mask over n) of a Beta draw where any trial of either
    gamma draw compared within ``margin_tol`` in the acceptance test or
    within ``v_tol`` in the ``v <= 0`` test."""
    tie = np.zeros(n, bool)
    for trials in info["gamma"]:
        for tr in trials:
            with np.errstate(invalid="ignore"):
                close = (np.abs(tr["margin"]) < margin_tol) | (np.abs(tr["v"]) < v_tol)
            tie[tr["idx"][close]] = True
    return tie
