"""The C-ABI library loads on a CPU-only host and exports every symbol that
include/zenflow_amd.h declares; host-only entry points (planning, error
reporting) behave, and the standalone entries reject bad arguments before
their first HIP call.  No GPU compute is called here."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "zenflow_amd.h"


def header_functions():
    text = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\**\s+\**\s*(zf_[a-z_0-9]+)\s*\(", text, flags=re.M)
    return sorted(set(names))


def test_header_parses():
    names = header_functions()
    assert "zf_flow_log_prob" in names and "zf_rqs_forward" in names
    assert len(names) >= 40


def test_library_exports_every_header_symbol():
    from zenflow_amd import _lib

    lib = _lib.load_library()
    missing = [n for n in header_functions() if not hasattr(lib, n)]
    assert not missing, missing
    # and the ctypes binding declares exactly the header's functions
    assert sorted(_lib.SIGNATURES) == header_functions()


def test_struct_layout_matches_header():
    from zenflow_amd import _lib

    assert ctypes.sizeof(_lib.ZfOpDesc) == 4 * 22 + 8 * (1 + 17 + 17 + 1)
    assert _lib.ZfFlowDesc.ops.offset == 24
    assert ctypes.sizeof(_lib.ZfFlowDesc) == 24 + 64 * ctypes.sizeof(_lib.ZfOpDesc)


def _desc(D, C, ops):
    from zenflow_amd import _lib as L

    d = L.ZfFlowDesc()
    d.dim, d.cond_dim, d.latent, d.n_ops = D, C, L.ZF_LATENT_NORMAL, len(ops)
    for i, op in enumerate(ops):
        o = d.ops[i]
        o.kind = op[0]
        if op[0] == L.ZF_OP_NSC:
            o.knots = op[1]
            o.n_hidden = len(op[2])
            for l, w in enumerate(op[2]):
                o.hidden[l] = w
        elif op[0] == L.ZF_OP_ROLL:
            o.shift = 1
    return d


def test_flow_plan_offsets_cfg2():
    """zf_flow_plan is host-only: the natural blob of rolling_spline_coupling(4,
    K=16, (128,128)) has exactly the FLAX parameter count + BN + SB records."""
    from zenflow_amd import _lib as L

    lib = L.load_library()
    nsc = (L.ZF_OP_NSC, 16, (128, 128))
    ops = [(L.ZF_OP_SHIFT_BOUNDS,)] + [nsc, (L.ZF_OP_ROLL,)] * 3 + [nsc]
    d = _desc(4, 0, ops)
    n = ctypes.c_int64()
    assert lib.zf_flow_plan(ctypes.byref(d), ctypes.byref(n)) == 0
    per_nsc = 4 * 2 + (2 * 128 + 128) + (128 * 128 + 128) + (128 * 94 + 94)
    assert n.value == 8 * 4 + 4 * per_nsc
    assert d.ops[0].off_sb == 0
    assert d.ops[1].off_bn == 32 and d.ops[1].off_w[0] == 40


@pytest.mark.parametrize(
    "D,ops,err",
    [
        (1, [(3, 16, (128,))], ValueError),  # NSC needs D >= 2
        (4, [(3, 0, (128,))], ValueError),  # knots < 1
        (4, [(3, 16, (5000,))], NotImplementedError),  # width > 4096 (257..4096 run layered)
        (4, [(9,)], ValueError),  # unknown op
    ],
)
def test_flow_plan_rejects(D, ops, err):
    from zenflow_amd import _lib as L

    d = _desc(D, 0, ops)
    n = ctypes.c_int64()
    rc = L.load_library().zf_flow_plan(ctypes.byref(d), ctypes.byref(n))
    with pytest.raises(err):
        L.check(rc, "zf_flow_plan")
    assert L.load_library().zf_last_error()


def test_no_gpu_fails_loudly(monkeypatch):
    """Without a GPU the product path raises instead of falling back to CPU."""
    from zenflow_amd import _lib as L

    if L.device_count() > 0:
        pytest.skip("a GPU is visible")
    monkeypatch.setattr(L, "_device_ready", False)
    with pytest.raises(RuntimeError, match="no HIP device"):
        L.ensure_device()
    import zenflow_amd.utils as u

    with pytest.raises(RuntimeError):
        u.rational_quadratic_spline_forward(np.zeros((1, 1)), np.ones((1, 1, 1)), np.ones((1, 1, 1)),
                                            np.ones((1, 1, 0)))


def test_header_constants_match_python():
    """Every `#define ZF_<NAME> <int>` of include/zenflow_amd.h that the
    Python side mirrors (`zenflow_amd._lib`) has the same value there."""
    from zenflow_amd import _lib as L

    hdr = (Path(__file__).resolve().parents[1] / "include" / "zenflow_amd.h").read_text()
    defs = dict(re.findall(r"^#define (ZF_[A-Z0-9_]+)\s+(-?\d+)\b", hdr, re.M))
    assert "ZF_KERNEL_LAYERED" in defs
    mirrored = [n for n in defs if hasattr(L, n)]
    assert len(mirrored) >= 20, mirrored
    for n in mirrored:
        assert getattr(L, n) == int(defs[n]), n


# ---------------------------------------------------------------------------
# Argument validation of the standalone entries: every check below returns
# before the first HIP call, so host pointers stand in for device ones.
# ---------------------------------------------------------------------------


def _host_ptr():
    buf = np.zeros(64, np.float32)
    return buf, buf.ctypes.data


def _rejected(rc, want):
    from zenflow_amd import _lib as L

    assert rc == want
    assert L.load_library().zf_last_error()


@pytest.mark.parametrize("K", [6144, 6145, 0])
def test_normalize_spline_params_rejects_k(K):
    """K = 6144 passes the K <= 6144 gate but leaves no room for one dx and one
    dy row (2 * 6145 floats > 12288): an error, not a division by zero rows."""
    from zenflow_amd import _lib as L

    buf, p = _host_ptr()
    _rejected(L.load_library().zf_normalize_spline_params(p, p, p, 3, K, None), -1)


@pytest.mark.parametrize("K", [6145, 0])
def test_softmax_with_threshold_rejects_k(K):
    from zenflow_amd import _lib as L

    buf, p = _host_ptr()
    _rejected(L.load_library().zf_softmax_with_threshold(p, p, 3, K, 1e-5, None), -1)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize(
    "M,N,K,rc",
    [
        (4, 2, 257, -1),
        (4, 2, 0, -1),
        (4, 0, 16, -1),
        (-1, 2, 16, -1),
        (4, 257, 16, -2),  # more items than one block's threads
        (4, 64, 64, -2),  # 64 * (3 * 65 + 1) = 12544 floats > 12288
        (4, 17, 255, -2),  # 17 * (3 * 257 + 1) = 13124
        (4, 256, 15, -2),  # 256 * (3 * 17 + 1) = 13312
    ],
)
def test_rqs_rejects_shapes(inverse, M, N, K, rc):
    from zenflow_amd import _lib as L

    lib = L.load_library()
    buf, p = _host_ptr()
    if inverse:
        got = lib.zf_rqs_inverse(p, p, p, p, p, M, N, K, None)
    else:
        got = lib.zf_rqs_forward(p, p, p, p, p, p, M, N, K, None)
    _rejected(got, rc)


@pytest.mark.parametrize(
    "N,ncols,ld,off,ws",
    [
        (8, 0, 4, 0, True),
        (8, 65, 70, 0, True),
        (8, 3, 4, 2, True),  # ld < ncols + col_offset
        (8, 3, 8, -1, True),
        (-1, 3, 3, 0, True),
        (8, 3, 3, 0, False),  # NULL workspace
    ],
)
def test_colstats_rejects(N, ncols, ld, off, ws):
    from zenflow_amd import _lib as L

    buf, p = _host_ptr()
    rc = L.load_library().zf_colstats(p, N, ncols, ld, off, None, None, p, p, p, p, p if ws else None, None)
    _rejected(rc, -1)


@pytest.mark.parametrize(
    "latent,param,N,D",
    [
        (0, 0.0, 4, 2),  # ZF_LATENT_NONE is not a distribution
        (5, 0.0, 4, 2),
        (-1, 0.0, 4, 2),
        (2, 0.5, 4, 2),  # Beta peakness < 1
        (2, float("nan"), 4, 2),
        (1, 0.0, 4, 0),
        (1, 0.0, -1, 2),
    ],
)
def test_latent_sample_rejects(latent, param, N, D):
    from zenflow_amd import _lib as L

    buf, p = _host_ptr()
    _rejected(L.load_library().zf_latent_sample(latent, param, 7, p, N, D, None), -1)
