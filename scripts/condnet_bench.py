"""Times of the conditioning network (zenflow_amd.nn, zf_condnet_*) at the
shape of examples/deep_set.ipynb, beside the way the example ran before it
existed, and of the segment sum alone.  GPU box only; not part of bench.py's
contract.

notebook    50,000 x 2 element rows (padded), 1,000 sets with the notebook's
            length distribution (``generate``), Phi = BatchNorm, 3 x Dense(128)
            swish, Dense(8), Dropout(0.3), sum; the flow
            rolling_spline_coupling(2, layers=(128,) * 6) on 1,000 rows.
            ``forward``, ``forward + backward`` and ``apply_gradient`` of the
            ConditionTrainer on device-resident inputs by device events (the
            backward's time is the difference of the first two), and the joint
            step ``ct.forward; tr.step(cond_grad=True); ct.step`` as one leg.
            ``joint_host``: the same joint step with phi in NumPy on the host
            (forward, hand-written chain rule, SGD update), c and gc crossing
            PCIe every step — the host clock around whole steps, each of which
            ends in the device-to-host copy of gc.
segment     zf_segment_sum alone on 2^24 x 8 floats (537 MB, past the
            Infinity Cache): evenly loaded sets of 256 rows, and the same
            bytes with one set holding half the rows; bytes read over time as
            a fraction of the 6.29 TB/s float4 copy (MI355X_MICROARCH.md), and
            the skewed / even ratio.

The legs are alternated round by round in one process.  One JSON line per
(leg group, round) goes to ``--out`` (default profiles/condnet_bench.jsonl).

    python scripts/condnet_bench.py [--rounds 3] [--only notebook|segment]
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from scripts.input_grad_bench import timed

COPY_RATE = 6.29e12  # bytes / s, float4 copy


def notebook_sets(rng, size=1000, padded=50_000):
    """``generate`` / ``preprocess`` of the notebook: set lengths, CSR offsets, padded X."""
    n = rng.exponential(size=size)
    n *= 400 / np.max(n)
    n = (n + 1).astype(int)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    assert off[-1] <= padded
    X = np.zeros((padded, 2), np.float32)
    X[: off[-1]] = rng.normal(size=(int(off[-1]), 2))
    Y = rng.normal(np.sqrt(n), 1, size=(2, size)).T.astype(np.float32)
    return X, Y, off


class HostPhi:
    """Phi on the host in NumPy: train-mode forward, the chain rule by hand, SGD."""

    def __init__(self, variables, offsets, rate, lr=1e-3):
        p = variables["params"]
        self.scale, self.bias = p["BatchNorm_0"]["scale"].copy(), p["BatchNorm_0"]["bias"].copy()
        blk = p["NNBlock_0"]
        self.W = [blk[f"Dense_{l}"]["kernel"].copy() for l in range(len(blk))]
        self.b = [blk[f"Dense_{l}"]["bias"].copy() for l in range(len(blk))]
        self.off, self.rate, self.lr = offsets, rate, lr
        self.starts = offsets[:-1]

    def forward(self, X, rng):
        mean, var = X.mean(axis=0), X.var(axis=0)
        self.rstd = 1 / np.sqrt(var + 1e-5)
        self.uhat = (X - mean) * self.rstd
        h = self.uhat * self.scale + self.bias
        self.acts, self.pre = [h], []
        for l in range(len(self.W) - 1):
            z = h @ self.W[l] + self.b[l]
            self.pre.append(z)
            h = z / (1 + np.exp(-z))
            self.acts.append(h)
        h = h @ self.W[-1] + self.b[-1]
        self.keep = rng.random(h.shape, dtype=np.float32) >= self.rate
        d = np.where(self.keep, h / np.float32(1 - self.rate), np.float32(0))
        n = int(self.off[-1])
        return np.add.reduceat(d[:n], self.starts, axis=0).astype(np.float32)

    def step(self, gc):
        n = int(self.off[-1])
        g = np.zeros((len(self.keep), gc.shape[1]), np.float32)
        g[:n] = np.repeat(gc, np.diff(self.off), axis=0)
        g = np.where(self.keep, g / np.float32(1 - self.rate), np.float32(0))
        for l in range(len(self.W) - 1, -1, -1):
            gw, gb = self.acts[l].T @ g, g.sum(axis=0)
            g_in = g @ self.W[l].T
            self.W[l] -= self.lr * gw
            self.b[l] -= self.lr * gb
            if l > 0:
                z = self.pre[l - 1]
                s = 1 / (1 + np.exp(-z))
                g = g_in * (s + z * s * (1 - s))
            else:
                g = g_in
        self.scale -= self.lr * (g * self.uhat).sum(axis=0)
        self.bias -= self.lr * g.sum(axis=0)


def bench_notebook(args, lines):
    import zenflow_amd as zf
    from zenflow_amd import _lib as L
    from zenflow_amd import nn
    from zenflow_amd._lib import DeviceArray
    from zenflow_amd.bijectors import rolling_spline_coupling
    from zenflow_amd.train import Trainer

    rng = np.random.default_rng(1)
    X, Y, off = notebook_sets(rng)
    S, rows = len(off) - 1, len(X)
    net = nn.ConditionNet(8, layers=(128,) * 3, dropout=0.3, pool="sum")
    v = net.init(zf.PRNGKey(0), X, off)
    flow = zf.Flow(rolling_spline_coupling(2, layers=(128,) * 6))
    fv = flow.init(zf.PRNGKey(1), Y, np.zeros((S, 8), np.float32))

    ct = nn.ConditionTrainer(net, v, 2, rows, sets_max=S)
    tr, tr_h = Trainer(flow, fv, 2, 8, S), Trainer(flow, fv, 2, 8, S)  # beside the device phi, beside the host phi
    host = HostPhi(v, off, 0.3)
    Xd, od, Yd = DeviceArray.from_numpy(X), DeviceArray.from_numpy(off), DeviceArray.from_numpy(Y)
    gcd = DeviceArray.from_numpy(rng.standard_normal((S, 8)).astype(np.float32))
    # the device legs call the C ABI on buffers allocated once, as scripts/custom_loss_bench.py does
    lib, st = L.load_library(), L.stream()
    cd, gc, loss = DeviceArray((S, 8)), DeviceArray((S, 8)), DeviceArray((1,), np.float64)
    seed = [0]

    def forward():
        seed[0] += 1
        L.check(lib.zf_condnet_forward(ct.handle, Xd.ptr, rows, od.ptr, S, 1, 1, seed[0], cd.ptr, st), "forward")

    def forward_backward():
        forward()
        L.check(lib.zf_condnet_backward(ct.handle, gcd.ptr, None, st), "backward")

    def apply_gradient():
        L.check(lib.zf_condnet_apply_gradient(ct.handle, None, st), "apply_gradient")

    def joint():
        forward()
        L.check(lib.zf_trainer_step_cond_shard(tr.handle, Yd.ptr, cd.ptr, S, S, loss.ptr, gc.ptr, st), "step")
        L.check(lib.zf_condnet_backward(ct.handle, gc.ptr, None, st), "backward")
        apply_gradient()

    hrng = np.random.default_rng(2)

    def joint_host():
        c = host.forward(X, hrng)
        gc = tr_h.step(Y, c, cond_grad=True)
        host.step(gc)

    forward_backward()  # a gradient for apply_gradient alone
    for rnd in range(args.rounds):
        rec = {"what": "notebook", "rows": rows, "sets": S, "round": rnd}
        for leg, fn in (("forward", forward), ("forward_backward", forward_backward),
                        ("apply_gradient", apply_gradient), ("joint_device", joint)):
            ms, calls = timed(fn, args.min_seconds)
            rec[leg + "_ms"], rec[leg + "_calls"] = round(ms, 5), calls
        rec["backward_ms"] = round(rec["forward_backward_ms"] - rec["forward_ms"], 5)
        joint_host()
        t0, n = time.perf_counter(), 0
        while time.perf_counter() - t0 < args.min_seconds or n < 3:
            joint_host()
            n += 1
        rec["joint_host_ms"], rec["joint_host_calls"] = round((time.perf_counter() - t0) * 1e3 / n, 5), n
        rec["host_over_device"] = round(rec["joint_host_ms"] / rec["joint_device_ms"], 3)
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    L.synchronize()


def bench_segment(args, lines):
    from zenflow_amd import _lib as L
    from zenflow_amd._lib import DeviceArray

    lib = L.load_library()
    rows, F, per = 1 << 24, 8, 256
    hd = DeviceArray.from_numpy(np.random.default_rng(3).standard_normal((rows, F), dtype=np.float32))
    even = np.arange(0, rows + 1, per, dtype=np.int64)
    skew = np.concatenate([[0], np.arange(rows // 2, rows + 1, per)]).astype(np.int64)
    legs = {}
    for name, off in (("even", even), ("skewed", skew)):
        S = len(off) - 1
        od, out = DeviceArray.from_numpy(off), DeviceArray((S, F))
        ws = DeviceArray((lib.zf_segment_workspace_bytes(rows, S, F),), np.uint8)

        def run(od=od, out=out, ws=ws, S=S):
            L.check(lib.zf_segment_sum(hd.ptr, rows, F, od.ptr, S, 0.0, 0, out.ptr, None, ws.ptr, L.stream()),
                    "zf_segment_sum")
        legs[name] = (run, S)
    nbytes = rows * F * 4
    for rnd in range(args.rounds):
        rec = {"what": "segment_sum", "rows": rows, "F": F, "bytes_read": nbytes, "round": rnd}
        for name, (run, S) in legs.items():
            ms, calls = timed(run, args.min_seconds)
            rec[name + "_sets"], rec[name + "_ms"], rec[name + "_calls"] = S, round(ms, 5), calls
            rec[name + "_fraction_of_copy_rate"] = round(nbytes / (ms * 1e-3) / COPY_RATE, 4)
        rec["skewed_over_even"] = round(rec["skewed_ms"] / rec["even_ms"], 4)
        lines.append(rec)
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--only", default="", help="notebook | segment")
    ap.add_argument("--out", default=os.path.join("profiles", "condnet_bench.jsonl"))
    args = ap.parse_args()
    lines = []
    if args.only in ("", "notebook"):
        bench_notebook(args, lines)
    if args.only in ("", "segment"):
        bench_segment(args, lines)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
