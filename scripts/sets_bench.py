"""What keeping a deep-set data set resident saves: an epoch of
``zenflow_amd.train.train_sets``' steps with every ragged minibatch gathered on
the device (zf_segment_take), beside the same loop with ``X[rows]`` /
``Y[take]`` gathered by NumPy on the host and uploaded per step — the loop the
primitives allowed before the entry existed.  GPU box only; not part of
bench.py's contract.

epoch       65,536 sets of 1 - 64 elements, in_dim 2; Phi = BatchNorm, 3 x
            Dense(128) swish, Dense(8), sum; the flow
            rolling_spline_coupling(2, knots=8, layers=(32, 32)); batch_sets
            1,024, so 64 steps an epoch.  ``device``: nn.segment_take,
            nn.take_rows, ct.forward, tr.step(cond_grad=True), ct.step on the
            resident copy.  ``host``: the same three trainer calls on a NumPy
            gather (vectorised: one fancy index per batch) uploaded with
            DeviceArray.from_numpy.  Each leg is a whole epoch, timed by device
            events and by the host clock around it (it ends in a synchronise);
            the two legs alternate round by round and share the permutations.
take        zf_segment_take alone, on buffers allocated once: one batch (1,024
            of the 65,536 sets) and a whole permutation (all 65,536), F = 2;
            bytes read plus bytes written over time, as a fraction of the 6.29
            TB/s float4 copy (MI355X_MICROARCH.md).

One JSON line per (group, round) and a closing line of medians go to ``--out``
(default profiles/sets_train_bench.jsonl).

    python scripts/sets_bench.py [--rounds 5] [--only epoch|take]
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
SETS, LONGEST, IN_DIM, BATCH_SETS = 65_536, 64, 2, 1024


def make_sets(rng):
    n = rng.integers(1, LONGEST + 1, SETS)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    X = rng.standard_normal((int(off[-1]), IN_DIM)).astype(np.float32)
    Y = (0.3 * np.sqrt(n)[:, None] * np.array([1.0, -1.0]) + 0.2 * rng.standard_normal((SETS, 2))).astype(np.float32)
    return X, off, Y


def bench_epoch(args, lines):
    import zenflow_amd as zf
    from zenflow_amd import _lib as L
    from zenflow_amd import nn
    from zenflow_amd._lib import DeviceArray
    from zenflow_amd.bijectors import rolling_spline_coupling
    from zenflow_amd.train import Trainer, plan_set_batches

    X, off, Y = make_sets(np.random.default_rng(1))
    lengths = np.diff(off)
    sizes, sets_max, rows_max = plan_set_batches(off, BATCH_SETS)
    phi = nn.ConditionNet(8, layers=(128,) * 3, pool="sum")
    flow = zf.Flow(rolling_spline_coupling(2, knots=8, layers=(32, 32)))
    pv = phi.init(zf.PRNGKey(0), X, off)
    fv = flow.init(zf.PRNGKey(1), Y[:1], np.zeros((1, 8), np.float32))
    # one pair of trainers per leg: both legs train, neither disturbs the other
    legs = {name: (Trainer(flow, fv, 2, 8, sets_max), nn.ConditionTrainer(phi, pv, IN_DIM, rows_max, sets_max=sets_max))
            for name in ("device", "host")}
    Xd, off_d, Yd = DeviceArray.from_numpy(X), DeviceArray.from_numpy(off), DeviceArray.from_numpy(Y)
    step = {"device": 0, "host": 0}

    def device_epoch(epoch):
        tr, ct = legs["device"]
        perm = np.random.default_rng([0, epoch]).permutation(SETS)
        take_d = DeviceArray.from_numpy(perm.astype(np.int64))
        first = 0
        for n in sizes:
            take_b = take_d.rows(first, first + n)
            xb, ob = nn.segment_take(Xd, off_d, take_b, rows=int(lengths[perm[first:first + n]].sum()))
            yb = nn.take_rows(Yd, take_b)
            c = ct.forward(xb, ob, seed=step["device"])
            ct.step(tr.step(yb, c, cond_grad=True))
            step["device"] += 1
            first += n

    def host_epoch(epoch):
        tr, ct = legs["host"]
        perm = np.random.default_rng([0, epoch]).permutation(SETS)
        first = 0
        for n in sizes:
            sets = perm[first:first + n]
            loc = np.concatenate([[0], np.cumsum(lengths[sets])]).astype(np.int64)
            rows = np.repeat(off[sets] - loc[:-1], lengths[sets]) + np.arange(loc[-1])
            xb, ob, yb = DeviceArray.from_numpy(X[rows]), DeviceArray.from_numpy(loc), DeviceArray.from_numpy(Y[sets])
            c = ct.forward(xb, ob, seed=step["host"])
            ct.step(tr.step(yb, c, cond_grad=True))
            step["host"] += 1
            first += n

    def one(fn, epoch):
        L.synchronize()
        a, b = L.Event(), L.Event()
        t0 = time.perf_counter()
        a.record()
        fn(epoch)
        b.record()
        b.synchronize()
        L.synchronize()
        return a.elapsed_ms(b), (time.perf_counter() - t0) * 1e3

    device_epoch(0)  # warm-up: code objects, the allocator
    host_epoch(0)
    recs = []
    for rnd in range(args.rounds):
        rec = {"what": "epoch", "sets": SETS, "rows": int(off[-1]), "batch_sets": BATCH_SETS, "steps": len(sizes),
               "round": rnd}
        order = (("device", device_epoch), ("host", host_epoch)) if rnd % 2 == 0 else (
            ("host", host_epoch), ("device", device_epoch))
        for name, fn in order:
            ev, wall = one(fn, 1 + rnd)
            rec[name + "_event_ms"], rec[name + "_wall_ms"] = round(ev, 3), round(wall, 3)
        rec["host_over_device_wall"] = round(rec["host_wall_ms"] / rec["device_wall_ms"], 4)
        rec["losses"] = [round(legs[k][0].last_loss(), 6) for k in ("device", "host")]
        recs.append(rec)
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    med = {"what": "epoch_medians", "rounds": args.rounds}
    for key in ("device_event_ms", "device_wall_ms", "host_event_ms", "host_wall_ms"):
        med[key] = round(float(np.median([r[key] for r in recs])), 3)
    med["host_over_device_wall"] = round(med["host_wall_ms"] / med["device_wall_ms"], 4)
    lines.append(med)
    print(json.dumps(med), flush=True)


def bench_take(args, lines):
    from zenflow_amd import _lib as L
    from zenflow_amd._lib import DeviceArray

    lib = L.load_library()
    X, off, _ = make_sets(np.random.default_rng(1))
    lengths = np.diff(off)
    rows, S = len(X), SETS
    Xd, off_d = DeviceArray.from_numpy(X), DeviceArray.from_numpy(off)
    perm = np.random.default_rng([0, 0]).permutation(S).astype(np.int64)
    legs = {}
    for name, n in (("batch", BATCH_SETS), ("permutation", S)):
        take = perm[:n]
        rows_out = int(lengths[take].sum())
        td, out, oo = DeviceArray.from_numpy(take), DeviceArray((rows_out, IN_DIM)), DeviceArray((n + 1,), np.int64)
        ws = DeviceArray((lib.zf_segment_take_workspace_bytes(S, n),), np.uint8)

        def run(td=td, out=out, oo=oo, ws=ws, n=n, rows_out=rows_out):
            L.check(lib.zf_segment_take(Xd.ptr, rows, IN_DIM, off_d.ptr, S, td.ptr, n, rows_out, out.ptr, oo.ptr,
                                        ws.ptr, L.stream()), "zf_segment_take")
        legs[name] = (run, n, rows_out)
    recs = []
    for rnd in range(args.rounds):
        rec = {"what": "segment_take", "sets": S, "rows": rows, "F": IN_DIM, "round": rnd}
        for name, (run, n, rows_out) in legs.items():
            ms, calls = timed(run, args.min_seconds)
            moved = 2 * rows_out * IN_DIM * 4  # the rows, read and written
            rec[name + "_take_n"], rec[name + "_rows_out"], rec[name + "_bytes_moved"] = n, rows_out, moved
            rec[name + "_ms"], rec[name + "_calls"] = round(ms, 5), calls
            rec[name + "_gb_per_s"] = round(moved / (ms * 1e-3) / 1e9, 2)
            rec[name + "_fraction_of_copy_rate"] = round(moved / (ms * 1e-3) / COPY_RATE, 5)
        recs.append(rec)
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    med = {"what": "segment_take_medians", "rounds": args.rounds}
    for name in legs:
        for key in ("_ms", "_gb_per_s", "_fraction_of_copy_rate"):
            med[name + key] = round(float(np.median([r[name + key] for r in recs])), 5)
    lines.append(med)
    print(json.dumps(med), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--only", default="", help="epoch | take")
    ap.add_argument("--out", default=os.path.join("profiles", "sets_train_bench.jsonl"))
    args = ap.parse_args()
    lines = []
    if args.only in ("", "epoch"):
        bench_epoch(args, lines)
    if args.only in ("", "take"):
        bench_take(args, lines)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
