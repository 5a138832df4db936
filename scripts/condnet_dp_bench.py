"""What data parallelism of the ConditionTrainer costs, at the shape of
examples/deep_set.ipynb (scripts/condnet_bench.py: 50,000 x 2 element rows,
1,000 sets, Phi = BatchNorm, 3 x Dense(128) swish, Dense(8), Dropout(0.3),
sum).  GPU box only; not part of bench.py's contract.  The timed step is

    zf_condnet_forward(train, update_stats) ; zf_condnet_backward ; zf_condnet_apply_gradient

on device-resident inputs and buffers allocated once, by device events.

(a) ``--ab PARENT_LIB``: one device must not pay.  The step through the
    existing entries with this tree's library and with the parent commit's
    (built on its own), a fresh process per library and round, alternated;
    each process also prints the sha256 of the blob after five steps.  The
    rounds and their summary go to ``--out`` (profiles/condnet_dp_ab.txt).
(b) ``--dp``: what the exchanges cost.  Two ranks, one GPU each, over
    dist.RcclCommunicator at 2 x 25,000 rows (zf_condnet_forward_shard)
    against one device at 50,000 rows, alternated rounds; the ratio goes to
    ``--out`` (profiles/condnet_dp_bench.jsonl).  Needs two GPUs and librccl:
    otherwise one line says "not measured".  The HostAllgather transport of
    the tests is not timed.

    python scripts/condnet_dp_bench.py --ab /path/to/parent/libzenflow_amd.so [--rounds 3]
    python scripts/condnet_dp_bench.py --dp [--rounds 3]
"""

import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

ROWS, SETS = 50_000, 1_000


def leg_step(args):
    """One process: the timed step on this rank's rows; one JSON line on stdout."""
    import zenflow_amd as zf
    from scripts.condnet_bench import notebook_sets
    from scripts.input_grad_bench import timed
    from zenflow_amd import _lib as L
    from zenflow_amd import nn
    from zenflow_amd._lib import DeviceArray

    world, rank, comm, rdzv = 1, 0, None, None
    if args.leg == "rank":
        from zenflow_amd.dist import RcclCommunicator
        from zenflow_amd.launch import FileRendezvous

        rdzv = FileRendezvous.from_env(timeout=120)
        world, rank = rdzv.world, rdzv.rank
        comm = RcclCommunicator(rank, world, lambda u: rdzv.broadcast_bytes(u, tag="rccl_uid"))
    rows, sets = ROWS // world, SETS // world
    if world == 1:
        X, _, off = notebook_sets(np.random.default_rng(1))
    else:  # this rank's half: the same distribution of lengths, scaled to fill 90% of its rows
        rng = np.random.default_rng(1 + rank)
        n = rng.exponential(size=sets)
        n = (n * (0.9 * rows - sets) / n.sum() + 1).astype(int)
        off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        X = np.zeros((rows, 2), np.float32)
        X[: off[-1]] = rng.normal(size=(int(off[-1]), 2))
    net = nn.ConditionNet(8, layers=(128,) * 3, dropout=0.3, pool="sum")
    v = net.init(zf.PRNGKey(0), X, off)
    ct = nn.ConditionTrainer(net, v, 2, rows, sets_max=sets, comm=comm)
    Xd, od = DeviceArray.from_numpy(X), DeviceArray.from_numpy(off)
    gcd = DeviceArray.from_numpy(np.random.default_rng(2).standard_normal((sets, 8)).astype(np.float32))
    cd = DeviceArray((sets, 8))
    lib, st = L.load_library(), L.stream()
    seed = [0]

    def step():
        seed[0] += 1
        if world == 1:
            L.check(lib.zf_condnet_forward(ct.handle, Xd.ptr, rows, od.ptr, sets, 1, 1, seed[0], cd.ptr, st), "forward")
        else:
            L.check(lib.zf_condnet_forward_shard(ct.handle, Xd.ptr, rows, ROWS, rank * rows, od.ptr, sets, 1, 1,
                                                 seed[0], cd.ptr, st), "forward_shard")
        L.check(lib.zf_condnet_backward(ct.handle, gcd.ptr, None, st), "backward")
        L.check(lib.zf_condnet_apply_gradient(ct.handle, None, st), "apply_gradient")

    for _ in range(5):
        step()
    digest = hashlib.sha256(ct._h.blob().tobytes()).hexdigest()[:16]
    ms, calls = timed(step, args.min_seconds)
    rec = {"leg": args.leg, "world": world, "rank": rank, "rows": rows, "sets": sets, "step_ms": round(ms, 5),
           "calls": calls, "blob_after_5_steps": digest}
    if rdzv is not None:
        rec["step_ms"] = round(rdzv.max(ms, "ms"), 5)  # the slowest rank
        rdzv.close()
        comm.close()
    if rank == 0:
        print(json.dumps(rec), flush=True)


def _child(args, leg, env=None):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--min-seconds",
                          str(args.min_seconds)], env=env, check=True, capture_output=True, text=True, cwd=ROOT).stdout
    return json.loads(out.strip().splitlines()[-1])


def run_ab(args):
    parent = os.path.abspath(args.ab)
    envs = {"parent": dict(os.environ, ZF_LIB=parent, ZF_ALLOW_MISSING_SYMBOLS="1"), "this": dict(os.environ)}
    lines = ["scripts/condnet_dp_bench.py --ab: forward + backward + apply_gradient of the ConditionTrainer through "
             "the existing entries,", f"{ROWS} x 2 rows in {SETS} sets (the notebook's shape), one MI355X, a fresh "
             "process per library and round, alternated"]
    ms = {"parent": [], "this": []}
    digests = set()
    for rnd in range(args.rounds):
        for name in ("parent", "this"):
            rec = _child(args, "one", envs[name])
            ms[name].append(rec["step_ms"])
            digests.add(rec["blob_after_5_steps"])
            lines += [f"round {rnd} {name}", json.dumps(rec)]
            print(lines[-2], lines[-1], flush=True)
    lines.append("")
    for name in ("parent", "this"):
        lines.append(f"{name:6s} ms/step {ms[name]} median {statistics.median(ms[name]):.5f} "
                     f"range {min(ms[name])}-{max(ms[name])}")
    mp, mt = statistics.median(ms["parent"]), statistics.median(ms["this"])
    inside = min(ms["parent"]) <= mt <= max(ms["parent"])
    lines.append(f"median difference {100 * (mt / mp - 1):+.2f}% (the parent's own round-to-round range is "
                 f"{100 * (max(ms['parent']) - min(ms['parent'])) / mp:.2f}%); this tree's median lies "
                 f"{'inside' if inside else 'below' if mt < min(ms['parent']) else 'ABOVE'} the parent's range; "
                 f"the blob after five steps is {'the same to the last bit' if len(digests) == 1 else 'DIFFERENT'}.")
    lines.append("Parent = the commit before this change, built on its own.")
    with open(args.out or os.path.join(ROOT, "profiles", "condnet_dp_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-5:]))


def run_dp(args):
    out = args.out or os.path.join(ROOT, "profiles", "condnet_dp_bench.jsonl")
    # counted in a child: this process must not hold the GPU when it starts the ranks
    n = int(subprocess.run([sys.executable, "-c", "from zenflow_amd import _lib as L; print(L.device_count() if "
                            "L.load_library().zf_rccl_available() else 0)"], capture_output=True, text=True,
                           cwd=ROOT).stdout.strip() or 0)
    recs = []
    if n < 2:
        recs.append({"what": "rccl two ranks against one device", "result": "not measured",
                     "why": "needs two GPUs and librccl"})
    else:
        env = dict(os.environ)
        env.pop("ZF_DEVICE", None)
        for rnd in range(args.rounds):
            one = _child(args, "one")
            two = subprocess.run([sys.executable, "-c", "import sys; from zenflow_amd.launch import spawn; "
                                  f"sys.exit(spawn(2, [{os.path.abspath(__file__)!r}, '--leg', 'rank', "
                                  f"'--min-seconds', '{args.min_seconds}'], timeout=300))"], env=env, check=True,
                                 capture_output=True, text=True, cwd=ROOT).stdout
            two = json.loads(two.strip().splitlines()[-1])
            recs.append({"what": "rccl two ranks against one device", "round": rnd, "one_device_ms": one["step_ms"],
                         "two_ranks_ms": two["step_ms"], "two_over_one": round(two["step_ms"] / one["step_ms"], 4)})
    with open(out, "w") as f:
        for rec in recs:
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", default="", help="the parent commit's libzenflow_amd.so")
    ap.add_argument("--dp", action="store_true")
    ap.add_argument("--leg", default="", help="one | rank (a child process of --ab / --dp)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.leg:
        leg_step(args)
    elif args.ab:
        run_ab(args)
    elif args.dp:
        run_dp(args)
    else:
        ap.error("one of --ab, --dp")


if __name__ == "__main__":
    main()
