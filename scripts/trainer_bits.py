"""sha256 of every output of every Trainer pass, one line per output:

    case call output sha256(bytes)

A host-only refactor of the trainer must leave every line as it is, so the
listing is compared between two builds of the library (``ZF_LIB`` names the one
to load; ``zenflow_amd.build --out`` builds a checkout into a second file):

    ZF_LIB=tune/libparent.so python scripts/trainer_bits.py > parent.txt
    python scripts/trainer_bits.py > tree.txt
    diff parent.txt tree.txt

The cases and row counts are chosen for the host branches of zf_train.hip:
``small`` x 3 (one leaf, the single-block BatchNorm kernels), ``cfg4`` x 128
with ``ZF_TRAIN_BN_SMALL`` 1 and 0 (C > 0; four leaves, the tree BatchNorm
path), ``odd`` x 300 (three hidden layers, eight leaves of 38 rows: the unfused
loss leaves; C = 3, truncated-normal latent), ``bounded`` x 256 (a leading
ShiftBounds) and ``cfg2`` x 4096 (128 leaves: the two-level tree).  Every group
of calls runs on a fresh trainer built from the same seeded case, with fixed
inputs.  GPU box only; a tool, not a test.

``--cases`` keeps the cases whose label starts with one of the given names;
``--delimit`` launches a one-row ``zf_latent_sample`` before and after every
call, a kernel no pass launches, and writes ``call <case> <call>`` / ``end`` on
stderr, so that a kernel trace of the run can be cut into calls.
"""

import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

CASES = [  # label, flowcases name, rows, ZF_TRAIN_BN_SMALL
    ("small/3", "small", 3, None),
    ("cfg4/128/bn_small=1", "cfg4", 128, "1"),
    ("cfg4/128/bn_small=0", "cfg4", 128, "0"),
    ("odd/300", "odd", 300, None),
    ("bounded/256", "bounded", 256, None),
    ("cfg2/4096", "cfg2", 4096, None),
]
SEED = 11


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", default="", help="comma-separated label prefixes (default: all)")
    ap.add_argument("--delimit", action="store_true", help="a one-row zf_latent_sample launch around every call")
    args = ap.parse_args()

    from tests.flowcases import _blob, _trainer, make_case
    from tests.sample_grad_oracle import make_inputs
    from zenflow_amd import _lib as L
    from zenflow_amd._lib import DeviceArray

    lib = L.load_library()
    mark = DeviceArray((1, 1))

    def env(name, value):
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value

    for label, name, N, bn_small in CASES:
        if args.cases and not any(label.startswith(p) for p in args.cases.split(",")):
            continue
        case = make_case(name, N=N, seed=SEED)
        C = case["cfg"]["C"]
        x, c = case["x"], case["c"]
        rng = np.random.default_rng(SEED)
        w = rng.exponential(1.0, N).astype(np.float32)
        if N >= 16:  # an eighth of the weights zero, a sixteenth negative
            w[rng.choice(N, N // 8, replace=False)] = 0.0
            w[rng.choice(N, N // 16, replace=False)] = -0.25
        cot = (rng.standard_normal(N) / N).astype(np.float32)
        z, gx, glq = make_inputs(case, N, SEED)
        xd = DeviceArray.from_numpy(np.ascontiguousarray(x))
        cd = None if c is None else DeviceArray.from_numpy(np.ascontiguousarray(c))
        cotd = DeviceArray.from_numpy(cot)

        def fresh(graph=None):
            """A trainer of this case; the library reads both switches when it is created."""
            env("ZF_TRAIN_BN_SMALL", bn_small)
            env("ZF_TRAIN_GRAPH", graph)
            return _trainer(case, N)

        def delimiter(line):
            if args.delimit:
                L.check(lib.zf_latent_sample(1, 0.0, 1, mark.ptr, 1, 1, L.stream()), "zf_latent_sample")
                L.synchronize()
                print(line, file=sys.stderr, flush=True)

        def call(what):
            delimiter(f"call {label} {what}")
            return what

        def out(what, **arrays):
            delimiter("end")
            for key, a in arrays.items():
                a = a.numpy() if isinstance(a, DeviceArray) else np.asarray(a)
                print(label, what, key, hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest(), flush=True)

        def loss_of(tr):
            return tr._loss.numpy()  # the device's fp64 value as it is

        # ---- loss_grad: plain, with d loss / d c, weighted
        tr = fresh()
        what = call("loss_grad")
        _, g = tr.loss_grad(x, c)
        out(what, loss=loss_of(tr), grad=g)
        if C:
            what = call("loss_grad(cond_grad)")
            _, g, gc = tr.loss_grad(x, c, cond_grad=True)
            out(what, loss=loss_of(tr), grad=g, gc=gc)
        what = call("loss_grad(w)")
        _, g = tr.loss_grad(x, c, w=w)
        out(what, loss=loss_of(tr), grad=g)

        # ---- step: captured (the default) and eager, plain and weighted
        for graph in (None, "0"):
            tr = fresh(graph)
            tag = "graph=default" if graph is None else "graph=0"
            for k in range(2):
                what = call(f"step[{tag}]#{k}")
                tr.step(x, c)
                out(what, loss=loss_of(tr))
            out(f"step[{tag}]", blob=_blob(tr))
            for k in range(2):
                what = call(f"step(w)[{tag}]#{k}")
                tr.step(x, c, w=w)
                out(what, loss=loss_of(tr))
            out(f"step(w)[{tag}]", blob=_blob(tr))
        if C:
            tr = fresh()
            what = call("step(cond_grad)")
            gc = tr.step(x, c, cond_grad=True)
            out(what, loss=loss_of(tr), gc=gc, blob=_blob(tr))

        # ---- forward + backward in train and eval mode, then apply_gradient
        for train in (True, False):
            tr = fresh()
            mode = "train" if train else "eval"
            what = call(f"forward({mode})")
            lp = tr.forward(x, c, train=train)
            out(what, log_prob=lp, blob=_blob(tr))
            what = call(f"backward({mode})")
            if C:
                g, gc = tr.backward(cot, cond_grad=True)
                out(what, grad=g, gc=gc)
            else:
                g = tr.backward(cot)
                out(what, grad=g)
            what = call(f"apply_gradient({mode})")
            tr.apply_gradient()
            out(what, blob=_blob(tr))

        # ---- log_prob_vjp without and with a cotangent
        tr = fresh()
        for ct_name, ct in (("ones", None), ("cot", cotd)):
            what = call(f"log_prob_vjp({ct_name})")
            lp, dx, dc = tr.log_prob_vjp(xd, cd, ct)
            out(what, log_prob=lp, dx=dx, **({"dc": dc} if C else {}))

        # ---- sample_forward + sample_backward; bounded: after one step, so that
        # the stored bounds are what a train-mode pass left
        tr = fresh()
        if name == "bounded":
            call("step(before sample)")
            tr.step(x, c)
        cs = c if C else N
        what = call("sample_forward#0")
        xs, lq = tr.sample_forward(cs, z=z)
        out(what, x=xs, log_q=lq)
        what = call("sample_backward(glog_q=None)")
        out(what, grad=tr.sample_backward(gx))
        what = call("sample_forward#1")
        xs, lq = tr.sample_forward(cs, z=z)
        out(what, x=xs, log_q=lq)
        what = call("sample_backward(glog_q)")
        res = tr.sample_backward(gx, glq, cond_grad=bool(C), latent_grad=True)
        out(what, **dict(zip(["grad"] + (["gc"] if C else []) + ["gz"], res)))
        del tr
    return 0


if __name__ == "__main__":
    sys.exit(main())
