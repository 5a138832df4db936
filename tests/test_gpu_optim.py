"""Optimiser chains on the device (zenflow_amd/optim.py; sumsq_leaf_kernel,
opt_prologue_kernel and chain_update_kernel of zf_optim.hip) against the
float64 reference of tests/optim_ref.py, teacher forced as
tests/test_gpu_train_trajectory.py::test_teacher_forced_trajectory: 12 steps
over ``train_ref.trajectory_batches()`` on the 256-row cases, the handle
starting from ShiftBounds statistics at +inf / -inf.

Per step t: theta_t and the GPU's gradient g_t (loss_grad) ->
``chain_reference``; ``step()`` must land within ``chain_tolerance`` of it on
every parameter (tests/test_optim_ref_host.py shows that a correct fp32
evaluation does and seven wrong ones do not); the loss is the oracle's, every
statistic in the blob after the step is the oracle's new batch_stats, and no
other entry changes.  Every case runs with the captured step graph and
eagerly, and the two end with the same bits."""

import ctypes as ct
import functools

import numpy as np
import pytest

import zenflow_amd.optim as optim
from oracle import zf_oracle as O
from tests import optim_ref as R
from tests import train_ref as TR
from tests.flowcases import build_flow, make_case
from tests.test_gpu_train_trajectory import _bits, _blob, _leaves, _stat_index

pytestmark = pytest.mark.gpu

SEEDS = {"small": 101, "cfg4": 102, "relu": 103, "bounded": 104, "odd": 105}
SCHED = optim.warmup_cosine_decay_schedule(1e-3, 1e-2, 4, 12, 1e-4)


def _record(rec):
    from tests.test_gpu_flow import _append_record

    _append_record("optim_trajectory.jsonl", rec)


def _trainer(case, optimizer, batch_max=TR.TRAJ_BATCH, variables=None):
    from zenflow_amd.train import Trainer

    cfg = case["cfg"]
    flow = build_flow(cfg)
    flow.latent._dim = cfg["D"]
    v = TR.reset_shift_bounds(case["variables"]) if variables is None else variables
    return Trainer(flow, v, cfg["D"], cfg["C"], batch_max, optimizer=optimizer)


@functools.lru_cache(maxsize=None)
def _first_norm(name):
    """float64 norm of the first trajectory step's gradient (from the GPU)."""
    case = make_case(name, N=TR.TRAJ_ROWS, seed=SEEDS[name])
    lo, hi = TR.trajectory_batches()[0]
    tr = _trainer(case, None)
    _, g = tr.loss_grad(case["x"][lo:hi], None if case["c"] is None else case["c"][lo:hi])
    return float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))


def _forced(name, chain, oracle=True, per_step=None, label=""):
    """The teacher-forced trajectory of ``chain`` on case ``name``; returns
    ``(final blob, worst error / tolerance, ambiguous lion elements)``.
    ``oracle``: also the loss / statistics / untouched-entries checks.
    ``per_step(t, tr, g, state, blob0, blob1, dmask)``: further checks."""
    case = make_case(name, N=TR.TRAJ_ROWS, seed=SEEDS[name])
    tr = _trainer(case, chain)
    prog = tr.program
    mask = prog.param_mask == 1
    dmask = optim.lower_mask(chain.mask(), prog).astype(bool) if chain.mask() is not None else None
    index = _stat_index(prog)
    stat_entries = np.zeros(mask.shape, bool)
    for ix in index.values():
        stat_entries[ix] = True
    state = R.chain_state(chain, mask)
    worst, amb_total = 0.0, 0
    for t, (lo, hi) in enumerate(TR.trajectory_batches(), start=1):
        x = case["x"][lo:hi]
        c = None if case["c"] is None else case["c"][lo:hi]
        blob0 = _blob(tr)
        loss, g = tr.loss_grad(x, c)
        assert np.all(g[~mask] == 0)
        tr.step(x, c)
        assert tr.last_loss() == loss, f"step {t}: step() and loss_grad() losses differ"
        blob1 = _blob(tr)

        ratio, state, amb = R.chain_check(blob1, blob0, g, state, t - 1, chain, dmask)
        amb_total += amb
        over = ratio > 1.0
        print(f"{name}{label} step {t}: worst parameter error / tolerance {ratio.max():.3f}, ambiguous {amb}")
        assert not over.any(), (f"step {t}: {over.sum()} of {mask.sum()} parameters outside the tolerance, worst "
                                f"error / tolerance {ratio.max():.3g} at blob offset {int(np.argmax(ratio))}")
        worst = max(worst, float(ratio.max()))
        if per_step is not None:
            per_step(t, tr, g, state, blob0, blob1, dmask)
        if not oracle:
            continue
        v = prog.blob_to_variables(blob0)
        variables = {"params": {"bijector": v["params"]}, "batch_stats": {"bijector": v["batch_stats"]}}
        lp, ns = O.flow_log_prob(case["model"], variables, x.astype(np.float64),
                                 None if c is None else c.astype(np.float64), train=True, dtype=np.float64)
        assert loss == pytest.approx(float(-lp.mean()), rel=2e-5, abs=2e-5), f"step {t}"
        new = dict(_leaves(ns))
        assert set(new) == set(index)
        for path, ix in index.items():
            np.testing.assert_allclose(blob1[ix].astype(np.float64), np.asarray(new[path], np.float64).reshape(-1),
                                       rtol=2e-5, atol=1e-6, err_msg=f"step {t}: {'/'.join(path)}")
        rest = ~mask & ~stat_entries
        assert np.array_equal(_bits(blob1)[rest], _bits(blob0)[rest]), f"step {t}: an entry that is neither changed"
    assert tr.opt_state()["count"] == TR.TRAJ_STEPS
    return _blob(tr), worst, amb_total


def _both_modes(name, chain, monkeypatch, per_step=None, label=""):
    """Graph (all checks) and eager (parameters only): the same bits after 12 steps."""
    monkeypatch.setenv("ZF_TRAIN_GRAPH", "1")
    bg, wg, ag = _forced(name, chain, True, per_step, label + "/graph")
    monkeypatch.setenv("ZF_TRAIN_GRAPH", "0")
    be, we, ae = _forced(name, chain, False, per_step, label + "/eager")
    assert np.array_equal(_bits(bg), _bits(be)), f"{np.sum(_bits(bg) != _bits(be))} entries differ graph vs eager"
    _record({"test": "chain_teacher_forced", "case": name + label, "chain": repr(chain), "steps": TR.TRAJ_STEPS,
             "param_worst_err_over_tol": max(wg, we), "lion_ambiguous_elements": ag})
    return bg


def test_small_sgd_warmup_cosine(monkeypatch):
    """sgd with nesterov momentum on a warm-up + cosine schedule: the learning
    rate each step used is the host schedule's, rounded once to float; the run
    crosses the join (count 4) and reaches the end value (count 12 is past the
    last step; count 11 is the last one used)."""
    chain = optim.sgd(SCHED, momentum=0.8, nesterov=True)
    lrs = []

    def per_step(t, tr, g, state, blob0, blob1, dmask):
        st = tr.opt_state()
        assert st["count"] == t
        assert np.float32(st["learning_rate"]) == np.float32(SCHED(t - 1)), f"step {t}"
        assert st["learning_rate"] == float(np.float32(SCHED(t - 1)))
        assert np.isnan(st["grad_norm"])
        lrs.append(st["learning_rate"])

    _both_modes("small", chain, monkeypatch, per_step)
    assert lrs[4] == float(np.float32(1e-2)) and lrs[3] < lrs[4] > lrs[5]  # the peak, first count of the cosine
    assert lrs[11] < lrs[10] and SCHED(12) == pytest.approx(1e-4, rel=1e-12)
    assert SCHED(11) > SCHED(12) == SCHED(13)


def _norm_check(n):
    def per_step(t, tr, g, state, blob0, blob1, dmask):
        st = tr.opt_state()
        ref = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        # fp32 squares are exact in fp64: only the n additions (and the root) round
        assert abs(st["grad_norm"] - ref) <= n * 2.0**-53 * ref, (t, st["grad_norm"], ref)
        assert st["learning_rate"] == float(np.float32(3e-3))
    return per_step


def test_cfg4_clip_adamw(monkeypatch):
    """clip_by_global_norm + adamw.  c = 0.5 n1 clips step 1; c = 1e6 n1
    never clips, and then the parameters after 12 steps are bit-identical to
    the chain without the clip stage.  grad_norm is the float64 norm of the
    gradient the step descended."""
    n1 = _first_norm("cfg4")
    adamw = lambda: optim.adamw(3e-3, 0.8, 0.95, weight_decay=1e-2)  # noqa: E731
    clipped = []

    def per_step(t, tr, g, state, blob0, blob1, dmask):
        _norm_check(tr.program.blob.size)(t, tr, g, state, blob0, blob1, dmask)
        clipped.append(state["info"]["clip"] < 1.0)

    _both_modes("cfg4", optim.chain(optim.clip_by_global_norm(0.5 * n1), adamw()), monkeypatch, per_step, ":clip")
    assert clipped[0], "step 1 was not clipped"
    clipped.clear()
    loose = _both_modes("cfg4", optim.chain(optim.clip_by_global_norm(1e6 * n1), adamw()), monkeypatch, per_step,
                        ":noclip")
    assert not any(clipped)
    monkeypatch.setenv("ZF_TRAIN_GRAPH", "1")
    plain, _, _ = _forced("cfg4", adamw(), oracle=False, label=":plain")
    assert np.array_equal(_bits(loose), _bits(plain)), f"{np.sum(_bits(loose) != _bits(plain))} entries differ"


def test_bounded_nadamw_masked_decay(monkeypatch):
    """nadamw whose weight decay skips biases and BatchNorm scale / bias.  A
    second run with weight_decay = 0 is held to its own reference, and that
    reference differs from the decayed one, from the same theta_t and g_t, on
    masked-in entries only."""
    mask_fn = R.no_decay_on_biases_and_batchnorm
    chain = optim.nadamw(3e-3, 0.8, 0.95, weight_decay=1e-2, mask=mask_fn)
    _both_modes("bounded", chain, monkeypatch)

    zero = optim.nadamw(3e-3, 0.8, 0.95, weight_decay=0.0, mask=mask_fn)
    refs = {}

    def per_step(t, tr, g, state, blob0, blob1, dmask):
        pm = state["mask"]
        if not refs:
            refs["wd"], refs["0"] = R.chain_state(chain, pm), R.chain_state(zero, pm)
        ref_wd, refs["wd"] = R.chain_reference(blob0, g, refs["wd"], t - 1, chain, dmask)
        ref_0, refs["0"] = R.chain_reference(blob0, g, refs["0"], t - 1, zero, dmask)
        differ = ref_wd != ref_0
        on = dmask & pm
        assert 0 < on.sum() < pm.sum()
        assert not (differ & ~on).any(), "the decay reached an entry outside the mask"
        assert differ[on & (blob0 != 0)].mean() > 0.99
        # so the GPU's no-decay step is also the decayed reference's wherever the mask is off
        tol = R.chain_tolerance(ref_wd, refs["wd"], t, chain)
        off = pm & ~dmask
        assert (np.abs(blob1[off].astype(np.float64) - ref_wd[off]) <= tol[off]).all()

    monkeypatch.setenv("ZF_TRAIN_GRAPH", "1")
    _forced("bounded", zero, oracle=False, per_step=per_step, label=":wd0")


def test_relu_lion(monkeypatch):
    """lion: an element whose b1 mu + (1 - b1) g is within its own rounding
    of zero may take any sign (tests/optim_ref.py); every other element must
    match the one reference.  The number of ambiguous elements is recorded."""
    _both_modes("relu", optim.lion(3e-4, 0.8, 0.9, weight_decay=1e-2), monkeypatch)


def test_odd_generic_stage_loop(monkeypatch):
    """A chain no alias builds (the generic stage loop): clip -> scale_by_adam
    with eps_root -> scale, no learning-rate stage."""
    chain = optim.chain(optim.clip(1e-3), optim.scale_by_adam(0.8, 0.95, eps_root=1e-8), optim.scale(-3e-3))

    def per_step(t, tr, g, state, blob0, blob1, dmask):
        st = tr.opt_state()
        assert np.isnan(st["learning_rate"]) and np.isnan(st["grad_norm"]) and len(st["slots"]) == 2

    _both_modes("odd", chain, monkeypatch, per_step)


# ---- resume ---------------------------------------------------------------------------------
def _steps(tr, case, batches):
    for lo, hi in batches:
        tr.step(case["x"][lo:hi], None if case["c"] is None else case["c"][lo:hi])


@pytest.mark.parametrize("kind", ["chain", "legacy"])
def test_resume_bit_for_bit(kind, tmp_path):
    """6 steps == 3 steps, variables() + opt_state() through
    io.save_opt_state / load_opt_state, a new Trainer, load_opt_state, 3 more
    steps: the same bits, for a chain (clip + nadamw on a schedule: the norm,
    the counter that drives schedule and bias corrections, both moments) and
    for the legacy Optimizer (m, v, the counter and its bias corrections)."""
    import zenflow_amd as zf
    from zenflow_amd.train import Optimizer

    name = "small"
    case = make_case(name, N=TR.TRAJ_ROWS, seed=SEEDS[name])
    batches = TR.trajectory_batches()[:6]
    if kind == "chain":
        make = lambda: optim.chain(optim.clip_by_global_norm(0.5 * _first_norm(name)),  # noqa: E731
                                   optim.nadamw(SCHED, 0.8, 0.95, weight_decay=1e-2))
    else:
        make = lambda: Optimizer(3e-3, 0.8, 0.95, 1e-8, 1e-2, True)  # noqa: E731
    whole = _trainer(case, make())
    _steps(whole, case, batches)
    first = _trainer(case, make())
    _steps(first, case, batches[:3])
    variables, state = first.variables(), first.opt_state()
    assert state["count"] == 3 and len(state["slots"]) == 2
    assert any(np.any(l != 0) for _, l in _leaves(state["slots"][0]))
    zf.save_opt_state(tmp_path / "opt.npz", state)
    del first
    loaded = zf.load_opt_state(tmp_path / "opt.npz")
    assert loaded["count"] == 3 and len(loaded["slots"]) == 2
    for a, b in zip(state["slots"], loaded["slots"]):
        for (pa, la), (pb, lb) in zip(_leaves(a), _leaves(b)):
            assert pa == pb and np.array_equal(_bits(la), _bits(lb))
    second = _trainer(case, make(), variables=variables)
    second.load_opt_state(loaded)
    assert second.opt_state()["count"] == 3
    _steps(second, case, batches[3:])
    a, b = _blob(whole), _blob(second)
    assert np.array_equal(_bits(a), _bits(b)), f"{np.sum(_bits(a) != _bits(b))} entries differ after the resume"
    sa, sb = whole.opt_state(), second.opt_state()
    assert sa["count"] == sb["count"] == 6
    assert sa["learning_rate"] == sb["learning_rate"]
    assert sa["grad_norm"] == sb["grad_norm"] or (np.isnan(sa["grad_norm"]) and np.isnan(sb["grad_norm"]))
    for x, y in zip(sa["slots"], sb["slots"]):
        for (_, lx), (_, ly) in zip(_leaves(x), _leaves(y)):
            assert np.array_equal(_bits(lx), _bits(ly))


# ---- train() ----------------------------------------------------------------------------------
def test_train_function_takes_a_chain():
    """train(..., optimizer=chain) on 300 rows in batches of 64 (the last one
    44 rows) returns the variables of the same loop written with Trainer.step.
    ``patience=3`` (in epochs): with the default 0.05 of 3 epochs train()'s
    early-stopping rule, the reference's, divides by a patience of 0."""
    import zenflow_amd as zf
    from zenflow_amd.io import flatten_variables

    case = make_case("small", N=340, seed=31)
    X, Xt = case["x"][:300], case["x"][300:]
    make = lambda: optim.chain(optim.clip_by_global_norm(1.0),  # noqa: E731
                               optim.adamw(optim.cosine_decay_schedule(3e-3, 15), weight_decay=1e-2))
    flow = build_flow(case["cfg"])
    flow.latent._dim = case["cfg"]["D"]
    best, best_epoch, lt, ls = zf.train(flow, X, Xt, optimizer=make(), epochs=3, batch_size=64, progress=False,
                                        patience=3, initial_variables=case["variables"])
    assert len(lt) == len(ls) == 3 and np.isfinite(lt).all()
    tr = _trainer(case, make(), batch_max=64, variables=case["variables"])
    per_epoch = []
    for epoch in range(3):
        Xp = X[np.random.default_rng([0, epoch]).permutation(300)]
        for lo in range(0, 300, 64):
            tr.step(Xp[lo:lo + 64])
        per_epoch.append(tr.variables())
    assert tr.opt_state()["count"] == 15
    want, got = flatten_variables(per_epoch[best_epoch]), flatten_variables(best)
    assert sorted(want) == sorted(got)
    for k in want:
        assert np.array_equal(_bits(want[k]), _bits(got[k])), k
    moved = flatten_variables(case["variables"])
    assert any(not np.array_equal(moved[k], got[k]) for k in got if k.startswith("params"))


# ---- rejected chains ----------------------------------------------------------------------------
def test_rejected_chains_leave_no_handle():
    from zenflow_amd import _lib as L
    from zenflow_amd.train import Trainer

    case = make_case("small", N=64, seed=1)
    bad = [optim.chain(*[optim.scale(1.0)] * 9),
           optim.chain(optim.scale_by_adam(), optim.trace(0.9), optim.trace(0.9), optim.scale_by_lion()),
           optim.chain(optim.scale(2.0), optim.clip_by_global_norm(1.0)),
           optim.chain(optim.clip_by_global_norm(1.0), optim.clip_by_global_norm(1.0))]
    for ch in bad:
        made = []
        orig = Trainer._open

        def spy(self, *a, **k):
            made.append(self)
            return orig(self, *a, **k)

        Trainer._open = spy
        try:
            with pytest.raises(NotImplementedError, match="optimiser chain"):
                _trainer(case, ch, batch_max=64)
        finally:
            Trainer._open = orig
        assert len(made) == 1 and not getattr(made[0], "handle", None)
    # the library rejects them too, names the stage, and leaves the trainer as it was
    tr = _trainer(case, None, batch_max=64)
    lib = L.load_library()
    c = L.ZfOptimChain()
    c.n_stages = 2
    c.stages[0].kind, c.stages[1].kind = L.ZF_OPT_SCALE, L.ZF_OPT_CLIP_BY_GLOBAL_NORM
    assert lib.zf_trainer_set_optim_chain(tr.handle, ct.byref(c), None) == -2
    assert b"clip_by_global_norm after scale" in lib.zf_last_error()
    c.n_stages = 9
    assert lib.zf_trainer_set_optim_chain(tr.handle, ct.byref(c), None) == -2
    for k in range(3):
        c.stages[k].kind = L.ZF_OPT_SCALE_BY_ADAM if k == 0 else L.ZF_OPT_TRACE
    c.stages[3].kind = L.ZF_OPT_SCALE_BY_LION
    c.n_stages = 4
    assert lib.zf_trainer_set_optim_chain(tr.handle, ct.byref(c), None) == -2
    assert b"scale_by_lion" in lib.zf_last_error()
    tr.step(case["x"])  # still the (n)adamw it was created with
    assert tr.opt_state()["count"] == 1 and len(tr.opt_state()["slots"]) == 2
