"""zenflow_amd.optim and tests/optim_ref.py on the host: the schedules' known
answers, the chain API, the lowering of a decay mask to blob entries, and that
the tolerance the GPU test (tests/test_gpu_optim.py) holds the chain kernels
to is wide enough for a correct fp32 evaluation of every kernel form and
narrow enough to catch a wrong one.

The fp32 side is ``chain_kernel_f32`` (the kernels' arithmetic operation by
operation in NumPy float32), the float64 side ``chain_reference``, teacher
forced as in the GPU test: every step starts from the fp32 parameters, the
float64 moments and their twins are carried from the same gradients.  The
problem is the one of tests/test_train_ref_host.py (gradient magnitudes 1e-12
.. 10, cancelling and random signs, dead elements, a tenth of the entries
statistics), the settings start from train_ref.Opt's (lr 3e-3, b1 0.8, b2
0.95, wd 1e-2, momentum 0.8)."""

import math

import numpy as np
import pytest

import zenflow_amd.optim as optim
from tests import optim_ref as R
from tests.test_train_ref_host import N, _problem

STEPS = 12
SCHED = optim.warmup_cosine_decay_schedule(1e-3, 1e-2, 4, 12, 1e-4)


# ---- schedules ---------------------------------------------------------------------
def test_cosine_known_answers():
    s = optim.cosine_decay_schedule(2.0, 10, alpha=0.2)
    assert s(0) == 2.0
    assert s(5) == pytest.approx(2.0 * (1 + 0.2) / 2, rel=1e-15)
    assert s(10) == pytest.approx(0.4, rel=1e-15) and s(11) == s(10) == s(10**6)
    e = optim.cosine_decay_schedule(2.0, 10, alpha=0.0, exponent=2.0)
    assert e(5) == pytest.approx(2.0 * 0.25, rel=1e-15)


def test_linear_known_answers():
    s = optim.linear_schedule(1.0, 3.0, 4, transition_begin=2)
    assert [s(c) for c in (0, 2, 3, 4, 6, 7, 100)] == [1.0, 1.0, 1.5, 2.0, 3.0, 3.0, 3.0]
    assert optim.linear_schedule(1.0, 3.0, 0)(5) == 1.0
    assert optim.constant_schedule(0.25)(10**9) == 0.25


def test_warmup_cosine_joins_at_the_peak():
    s = optim.warmup_cosine_decay_schedule(1e-3, 1e-2, 4, 12, 1e-4)
    assert s(0) == pytest.approx(1e-3, rel=1e-14)  # (init - end) 1 + end rounds
    # the warm-up segment ends at the peak; count == warmup_steps is the cosine's count 0
    assert optim.linear_schedule(1e-3, 1e-2, 4)(4) == 1e-2
    assert s(4) == 1e-2
    assert len(s.segments) == 2 and s.segments[1][0] == 4.0
    assert s(3) == pytest.approx(1e-3 + 0.75 * 9e-3, rel=1e-14)
    assert s(8) == pytest.approx(1e-2 * (1 + 1e-2) / 2, rel=1e-14)  # the cosine's half way
    assert s(12) == pytest.approx(1e-4, rel=1e-13) and s(13) == s(12) == s(1000)
    j = optim.join_schedules([optim.linear_schedule(1e-3, 1e-2, 4), optim.cosine_decay_schedule(1e-2, 8, 1e-2)], [4])
    assert all(j(c) == s(c) for c in range(16))
    assert optim.warmup_cosine_decay_schedule(0.0, 0.0, 2, 6, 1.0)(5) == 0.0  # peak 0: alpha 0


def test_exponential_known_answers():
    s = optim.exponential_decay(1.0, 4, 0.5)
    assert s(0) == 1.0 and s(4) == 0.5 and s(2) == pytest.approx(math.sqrt(0.5), rel=1e-15)
    st = optim.exponential_decay(1.0, 4, 0.5, staircase=True)
    assert [st(c) for c in (0, 3, 4, 7, 8)] == [1.0, 1.0, 0.5, 0.5, 0.25]
    lo = optim.exponential_decay(1.0, 1, 0.5, end_value=0.2)
    assert lo(2) == 0.25 and lo(3) == 0.2 and lo(50) == 0.2
    hi = optim.exponential_decay(1.0, 1, 2.0, end_value=5.0)
    assert hi(2) == 4.0 and hi(3) == 5.0
    b = optim.exponential_decay(1.0, 2, 0.5, transition_begin=3)
    assert b(3) == 1.0 and b(2) == 1.0 and b(5) == 0.5


def test_piecewise_and_join():
    s = optim.piecewise_constant_schedule(1.0, {2: 0.5, 5: 0.1})
    assert [s(c) for c in (0, 2, 3, 5, 6, 99)] == [1.0, 1.0, 0.5, 0.5, 0.05, 0.05]
    j = optim.join_schedules([optim.constant_schedule(1.0), optim.linear_schedule(2.0, 4.0, 2),
                              optim.constant_schedule(7.0)], [3, 10])
    assert [j(c) for c in (0, 2, 3, 4, 5, 9, 10, 11)] == [1.0, 1.0, 2.0, 3.0, 4.0, 4.0, 7.0, 7.0]
    with pytest.raises(NotImplementedError, match="segments"):
        optim.join_schedules([optim.constant_schedule(1.0)] * 5, [1, 2, 3, 4])
    with pytest.raises(NotImplementedError, match="boundaries"):
        optim.piecewise_constant_schedule(1.0, {1: 0.5, 2: 0.5, 3: 0.5, 4: 0.5})


def test_schedule_lowers_to_the_abi():
    from zenflow_amd import _lib as L

    s = SCHED.lower()
    assert s.kind == L.ZF_SCHED_JOIN and s.n_segments == 2
    assert list(s.seg_kind)[:2] == [L.ZF_SCHED_LINEAR, L.ZF_SCHED_COSINE]
    assert s.boundary[1] == 4.0 and list(s.p[1])[:4] == [1e-2, 8.0, 1e-2, 1.0]
    assert optim.constant_schedule(3.0).lower().kind == L.ZF_SCHED_CONSTANT


# ---- the chain API -------------------------------------------------------------------
def test_chain_flattens_and_aliases():
    from zenflow_amd import _lib as L
    import zenflow_amd as zf

    assert zf.optim is optim
    c = optim.chain(optim.clip_by_global_norm(1.0), optim.chain(optim.adamw(1e-3), optim.scale(0.5)))
    assert [s.name for s in c] == ["clip_by_global_norm", "scale_by_adam", "add_decayed_weights",
                                   "scale_by_learning_rate", "scale"]
    assert c.n_slots == 2
    assert [s.name for s in optim.sgd(0.1)] == ["scale_by_learning_rate"]
    assert [s.name for s in optim.sgd(0.1, 0.9, True)] == ["trace", "scale_by_learning_rate"]
    assert optim.sgd(0.1, 0.9, True).stages[0].nesterov
    assert [s.name for s in optim.lion(1e-4)] == ["scale_by_lion", "add_decayed_weights", "scale_by_learning_rate"]
    assert optim.lion(1e-4).stages[1].p == (1e-3,) and optim.lion(1e-4).stages[0].p == (0.9, 0.99)
    a = optim.adamw(1e-3)
    assert a.stages[0].p == (0.9, 0.999, 1e-8, 0.0) and a.stages[1].p == (1e-4,) and not a.stages[0].nesterov
    assert optim.nadamw(1e-3).stages[0].nesterov and optim.nadam(1e-3).stages[0].nesterov
    assert [s.name for s in optim.adam(1e-3)] == ["scale_by_adam", "scale_by_learning_rate"]
    low = optim.nadamw(SCHED, mask={"bijector": {}}).lower()
    assert low.n_stages == 3 and low.stages[0].flags == L.ZF_OPT_FLAG_NESTEROV
    assert low.stages[1].flags == L.ZF_OPT_FLAG_MASKED and low.stages[2].sched.n_segments == 2
    assert low.stages[0].p[0] == np.float32(0.9)
    with pytest.raises(TypeError):
        optim.chain(1e-3)


@pytest.mark.parametrize("bad,match", [
    (lambda: optim.chain(*[optim.scale(1.0)] * 9), "stages"),
    (lambda: optim.chain(optim.scale_by_adam(), optim.trace(0.9), optim.trace(0.9), optim.scale_by_lion()),
     "scale_by_lion"),
    (lambda: optim.chain(optim.scale(2.0), optim.clip_by_global_norm(1.0), optim.adam(1e-3)), "clip_by_global_norm"),
    (lambda: optim.chain(optim.clip_by_global_norm(1.0), optim.clip_by_global_norm(2.0)), "clip_by_global_norm"),
])
def test_rejected_chains(bad, match):
    with pytest.raises(NotImplementedError, match=match):
        bad().lower()


def test_mask_lowers_to_blob_entries():
    """A tree mask and the callable that returns it lower to the same bytes:
    set exactly on the blob entries of the leaves the mask selects."""
    from tests.flowcases import make_case

    case = make_case("bounded", N=8, seed=3)
    prog = R.host_program(case["cfg"], case["variables"])
    pm = prog.param_mask == 1
    tree = R.no_decay_on_biases_and_batchnorm(case["variables"]["params"])
    m_tree = optim.lower_mask(tree, prog)
    m_call = optim.lower_mask(R.no_decay_on_biases_and_batchnorm, prog)
    assert m_tree.dtype == np.uint8 and np.array_equal(m_tree, m_call)
    # the blob_to_variables(np.arange(n)) trick: where each leaf lives
    at = prog.blob_to_variables(np.arange(prog.blob.size, dtype=np.float32))["params"]
    want = np.zeros(prog.blob.size, bool)
    n_kernels = 0
    for bij in at.values():
        for name, layer in bij.items():
            if name.startswith("Dense_"):
                want[layer["kernel"].reshape(-1).astype(np.int64)] = True
                n_kernels += 1
    assert n_kernels == 9 and np.array_equal(m_tree.astype(bool), want)
    assert not (want & ~pm).any() and (pm & ~want).sum() > 0
    # the round trip of a params-shaped tree through the blob
    blob = optim.tree_to_blob(prog, case["variables"]["params"])
    assert np.array_equal(blob[pm], prog.blob[pm]) and not blob[~pm].any()
    back = optim.blob_to_tree(prog, blob)
    k = "bijectors_3"
    assert np.array_equal(back["bijector"][k]["Dense_1"]["kernel"],
                          case["variables"]["params"]["bijector"][k]["Dense_1"]["kernel"])
    # one bool for a whole leaf broadcasts
    per_leaf = optim.lower_mask(lambda p: {"bijector": {b: {l: {n: l == "Dense_0" for n in v} for l, v in t.items()}
                                                        for b, t in p["bijector"].items()}}, prog)
    assert 0 < per_leaf.sum() < m_tree.sum()


# ---- the tolerance -------------------------------------------------------------------------
def _dmask(seed=9):
    return np.random.default_rng(seed).uniform(size=N) < 0.5


def _norm1():
    theta, g, mask = _problem()
    return float(np.sqrt(np.sum(np.where(mask, g[0].astype(np.float64), 0) ** 2)))


def _chains():
    n1 = _norm1()
    tree = {"bijector": {}}  # stands for "masked": the blob mask comes from _dmask
    return {
        "sgd": optim.sgd(SCHED, momentum=0.8, nesterov=True),
        "sgd_plain_clip": optim.chain(optim.clip_by_global_norm(0.5 * n1), optim.sgd(3e-3)),
        "sgd_clip": optim.chain(optim.clip_by_global_norm(0.5 * n1), optim.sgd(SCHED, momentum=0.8)),
        "sgd_noclip": optim.chain(optim.clip_by_global_norm(1e3 * n1), optim.sgd(SCHED, momentum=0.8, nesterov=True)),
        "adamw_clip": optim.chain(optim.clip_by_global_norm(0.5 * n1),
                                  optim.adamw(3e-3, 0.8, 0.95, weight_decay=1e-2)),
        "nadamw_masked": optim.nadamw(SCHED, 0.8, 0.95, weight_decay=1e-2, mask=tree),
        "adam": optim.adam(3e-3, 0.8, 0.95),
        "lion": optim.lion(3e-4, 0.8, 0.9, weight_decay=1e-2),
        "lion_masked": optim.lion(SCHED, 0.8, 0.9, weight_decay=1e-2, mask=tree),
        "generic": optim.chain(optim.clip(1e-3), optim.scale_by_adam(0.8, 0.95, eps_root=1e-8), optim.scale(-3e-3)),
        "generic_nesterov": optim.chain(optim.scale_by_adam(0.8, 0.95, eps_root=1e-8, nesterov=True),
                                        optim.add_decayed_weights(1e-2, mask=tree), optim.trace(0.8),
                                        optim.scale_by_learning_rate(SCHED)),
    }


def _ratios(chain, fault=None):
    """Per step: |fp32 - reference| / tolerance over the masked-in elements,
    and the ambiguous lion elements."""
    theta, g, mask = _problem()
    dmask = _dmask()
    state = R.chain_state(chain, mask)
    slots = [np.zeros(N, np.float32) for _ in range(chain.n_slots)]
    out, amb = [], 0
    for count in range(STEPS):
        nxt, slots = R.chain_kernel_f32(theta, g[count], slots, count, chain, mask, dmask, fault=fault)
        ratio, state, a = R.chain_check(nxt, theta, g[count], state, count, chain, dmask)
        assert np.array_equal(nxt[~mask], theta[~mask])
        out.append(ratio[mask])
        amb += a
        theta = nxt
    return out, amb


@pytest.mark.parametrize("name", list(_chains()))
def test_fp32_chain_within_tolerance(name):
    ratios, amb = _ratios(_chains()[name])
    worst = [float(r.max()) for r in ratios]
    print(f"{name}: worst error / tolerance per step:", [f"{w:.3f}" for w in worst], "ambiguous:", amb)
    assert max(worst) <= 1.0, worst
    assert max(worst) > 0.02, worst  # the bound is not slack by orders of magnitude either


# fault -> the chains it can show in
FAULT_CHAINS = {
    "schedule_at_count_plus_1": ("sgd", "nadamw_masked", "lion_masked"),
    "clip_below_max_norm": ("sgd_noclip",),
    "norm_over_statistics": ("sgd_clip", "sgd_plain_clip"),
    "nesterov_old_trace": ("sgd",),
    "decay_mask_ignored": ("nadamw_masked", "lion_masked", "generic_nesterov"),
    "lion_moment_b1": ("lion",),
    "eps_root_outside_sqrt": ("generic", "generic_nesterov"),
}


def test_every_fault_is_covered():
    assert set(FAULT_CHAINS) == set(R.FAULTS)


@pytest.mark.parametrize("fault,name", [(f, n) for f in R.FAULTS for n in FAULT_CHAINS[f]])
def test_faulty_chain_exceeds_tolerance(fault, name):
    ratios, _ = _ratios(_chains()[name], fault=fault)
    share = [float((r > 1.0).mean()) for r in ratios]
    print(f"{fault}/{name}: share of elements over the tolerance per step:", [f"{s:.3f}" for s in share])
    assert min(share[1:]) >= 0.01, share  # from step 2 on (at t = 1 the moments are zero)


def test_reference_matches_direct_formula():
    """Two steps of chain_reference against sgd with nesterov momentum, a
    schedule and a clip written out by hand."""
    ch = optim.chain(optim.clip_by_global_norm(1.0), optim.sgd(optim.linear_schedule(0.5, 0.25, 1), 0.5, True))
    th0, g1, g2 = np.array([0.5, -2.0]), np.array([3.0, -4.0]), np.array([-0.3, 0.4])
    st = R.chain_state(ch, np.ones(2, bool))
    th1, st = R.chain_reference(th0, g1, st, 0, ch)
    assert st["info"]["norm"] == 5.0 and st["info"]["clip"] == 0.2 and st["info"]["lr"] == 0.5
    u1 = g1 / 5.0
    np.testing.assert_allclose(th1, th0 - 0.5 * (u1 + 0.5 * u1), rtol=1e-14)
    th2, st = R.chain_reference(th1, g2, st, 1, ch)
    assert st["info"]["norm"] == 0.5 and st["info"]["clip"] == 1.0 and st["info"]["lr"] == 0.25
    tr2 = g2 + 0.5 * u1
    np.testing.assert_allclose(th2, th1 - 0.25 * (g2 + 0.5 * tr2), rtol=1e-14)
    np.testing.assert_allclose(st["stages"][1]["T"], np.abs(g2) + 0.5 * np.abs(u1), rtol=1e-14)
    # lion: the sign of b1 mu + (1 - b1) g, the moment with b2, decay on theta
    li = optim.lion(0.1, 0.5, 0.75, weight_decay=0.5)
    s0 = R.chain_state(li, np.ones(2, bool))
    a1, s1 = R.chain_reference(th0, g1, s0, 0, li)
    np.testing.assert_allclose(a1, th0 - 0.1 * (np.sign(g1) + 0.5 * th0), rtol=1e-14)
    np.testing.assert_allclose(s1["stages"][0]["mu"], 0.25 * g1, rtol=1e-14)
    a2, s2 = R.chain_reference(a1, g2, s1, 1, li)
    np.testing.assert_allclose(a2, a1 - 0.1 * (np.sign(0.5 * 0.25 * g1 + 0.5 * g2) + 0.5 * a1), rtol=1e-14)
