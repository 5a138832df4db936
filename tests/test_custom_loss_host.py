"""Host-side checks of the custom-loss interface (no GPU): the three C
entries are bound with the header's arity, exported, and reject a NULL
trainer; ``Trainer.forward / backward / apply_gradient`` have their
signatures; a bad cotangent raises before any device call; and the oracle
worker (tests/custom_loss_oracle.py) with ``cot = -1/N`` in train mode is the
arithmetic of ``tests.input_grad_oracle.train_grads``, bit for bit."""

import inspect

import numpy as np
import pytest

from tests.test_input_grad_host import _header_args
from zenflow_amd import _lib as L

NEW = {"zf_trainer_forward": 9, "zf_trainer_backward": 5, "zf_trainer_apply_gradient": 3}


def test_new_symbols_bound_and_exported():
    lib = L.load_library()
    for name, arity in NEW.items():
        _, args = L.SIGNATURES[name]
        assert len(args) == len(_header_args(name)) == arity, name
        assert hasattr(lib, name), name
        # the eight loss_grad / step entries stay eight
        assert not name.startswith(("zf_trainer_loss_grad", "zf_trainer_step"))


def test_each_entry_rejects_a_null_trainer():
    lib = L.load_library()
    for name in NEW:
        _, args = L.SIGNATURES[name]
        zeros = [0 if a in (L.C.c_int, L.C.c_int64) else None for a in args]
        assert getattr(lib, name)(*zeros) == -1, name
        assert "trainer is NULL" in lib.zf_last_error().decode(), name
        # another message in between: the next entry must set its own
        assert lib.zf_trainer_get_blob(None, None) == -1
        assert "trainer is NULL" not in lib.zf_last_error().decode()


def test_signatures():
    from zenflow_amd.train import Trainer

    kw = inspect.Parameter.KEYWORD_ONLY
    f = inspect.signature(Trainer.forward).parameters
    assert list(f) == ["self", "x", "c", "train", "update_stats", "global_rows"]
    assert f["c"].default is None and f["train"].default is True and f["train"].kind is kw
    assert f["update_stats"].default is None and f["update_stats"].kind is kw
    assert f["global_rows"].default is None and f["global_rows"].kind is kw
    b = inspect.signature(Trainer.backward).parameters
    assert list(b) == ["self", "cotangent", "cond_grad"]
    assert b["cond_grad"].default is False and b["cond_grad"].kind is kw
    a = inspect.signature(Trainer.apply_gradient).parameters
    assert list(a) == ["self", "g"] and a["g"].default is None


def _pending(rows):
    """A Trainer object with a forward of ``rows`` rows pending and no device behind it."""
    from zenflow_amd.train import Trainer

    tr = Trainer.__new__(Trainer)
    tr.handle = None
    tr.C = 0
    tr._pending_rows = rows
    tr._pending_device = False
    return tr


def test_bad_cotangent_raises_before_any_device_call(monkeypatch):
    # any device call would go through ensure_device: make it fail loudly
    def no_device():
        raise AssertionError("device touched before the cotangent was checked")

    monkeypatch.setattr(L, "ensure_device", no_device)
    monkeypatch.setattr(L, "load_library", no_device)
    with pytest.raises(ValueError, match="cotangent"):
        _pending(8).backward(np.ones(9, np.float32))
    with pytest.raises(ValueError, match="cotangent"):
        _pending(8).backward(np.ones((8, 1), np.float32))
    for bad in (np.nan, np.inf):
        cot = np.ones(8, np.float32)
        cot[3] = bad
        with pytest.raises(ValueError, match="non-finite"):
            _pending(8).backward(cot)
    # the check is what raised: a good cotangent gets as far as the device
    with pytest.raises(AssertionError, match="device touched"):
        _pending(8).backward(np.ones(8, np.float32))


def test_backward_without_forward_and_eval_update_stats(monkeypatch):
    def no_device():
        raise AssertionError("device touched")

    monkeypatch.setattr(L, "ensure_device", no_device)
    monkeypatch.setattr(L, "load_library", no_device)
    with pytest.raises(ValueError, match="pending forward"):
        _pending(None).backward(np.ones(8, np.float32))
    with pytest.raises(ValueError, match="update_stats"):
        _pending(None).forward(np.zeros((4, 2), np.float32), train=False, update_stats=True)


def test_oracle_with_minus_one_over_n_is_the_train_loss_oracle():
    """cot = -1/N, train mode: sum(cot * lp) is -mean(lp) term by term, so
    d / d c has the bits of ``train_grads``' gc64 (cfg4, 128 rows: -1/128 is
    exact, and so is every product by it)."""
    import torch

    from tests.custom_loss_oracle import custom_grads
    from tests.flowcases import make_case
    from tests.input_grad_oracle import train_grads

    N = 128
    case = make_case("cfg4", N=N, seed=63)
    job = {"model": case["model"], "variables": case["variables"], "x": case["x"], "c": case["c"]}
    loss, gc_ref, _, _ = train_grads(job, torch.float64)
    lp, _, gc, _ = custom_grads(case["model"], case["variables"], case["x"], case["c"], np.full(N, -1.0 / N), True,
                                torch.float64)
    assert np.isfinite(lp).all() and np.isfinite(gc_ref).all() and np.abs(gc_ref).max() > 0
    assert gc.shape == gc_ref.shape == case["c"].shape
    assert np.array_equal(gc.view(np.uint64), gc_ref.view(np.uint64))
    assert -lp.mean() == pytest.approx(loss, rel=1e-14)
