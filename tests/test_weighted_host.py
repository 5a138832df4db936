"""Host-side checks of the weighted-loss interface (no GPU): ``train()``
rejects bad weights before any device call, the weighted metric is the fp64
weighted mean, the new C entries are bound with the header's arity, and the
existing calls keep their signatures."""

import inspect

import numpy as np
import pytest

from tests.test_input_grad_host import _header_args
from zenflow_amd import _lib as L

NEW = {"zf_trainer_loss_grad_weighted_shard": 11, "zf_trainer_step_weighted_shard": 9}


def _moons(n=64):
    rng = np.random.default_rng(0)
    return rng.uniform(0.1, 0.9, (n, 2)).astype(np.float32)


def _train(**kw):
    import zenflow_amd as zf
    from tests.dist_worker import two_moons_flow

    X = _moons()
    return zf.train(two_moons_flow(), X[:48], X[48:], epochs=20, batch_size=16, progress=False, **kw)


@pytest.mark.parametrize("key,n", [("W_train", 48), ("W_test", 16)])
def test_train_rejects_bad_weights_without_a_device(key, n, monkeypatch):
    # any device call would go through ensure_device: make it fail loudly
    def no_device():
        raise AssertionError("device touched before the weights were checked")

    monkeypatch.setattr(L, "ensure_device", no_device)
    with pytest.raises(ValueError, match=key):
        _train(**{key: np.ones(n + 1, np.float32)})
    with pytest.raises(ValueError, match=key):
        _train(**{key: np.ones((n, 1), np.float32)})
    w = np.ones(n, np.float32)
    w[3] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        _train(**{key: w})
    w[3] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        _train(**{key: w})


def test_train_rejects_a_non_positive_test_sum():
    w = np.ones(16, np.float32)
    w[:8] = -1.0
    with pytest.raises(ValueError, match="W_test"):
        _train(W_test=w)


def test_weighted_metric_is_the_fp64_weighted_mean():
    from tests.weighted_grad_oracle import make_weights
    from zenflow_amd.train import weighted_nll

    rng = np.random.default_rng(5)
    for n in (8, 300, 4096):
        lp = (3.0 * rng.standard_normal(n) - 1.0).astype(np.float32)
        w = make_weights(n, n)
        got = weighted_nll(lp, w)
        assert isinstance(got, float)
        assert got == np.average(-lp.astype(np.float64), weights=w.astype(np.float64))
    assert weighted_nll(np.array([1.0, 5.0], np.float32), np.array([1.0, 0.0], np.float32)) == -1.0


def test_check_weights():
    from zenflow_amd.train import check_weights

    w = check_weights([0.0, -0.25, 2.0], 3, "w")
    assert w.dtype == np.float32 and w.flags["C_CONTIGUOUS"] and w.tolist() == [0.0, -0.25, 2.0]
    with pytest.raises(ValueError, match=r"shape \(4,\)"):
        check_weights(w, 4, "w")


def test_new_symbols_bound_and_exported():
    lib = L.load_library()
    for name, arity in NEW.items():
        _, args = L.SIGNATURES[name]
        assert len(args) == len(_header_args(name)) == arity, name
        assert hasattr(lib, name), name


def test_every_entry_rejects_a_null_trainer():
    """Each of the eight loss_grad / step entries, called with a NULL trainer
    (no device is touched): -1 and "trainer is NULL"."""
    lib = L.load_library()
    entries = [n for n in L.SIGNATURES if n.startswith(("zf_trainer_loss_grad", "zf_trainer_step"))]
    assert len(entries) == 8
    for name in entries:
        _, args = L.SIGNATURES[name]
        zeros = [0 if a in (L.C.c_int, L.C.c_int64) else None for a in args]
        assert getattr(lib, name)(*zeros) == -1, name
        assert "trainer is NULL" in lib.zf_last_error().decode(), name
        # another message in between: the next entry must set its own
        assert lib.zf_trainer_get_blob(None, None) == -1
        assert "trainer is NULL" not in lib.zf_last_error().decode()


def test_signatures():
    from zenflow_amd.train import Trainer, train

    lg = inspect.signature(Trainer.loss_grad).parameters
    assert list(lg)[:6] == ["self", "x", "c", "update_stats", "global_rows", "cond_grad"] and lg["w"].default is None
    st = inspect.signature(Trainer.step).parameters
    assert list(st)[:5] == ["self", "x", "c", "global_rows", "cond_grad"] and st["w"].default is None
    assert inspect.signature(Trainer._step_rows).parameters["wptr"].default is None
    assert inspect.signature(Trainer._step_local).parameters["wptr"].default is None
    tp = inspect.signature(train).parameters
    for k in ("W_train", "W_test"):
        assert tp[k].default is None and tp[k].kind is inspect.Parameter.KEYWORD_ONLY
