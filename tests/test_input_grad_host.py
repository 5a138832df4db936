"""Host-side checks of the input-gradient interface (no GPU): the new C
symbols are bound with the header's argument counts, and the existing
Trainer calls keep their signatures and defaults."""

import inspect
import re
from pathlib import Path

from zenflow_amd import _lib as L

HEADER = Path(__file__).resolve().parents[1] / "include" / "zenflow_amd.h"
NEW = ["zf_trainer_loss_grad_cond_shard", "zf_trainer_step_cond_shard", "zf_trainer_log_prob_vjp"]


def _header_args(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in the header"
    return [a.strip() for a in m.group(1).split(",")]


def test_new_symbols_bound_with_header_arity():
    for name in NEW:
        res, args = L.SIGNATURES[name]
        assert len(args) == len(_header_args(name)), name
    assert len(_header_args("zf_trainer_loss_grad_cond_shard")) == 10
    assert len(_header_args("zf_trainer_step_cond_shard")) == 8
    assert len(_header_args("zf_trainer_log_prob_vjp")) == 9


def test_new_symbols_exported():
    lib = L.load_library()
    for name in NEW:
        assert hasattr(lib, name), name


def test_trainer_signatures_keep_their_defaults():
    from zenflow_amd.train import Trainer

    lg = inspect.signature(Trainer.loss_grad).parameters
    assert list(lg)[:5] == ["self", "x", "c", "update_stats", "global_rows"]
    assert lg["c"].default is None and lg["update_stats"].default is False and lg["global_rows"].default is None
    assert lg["cond_grad"].default is False
    st = inspect.signature(Trainer.step).parameters
    assert list(st)[:4] == ["self", "x", "c", "global_rows"]
    assert st["c"].default is None and st["global_rows"].default is None and st["cond_grad"].default is False


def test_flow_methods_exist():
    from zenflow_amd.flow import BoundFlow, Flow

    p = inspect.signature(Flow.log_prob_and_grad).parameters
    assert p["c"].default is None and p["cotangent"].default is None and p["chunk_rows"].default is None
    assert p["cotangent"].kind is inspect.Parameter.KEYWORD_ONLY
    b = inspect.signature(BoundFlow.log_prob_and_grad).parameters
    assert list(b)[:4] == ["self", "x", "c", "cotangent"] and b["cotangent"].default is None
