"""The shipped kernel sources compile exactly one kernel (no GPU): the build
passes no -D, and the sources test no build-time macro besides the two
tuning aids that leave results unchanged."""

import re
from pathlib import Path

from zenflow_amd import build

# ZF_X3_TRACE: the phase trace and the resident stamp trace; ZF_X3_MARK: the
# marker comments scripts/valu_budget.py reads.  Neither is set by build.py.
# The sources use no include guards (#pragma once) and test no
# compiler-provided macro; one that comes to be needed is added here by name.
ALLOWED = {"ZF_X3_TRACE", "ZF_X3_MARK"}

_COND = re.compile(r"^[ \t]*#[ \t]*(if|ifdef|ifndef|elif)\b(.*)$", re.M)
_IDENT = re.compile(r"[A-Za-z_]\w*")


def _tested_macros(text: str) -> set:
    text = text.replace("\\\n", " ")
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    names = set()
    for m in _COND.finditer(text):
        expr = m.group(2).split("//")[0]
        names |= {n for n in _IDENT.findall(expr) if n != "defined"}
    return names


def test_build_defines_no_macro():
    assert [f for f in build.FLAGS + build.X3_FLAGS if f.startswith("-D")] == []


def test_sources_test_only_the_two_tuning_macros():
    files = sorted(build.CSRC.glob("*.h")) + sorted(build.CSRC.glob("*.hip"))
    assert len(files) >= len(build.SOURCES)
    seen = {}
    for f in files:
        for name in _tested_macros(f.read_text()):
            seen.setdefault(name, []).append(f.name)
    extra = {n: fs for n, fs in seen.items() if n not in ALLOWED}
    assert not extra, f"build-time macros tested by the sources besides {sorted(ALLOWED)}: {extra}"
    assert set(seen) == ALLOWED  # the scan sees the ones that are there


def test_scan_sees_every_conditional_form():
    text = "#if A == 1 && defined(B)\n#elif !defined C // D\n  # ifdef E\n#ifndef F\n/* #if G */\n// #if H\n#if I \\\n  || J\n"
    assert _tested_macros(text) == {"A", "B", "C", "E", "F", "I", "J"}
