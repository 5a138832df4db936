"""The flow image on the CPU (no GPU): tests/host/flow_image_check.cpp, built
host-only with zf_flow_image.hip and zf_runtime.hip, reproduces the digests
recorded from zf_flow_create before the image had a unit of its own
(tests/host/flow_image_digests.json) and holds the per-op launch flags to the
loops launch_flow used to run."""

import json
import re
import subprocess
from pathlib import Path

import pytest

from zenflow_amd import build

HOST = Path(__file__).resolve().parent / "host"


def test_image_unit_is_host_only():
    text = (build.CSRC / "zf_flow_image.hip").read_text() + (build.CSRC / "zf_flow_image.h").read_text()
    assert "zf_flow_image.hip" in build.SOURCES
    code = re.sub(r"//.*", "", text)
    assert not re.search(r"getenv|__global__|__device__|\bhip[A-Z]\w*\s*\(", code)
    assert sorted(set(re.findall(r'#include "([^"]+)"', code))) == ["../../include/zenflow_amd.h", "zf_flow_image.h", "zf_internal.h"]


@pytest.mark.skipif(not Path(build.HIPCC).exists(), reason=f"no compiler at {build.HIPCC}")
def test_flow_image_digests(tmp_path):
    exe = tmp_path / "flow_image_check"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC") and not f.startswith("--offload-arch")]
    sources = [HOST / "flow_image_check.cpp", build.CSRC / "zf_flow_image.hip", build.CSRC / "zf_runtime.hip"]
    cmd = [build.HIPCC, "--cuda-host-only", *flags, f"-I{build.CSRC}", "-o", str(exe), *map(str, sources)]
    subprocess.run(cmd, check=True, cwd=tmp_path)
    run = subprocess.run([str(exe)], capture_output=True, text=True, cwd=tmp_path)
    assert run.returncode == 0, run.stderr
    got = json.loads(run.stdout)
    want = json.loads((HOST / "flow_image_digests.json").read_text())
    assert list(got) == list(want)
    for name in want:
        assert got[name] == want[name], name
