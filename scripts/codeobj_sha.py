#!/usr/bin/env python3
"""sha256 of the device code of every translation unit, reproducibly.

A device-only compile with a fixed compilation-unit id gives the same bytes
from any directory, so a refactor that must not move a kernel is checked by
comparing this listing between two checkouts (plain ``.o`` files differ
between directories and cannot be compared):

    python scripts/codeobj_sha.py                         > new.txt
    python scripts/codeobj_sha.py --csrc ../parent/zenflow_amd/csrc > old.txt
    diff old.txt new.txt

Each unit is compiled with ``build.FLAGS`` minus ``-shared``, the unit's own
``_src_flags`` and ``--cuda-device-only -cuid=zf -c``.  ``--csrc DIR`` points
at another checkout's ``zenflow_amd/csrc``; its ``include`` is taken from the
same checkout.  No GPU is needed.
"""

from __future__ import annotations

import argparse
import hashlib
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from zenflow_amd import build  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--csrc", type=Path, default=build.CSRC, help="csrc directory of the checkout to hash")
    ap.add_argument("--jobs", type=int, default=int(os.environ.get("MAX_JOBS", min(16, os.cpu_count() or 1))))
    ap.add_argument("extra", nargs="*", help="further compiler flags, e.g. -DZF_X3_TRACE=1")
    args, unknown = ap.parse_known_args()
    csrc = args.csrc.resolve()
    include = csrc.parent.parent / "include"
    flags = [f for f in build.FLAGS if f != "-shared" and f != f"-I{build.INCLUDE}"] + [f"-I{include}"]
    flags += list(args.extra) + unknown

    with tempfile.TemporaryDirectory() as tmp:

        def sha(src: str) -> str:
            obj = Path(tmp) / (Path(src).stem + ".o")
            cmd = [build.HIPCC, *flags, *build._src_flags(src), "--cuda-device-only", "-cuid=zf", "-c", "-o", str(obj), str(csrc / src)]
            subprocess.run(cmd, check=True, cwd=tmp)
            return hashlib.sha256(obj.read_bytes()).hexdigest()

        with ThreadPoolExecutor(max(1, args.jobs)) as pool:
            for src, digest in zip(build.SOURCES, pool.map(sha, build.SOURCES)):
                print(f"{digest}  {src}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
