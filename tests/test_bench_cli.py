"""bench.py --dump-outputs DIR: the last timed step's outputs as .npy files,
whole or cut to the same seeded row sample from run to run."""

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def test_dump_outputs_small_arrays_whole(tmp_path):
    import bench

    lp = np.arange(1000, dtype=np.float32)
    bench.dump_outputs(tmp_path / "d", {"log_prob": lp, "nll": np.array([1.5], np.float64)}, 0, 1)
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == ["log_prob.npy", "nll.npy"]
    got = np.load(tmp_path / "d" / "log_prob.npy")
    assert got.dtype == np.float32 and np.array_equal(got, lp)
    nll = np.load(tmp_path / "d" / "nll.npy")
    assert nll.dtype == np.float64 and nll.tolist() == [1.5]


def test_dump_outputs_samples_large_arrays_the_same_way(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    x = np.random.default_rng(0).standard_normal((1000, 4))  # float64, 32000 bytes
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, {"x": x}, 0, 1)
    a, b = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    assert a.dtype == np.float64 and a.shape == (128, 4) and a.nbytes <= 4096
    assert np.array_equal(a, b)
    # rows of x, in row order
    idx = [int(np.flatnonzero((x == r).all(axis=1))[0]) for r in a]
    assert idx == sorted(set(idx))
    # one file per rank when there are several, each within its share
    bench.dump_outputs(tmp_path / "c", {"x": x}, 1, 2)
    c = np.load(tmp_path / "c" / "x_rank1.npy")
    assert c.nbytes <= 2048 and not (tmp_path / "c" / "x.npy").exists()
