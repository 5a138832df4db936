"""Host side of the data-parallel ConditionTrainer, no device needed:
``nn.shard_sets``, the reduction schedule the bitwise GPU tests
(tests/test_gpu_condnet_dp.py) rest on, and the Python argument checks that
fire before any library call."""

import numpy as np
import pytest

from zenflow_amd import nn
from zenflow_amd.dist import leaf_tree_colsum, shard_rows, tree_sum


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def test_shard_sets_ragged():
    lengths = [1, 0, 63, 64, 65, 9, 30, 4, 7, 5, 6, 2, 40, 3, 0, 17, 80, 1, 33, 12, 64, 21, 9]
    off = _offsets(lengths)
    assert nn.shard_sets(off, 0, 2) == (0, 12, 0, 256)
    assert nn.shard_sets(off, 1, 2) == (12, 23, 256, 536)
    assert nn.shard_sets(off, 0, 1) == (0, 23, 0, 536)
    assert nn.shard_sets(list(off), 2, 3) == (16, 23, int(off[16]), 536)  # 8 + 8 + 7 sets
    # the flow's rows are the sets: the same split as dist.shard_rows
    for world in (1, 2, 3, 4, 7):
        for rank in range(world):
            assert nn.shard_sets(off, rank, world)[:2] == shard_rows(len(lengths), rank, world)


@pytest.mark.parametrize("lengths,world", [([5, 0, 0, 3], 2), ([0, 0, 7], 3), ([4, 4], 5), ([0], 2), ([3, 1, 2, 9, 0], 4)])
def test_shard_sets_cover_every_set_and_row_once(lengths, world):
    """Empty sets, empty ranks (more ranks than sets): the ranks' ranges are
    contiguous, in order, and their union is every set and every row once."""
    off = _offsets(lengths)
    parts = [nn.shard_sets(off, r, world) for r in range(world)]
    assert parts[0][0] == 0 and parts[0][2] == 0
    assert parts[-1][1] == len(lengths) and parts[-1][3] == off[-1]
    for (s0, s1, r0, r1), nxt in zip(parts, parts[1:] + [None]):
        assert 0 <= s0 <= s1 and 0 <= r0 <= r1 and (r0, r1) == (off[s0], off[s1])
        if nxt is not None:
            assert (s1, r1) == (nxt[0], nxt[2])
    if world > len(lengths):
        assert any(s0 == s1 for s0, s1, _, _ in parts)
    sets = np.concatenate([np.arange(s0, s1) for s0, s1, _, _ in parts])
    rows = np.concatenate([np.arange(r0, r1) for _, _, r0, r1 in parts])
    assert np.array_equal(sets, np.arange(len(lengths))) and np.array_equal(rows, np.arange(off[-1]))


def test_shard_sets_rejects():
    off = _offsets([3, 4])
    for rank, world in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError, match="rank"):
            nn.shard_sets(off, rank, world)
    for bad in ([0, 5, 3], [-1, 2], [0.5, 2], [4], np.zeros((2, 2), np.int64)):
        with pytest.raises(ValueError):
            nn.shard_sets(bad, 0, 2)


@pytest.mark.parametrize("rows,world", [(512, 2), (2048, 2), (2048, 4), (65536, 2)])
def test_equal_shards_reproduce_the_one_device_tree(rows, world):
    """The ranks' subtree roots of leaf_tree_colsum over their rows / world
    rows, combined by tree_sum, are the one-device leaf_tree_colsum of all
    rows bit for bit: what cn_combine and the gradient close do with the
    all-gathered roots (values over 80 binades, so any other order shows)."""
    rng = np.random.default_rng(rows + world)
    x = (rng.standard_normal((rows, 3)) * np.exp2(rng.integers(-40, 40, (rows, 3)))).astype(np.float32)
    one = leaf_tree_colsum(x, rows, 1)
    roots = [leaf_tree_colsum(x[slice(*shard_rows(rows, r, world))], rows, world) for r in range(world)]
    assert np.array_equal(tree_sum(roots), one)
    # and the plain float64 sum in row order is another number
    assert not np.array_equal(np.cumsum(x.astype(np.float64), axis=0)[-1], one)


def _bare(world=1, rank=0, optimizer=None):
    """A ConditionTrainer without a handle: what the checks below read."""
    ct = nn.ConditionTrainer.__new__(nn.ConditionTrainer)
    ct.world, ct.rank, ct.optimizer, ct.in_dim = world, rank, optimizer, 2
    return ct


def test_forward_checks_its_shard_before_anything_else():
    x = np.zeros((8, 2), np.float32)
    ct = _bare(world=2, rank=1)
    with pytest.raises(ValueError, match="go together"):
        ct.forward(x, [0, 8], global_rows=16)
    with pytest.raises(ValueError, match="go together"):
        ct.forward(x, [0, 8], row_base=8)
    assert ct._shard(8, None, None) == (16, 8)  # the equal-shard defaults
    assert ct._shard(8, 20, 3) == (20, 3)
    for g, b in ((7, 0), (16, -1), (16, 9)):
        with pytest.raises(ValueError, match="global_rows"):
            ct.forward(x, [0, 8], global_rows=g, row_base=b)
    one = _bare()
    assert one._shard(8, None, None) == (8, 0) and one._shard(8, 8, None) == (8, 0)
    with pytest.raises(ValueError, match="global_rows"):
        one.forward(x, [0, 8], global_rows=16, row_base=0)


def test_load_opt_state_checks_the_slot_count():
    from zenflow_amd import optim
    from zenflow_amd.train import nadamw

    state = {"count": 3, "slots": [{}]}
    with pytest.raises(ValueError, match="1 moment arrays, this optimiser keeps 2"):
        _bare(optimizer=nadamw()).load_opt_state(state)
    with pytest.raises(ValueError, match="2 moment arrays, this optimiser keeps 1"):
        _bare(optimizer=optim.sgd(1e-2, momentum=0.9)).load_opt_state(dict(state, slots=[{}, {}]))
