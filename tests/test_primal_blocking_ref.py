"""The plain-Python restatement of the stay-on-goal blocking penalty
(tests/primal_blocking_ref.py) against the reference's own outputs
(tests/golden/primal_blocking/pb_*.npz, pbq_*.npz).  Rewards as fp64 bit patterns."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN
from primal_blocking_ref import BlockingWorld, bfs_dist, rooms_world

BLOCKING = os.path.join(GOLDEN, "primal_blocking")
PB = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(BLOCKING, "pb_*.npz")))
PBQ = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(BLOCKING, "pbq_*.npz")))


def _load(name):
    with np.load(os.path.join(GOLDEN if name.startswith("pd_") else BLOCKING, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_sets_are_there():
    assert len(PB) >= 18 and len(PBQ) >= 6
    n_stay = n_pen = 0
    for name in PB:
        fx = _load(name)
        n_stay += int(((fx["action"] == 0) & fx["on_goal"]).sum())
        n_pen += int(fx["blocking"].sum())
        assert np.array_equal(fx["blocking"], fx["n_blocking"] > 0)
        assert os.path.getsize(os.path.join(BLOCKING, name + ".npz")) < 64 * 1024
    assert n_stay >= 100 and n_pen >= 40


@pytest.mark.parametrize("name", PB)
def test_restatement_matches_reference_calls(name):
    fx = _load(name)
    w = BlockingWorld(fx["grid"], fx["starts"], fx["goals"], size=int(fx["size"]),
                      diagonal=bool(fx["diagonal"]))
    for k in range(len(fx["agent"])):
        maps, vec, r, done, mask, on_goal, blocking, valid = w.step(int(fx["agent"][k]) - 1,
                                                                    int(fx["action"][k]))
        assert np.float64(r).view(np.uint64) == fx["reward"][k].view(np.uint64), k
        assert blocking == bool(fx["blocking"][k]) and w.last_n == int(fx["n_blocking"][k]), k
        assert done == bool(fx["done"][k]) and mask == int(fx["next_mask"][k]), k
        assert on_goal == bool(fx["on_goal"][k]) and valid == bool(fx["valid"][k]), k
        assert np.array_equal(np.array(w.pos, dtype=np.int32), fx["pos"][k]), k


@pytest.mark.parametrize("name", PBQ)
def test_restatement_matches_reference_counts(name):
    fx = _load(name)
    for pos, counts in zip(fx["states"], fx["counts"]):
        w = BlockingWorld(fx["grid"], pos, fx["goals"], size=int(fx["size"]),
                          diagonal=bool(fx["diagonal"]))
        assert [w.blocking_count(a) for a in range(len(pos))] == counts.tolist()


def test_bfs_and_rooms_helpers():
    walls = {(1, c) for c in range(1, 6)}
    assert bfs_dist(walls, 3, 7, (0, 0), (2, 0)) == 2
    assert bfs_dist(walls | {(1, 0)}, 3, 7, (0, 0), (2, 0)) == 14
    assert bfs_dist(walls | {(1, 0), (1, 6)}, 3, 7, (0, 0), (2, 0)) is None
    assert bfs_dist(walls | {(2, 0)}, 3, 7, (0, 0), (2, 0)) is None
    assert bfs_dist(walls, 3, 7, (0, 3), (0, 3)) == 0
    grid, starts, goals, doors = rooms_world(np.random.default_rng(1), 14, 14, 10, 4)
    assert len(set(starts)) == 10 and len(set(goals)) == 10 and len(doors) == 4
    assert all(grid[p] == 0 for p in starts + goals)
    assert all(starts[a] == goals[a] for a in doors)
    # every room is reachable from every other: all free cells form one component
    free = {(r, c) for r in range(14) for c in range(14) if grid[r, c] == 0}
    blocked = {(r, c) for r in range(14) for c in range(14)} - free
    assert all(bfs_dist(blocked, 14, 14, (0, 0), p) is not None for p in free)
