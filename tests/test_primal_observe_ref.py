"""The CPU restatement as a checker of ALL-AGENT queries: oracle.mapf_oracle.primal_obs
(..., agents=...), PrimalWorld.next_mask and PrimalWorld.done against every snapshot the
reference recorded (tests/golden/primal_observe/po_*.npz, written by
tests/golden/gen_primal_observe_fixtures.py): `_observe` (:343-386) of every agent,
`_listNextValidActions` (:639-667) for every previous action, on_goal and `_complete`.
Bit-exact, goal vectors as fp64 bit patterns."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle.mapf_oracle import primal_obs
from oracle.primal_dyn_oracle import PrimalWorld

PO_DIR = os.path.join(GOLDEN, "primal_observe")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(PO_DIR, "po_*.npz")))


def load_po(name):
    with np.load(os.path.join(PO_DIR, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_set():
    """The cases the restatement and the device are held to."""
    assert FIXTURES == ["po_crowd6_n12", "po_diag_crowd6_n14", "po_diag_rand16_n20", "po_rand10_n8",
                        "po_rand16_n20", "po_rect5x9_n4", "po_script_goals"]
    fx = load_po("po_script_goals")
    assert fx["done"].any() and not fx["done"].all()
    # an agent standing on another agent's goal
    assert any((fx["pos"][i, a] == fx["goals"][b]).all() for i in range(len(fx["snap_at"]))
               for a in range(3) for b in range(3) if a != b)
    for name in ("po_diag_crowd6_n14", "po_diag_rand16_n20"):
        fx = load_po(name)
        assert bool(fx["diagonal"]) and ((fx["pos"] != fx["past"]).any(2).sum(1) >= 3).any()


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_reference_snapshots(name):
    fx = load_po(name)
    diag, s = bool(fx["diagonal"]), int(fx["size"])
    n, nact = len(fx["starts"]), 9 if diag else 5
    w = PrimalWorld(fx["grid"], fx["starts"], fx["goals"], s, diagonal=diag)
    snaps = {int(k): i for i, k in enumerate(fx["snap_at"])}
    for k in range(len(fx["agent"]) + 1):
        if k in snaps:
            i = snaps[k]
            assert np.array_equal(np.array(w.pos), fx["pos"][i]), k
            assert np.array_equal(np.array(w.past), fx["past"][i]), k
            maps, vec = primal_obs(w.grid, w.pos, w.goals, s, agents=list(range(n)))
            assert np.array_equal(maps, fx["obs"][i]), k
            assert np.array_equal(vec.view(np.uint64), fx["vec"][i].view(np.uint64)), k
            for a in range(n):
                assert [w.next_mask(a, p) for p in range(nact)] == fx["next_mask"][i, a].tolist(), (k, a)
                assert (w.pos[a] == w.goals[a]) == bool(fx["on_goal"][i, a]), (k, a)
            assert w.done() == bool(fx["done"][i]), k
        if k < len(fx["agent"]):
            w.move(int(fx["agent"][k]) - 1, int(fx["action"][k]))
