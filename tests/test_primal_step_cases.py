"""What the PRIMAL step cases (tests/primal_step_cases.py) cover, checked on the
restatement alone -- no device: the scripts finish worlds and un-finish them, every reward
class and status occurs, corner cases reach every corner / side, the comparer can fail and
names what differs, and the dispatch rule reproduces the instance every case names.
tests/test_gpu_primal_step_shapes.py runs the same cases on the device."""
import numpy as np
import pytest

import primal_step_cases as psc
from primal_step_cases import BOTTOM, CASES, LEFT, RIGHT, TOP, build, case_id, compare, expected_kernel

# the lane-rule cases have K = 3 calls per world and E in the thousands: their worlds
# start finished, so that three calls can un-finish and re-finish them
SHORT = [c for c in CASES if c.K < 70]


def _bits(x):
    return np.asarray(x, np.uint64).view(np.float64)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_scripts_cover_finished_worlds_rewards_and_edges(c):
    b = build(c)
    done, st, act = b["done"].astype(int), b["status"], b["actions"]
    rew = _bits(b["reward"])
    finished = done.any(1)
    assert 2 * finished.sum() >= c.E, "worlds with done = 1: %d of %d" % (finished.sum(), c.E)
    again = 0
    for e in range(c.E):
        flips = np.flatnonzero(np.diff(done[e]))
        first_one = int(np.argmax(done[e])) if done[e].any() else c.K
        again += (flips >= first_one).sum() >= 2      # 1 -> 0 -> 1 after the first done = 1
    assert again >= 1, "no world goes done 1 -> 0 -> 1"
    move = act != 0
    classes = {
        "-0.3 moved": move & (rew == -0.3) & np.isin(st, (0, 2)),
        "-0.5 idle": ~move & (rew == -0.5) & (st == 0),
        "-2 wall": move & (rew == -2.0) & (st == -2),
        "-2 robot": move & (rew == -2.0) & (st == -3),
        "0.0 arrived": move & (rew == 0.0) & (st == 1),
        "0.0 stayed on goal": ~move & (rew == 0.0) & (st == 1),
        "status 2 left goal": st == 2,
    }
    missing = [k for k, v in classes.items() if not v.any()]
    assert not missing, missing
    if c.diag:
        assert b["mid"].any(), "no move refused by the midpoint test alone"
        assert b["mid_mask"].any(), "no next_mask bit removed by the midpoint test alone"
    if c.corners:
        at = b["at"].reshape(-1, 2)
        for cell in ((0, 0), (0, c.W - 1), (c.H - 1, 0), (c.H - 1, c.W - 1)):
            assert ((at[:, 0] == cell[0]) & (at[:, 1] == cell[1])).any(), "corner %s never occupied" % (cell,)
        for side in (TOP, BOTTOM, LEFT, RIGHT):
            assert (b["oob"] & side).any(), "no out-of-bounds move on side %d" % side
            # a window that covers every row from wherever it stands clamps no goal to its
            # top or bottom: the 8 x 2048 world at s = 32 (16 rows each way) has no such record
            if side in (TOP, BOTTOM) and c.H < c.s // 2 + 2:
                assert not (b["clamp"] & side).any()
                continue
            assert (b["clamp"] & side).any(), "no visible goal clamped to side %d" % side


@pytest.mark.parametrize("c", SHORT, ids=case_id)
def test_lane_rule_cases_put_distinct_worlds_in_every_wave(c):
    """E worlds cycle through 509 distinct ones: a prime, so no two waves (4, 2 or 1
    worlds each) hold the same worlds in the same lanes; every world is compared."""
    b = build(c)
    assert b["distinct"] == 509 and c.E > 8 * 509 and c.K == 3
    assert len(np.unique(b["ids"][:509] * 16 + b["actions"][:509], axis=0)) > 100


@pytest.mark.parametrize("c", [c for c in CASES if c.name.startswith("abi-")], ids=case_id)
def test_chunked_launches_start_on_finished_worlds(c):
    """The C-ABI cases are also run as launches of 1, 63, 64 and 2 calls: the launches
    that begin at calls 64 and 128 find finished worlds (the kernel recounts the agents
    on their goals from pos at every launch) and worlds that are not."""
    done = build(c)["done"]
    assert c.K == 130 and c.E == 9
    for k in (64, 128):
        assert done[:, k - 1].any() and done[:, k].any() and not done[:, k].all()


def _case_arrays(c):
    b = build(c)
    want = {k: b[k] for k in psc.FIELDS}
    want["pos"], want["past"] = b["pos"], b["past"]
    got = {k: np.array(v) for k, v in want.items()}
    got["reward"] = got["reward"].view(np.float64)      # as the device returns them
    got["vec"] = got["vec"].view(np.float64)
    return got, want


def test_compare_names_each_flipped_element():
    c = next(x for x in CASES if x.name == "seq8" and x.diag)
    got, want = _case_arrays(c)
    assert compare(got, want) is None
    flips = [("reward", (4, 17), 1 << 0), ("done", (2, 5), 1), ("next_mask", (8, 69), 1 << 8),
             ("on_goal", (0, 0), 1), ("valid", (3, 64), 1), ("vec", (5, 63, 2), 1 << 51)]
    flips += [("obs", (6, 33, p, 3, 5), 1) for p in range(4)]
    for field, idx, bit in flips:
        g = dict(got)
        g[field] = got[field].copy()
        raw = g[field].view(np.uint64) if g[field].dtype == np.float64 else g[field]
        raw[idx] ^= np.array(bit).astype(raw.dtype)
        d = compare(g, want)
        inner = {"vec": idx[2:], "obs": idx[2:]}.get(field, ())
        flat = int(np.ravel_multi_index(inner, (3,) if field == "vec" else (4, c.s, c.s))) if inner else 0
        assert d is not None and (d.world, d.call, d.field, d.index) == (idx[0], idx[1], field, flat), (field, d)
        assert d.got != d.want
    for field in ("pos", "past"):
        g = dict(got)
        g[field] = got[field].copy()
        g[field][7, c.N - 1, 1] += 1
        d = compare(g, want)
        assert (d.world, d.call, d.field, d.index) == (7, -1, field, 2 * (c.N - 1) + 1), d
    # the earliest (world, call) wins, and calls from `upto` on are not looked at
    g = dict(got)
    g["done"], g["valid"] = got["done"].copy(), got["valid"].copy()
    g["done"][3, 9] ^= 1
    g["valid"][3, 8] ^= 1
    assert compare(g, want)[:3] == (3, 8, "valid")
    assert compare(g, want, upto=9)[:3] == (3, 8, "valid")
    assert compare(g, want, upto=8) is None
    upto = np.full(c.E, c.K)
    upto[3] = 8
    assert compare(g, want, upto=upto) is None
    # an output that was not produced is not compared
    assert compare({k: v for k, v in g.items() if k in ("obs", "pos")}, want) is None


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_dispatch_rule_names_the_cases_instance(c):
    assert expected_kernel(c.H, c.W, c.N, c.s, c.E, c.diag, c.lanes, c.path, True) == c.kernel


def test_dispatch_rule_table():
    """The instance column of the case table, written out (the cases carry the same names:
    this keeps a change of both from going unnoticed), the obs-alignment fallback, and
    all 8 + 24 instances reached."""
    rows = [
        (11, 9, 5, 6, 9, False, "", "", "primal_seq_kernel<6, false>"),
        (13, 16, 9, 8, 9, True, "", "", "primal_seq_kernel<8, true>"),
        (54, 54, 64, 10, 9, True, "", "", "primal_seq_kernel<10, true>"),
        (60, 60, 64, 4, 9, False, "", "", "primal_seq_kernel<4, false>"),
        (55, 20, 8, 10, 9, False, "", "", "primal_act_kernel<10, 6, false, 1>"),
        (20, 55, 8, 10, 9, True, "", "", "primal_act_kernel<10, 6, true, 1>"),
        (20, 20, 65, 10, 9, False, "", "", "primal_act_kernel<10, 6, false, 4>"),
        (61, 30, 6, 4, 9, False, "", "", "primal_act_kernel<0, 6, false, 1>"),
        (70, 70, 16, 10, 9, False, "", "", "primal_act_kernel<10, 6, false, 1>"),
        (12, 12, 6, 10, 9, False, "", "groups", "primal_act_kernel<10, 6, false, 1>"),
        (5, 5, 2, 3, 4093, False, "", "", "primal_act_kernel<0, 6, false, 1>"),
        (5, 5, 2, 3, 4096, False, "", "", "primal_act_kernel<0, 5, false, 1>"),
        (5, 5, 2, 3, 8188, False, "", "", "primal_act_kernel<0, 5, false, 1>"),
        (5, 5, 2, 3, 8189, False, "", "", "primal_act_kernel<0, 4, false, 1>"),
        (12, 12, 4, 10, 8192, False, "", "groups", "primal_act_kernel<10, 4, false, 1>"),
        (8, 2048, 6, 32, 3, False, "", "", "primal_act_kernel<0, 6, false, 1>"),
        (2, 8000, 5, 3, 9, True, "", "", "primal_act_kernel<0, 6, true, 1>"),
        (128, 128, 255, 32, 3, True, "", "", "primal_act_kernel<0, 6, true, 4>"),
        (120, 120, 8, 10, 9, False, "16", "", "primal_act_kernel<10, 5, false, 1>"),
        (7, 7, 3, 1, 9, False, "", "", "primal_act_kernel<0, 6, false, 1>"),
        (7, 7, 3, 2, 9, True, "", "", "primal_act_kernel<0, 6, true, 1>"),
        (20, 20, 6, 12, 9, False, "", "", "primal_act_kernel<0, 6, false, 1>"),
        (12, 12, 17, 7, 9, False, "16", "", "primal_act_kernel<0, 4, false, 4>"),
    ]
    for H, W, N, s, E, diag, lanes, path, name in rows:
        assert expected_kernel(H, W, N, s, E, diag, lanes, path, True) == name, (H, W, N, s, E)
    assert expected_kernel(32, 32, 16, 10, 9, False) == "primal_seq_kernel<10, false>"
    assert expected_kernel(32, 32, 16, 10, 9, False, obs_aligned=False) == "primal_act_kernel<10, 6, false, 1>"
    reached = {c.kernel for c in CASES}
    assert len({k for k in reached if k.startswith("primal_seq")}) == 8
    assert len({k for k in reached if k.startswith("primal_act")}) == 24
    # the 8 x 2048, s = 32 world needs the > 64 KB attribute path, 1 x 16384 is past 160 KB
    assert 65536 < psc.world_lds(8, 2048, 6, 32) <= 160 * 1024 < psc.world_lds(1, 16384, 2, 32)
