"""What the graph-replay selection and episodes (tests/graph_replay_cases.py) hold, checked
without a device and without libmapfx.so: the selection reaches every launch class -- computed
from the case tables' own dispatch restatements, never from a name --, the three episodes of
every selected case differ where a graph that replays what it saw at capture time would be
caught, each family's `compare` can fail on them, and the `episode` helpers of the case
modules run the code path `build` runs.  tests/test_gpu_graph_replay.py replays the same
cases on the device.
"""
import itertools

import numpy as np
import pytest

import graph_replay_cases as grc
import mapf_step_cases as msc
import partial_step_cases as psc
import primal_step_cases as qsc
from graph_replay_cases import CLASSES, SELECTED, case_id, differing, episodes, members, of_family

OUTPUT_ARRAYS = {"mapf": ("avail", "term", "obs_full", "obs_window", "obs_window_occ", "obs_primal", "primal_vec"),
                 "partial": ("obs", "state", "avail"),
                 "primal": ("obs", "vec", "next_mask", "on_goal", "valid")}


@pytest.fixture(scope="module", autouse=True)
def _built():
    from oracle import corc
    corc.lib()


# ------------------------------------------------------------------ selection
@pytest.mark.parametrize("cl", CLASSES, ids=lambda cl: "%s: %s" % (cl.family, cl.name))
def test_selection_reaches_the_class(cl):
    got = members(cl)
    assert len(got) >= cl.need, (cl.name, [c.name for c in got])
    assert all(grc.eligible(cl.family, c) for c in got)


def test_selection_size_and_limits():
    assert 35 <= len(SELECTED) <= 45, len(SELECTED)
    assert len(set(SELECTED)) == len(SELECTED)
    for f, c in SELECTED:
        assert c.E <= 131, case_id(f, c)
        if f != "primal":
            assert c.T <= 40, case_id(f, c)
    for c in of_family("partial"):          # the workgroup cases: E = 3 to 5
        if psc.family(c) == "workgroup":
            assert 3 <= c.E <= 5, c


def test_selection_by_the_tables_own_dispatch():
    """The classes once more, straight from expected_kernel / expected_action_path / family."""
    mapf = of_family("mapf")
    own = {c: dict(msc.case_launches(c))[c.entry] for c in mapf}
    wave_step = [c for c in mapf if c.entry == "step" and msc.expected_kernel(c)[0] == "mapf_wave_kernel"]
    assert {own[c]["fullw"] for c in wave_step} == {True, False}
    assert any(c.entry == "observe" and msc.expected_kernel(c)[0] == "mapf_wave_kernel" for c in mapf)
    roll = [c for c in mapf if c.entry == "rollout"]
    assert any(own[c]["path"] == "wave" and not own[c]["runner"] and c.act == "gen" and c.env_offset and c.t0
               for c in roll)
    assert any(own[c]["runner"] and own[c]["path"] == "wave" and not own[c]["split"] for c in roll)
    split = [c for c in roll if own[c]["split"]]
    assert {msc.expected_action_path(c) for c in split} == {0, 1, 2}
    assert {c.N for c in split if msc.expected_action_path(c) == 2} == {16, 64}
    path1 = [c for c in split if msc.expected_action_path(c) == 1]
    assert any(c.act == "int8" and c.act_off % 16 for c in path1)
    assert {"int32", "int64"} & {c.act for c in path1}
    assert all(c.act == "gen" for c in split if msc.expected_action_path(c) == 0)
    assert any(c.autoreset for c in split)
    kinds = {(c.entry, msc.expected_kernel(c)[0], msc.expected_kernel(c)[1].split(",")[0]) for c in mapf}
    assert ("step", "mapf_step_kernel", "unsignedchar") in kinds
    assert ("rollout", "mapf_rollout_kernel", "unsignedchar") in kinds
    assert any(c.entry == "step" and msc.expected_kernel(c)[1].startswith("unsignedshort,")
               and int(msc.expected_kernel(c)[1].split(",")[1]) > 1 for c in mapf)
    assert any(c.entry == "rollout" and msc.expected_kernel(c)[0] == "mapf_rollout_kernel"
               and msc.case_geometry(c).fold_R == 8 for c in mapf)
    assert {c.shared for c in mapf} == {True, False}
    part = of_family("partial")
    fast = [c for c in part if psc.family(c) == "fast"]
    assert any(psc.table_bytes(c.H, c.W) == 1 and psc.expected_geometry(c)["sqrt_table"] for c in fast)
    assert {psc.table_bytes(c.H, c.W) for c in fast} == {1, 2, 4}
    assert any(psc.table_bytes(c.H, c.W) == 4 and psc.expected_geometry(c)["EPW"] == 1 for c in fast)
    assert any(psc.family(c) == "generic" for c in part)
    wg = {psc.expected_step_kernel(c)[1].split(",")[1] for c in part
          if psc.expected_step_kernel(c)[0] == "partial_wg_kernel"}
    assert "1" in wg and wg - {"1"}
    assert {psc.expected_bfs_kernel(c)[0] for c in part} == {k for k, _ in psc.ALL_BFS_KERNELS}
    masked = [c for c in part if grc.has_masked_reset(c)]
    assert sorted(psc.family(c) for c in masked) == ["fast", "generic", "workgroup"]
    prim = of_family("primal")
    for c in prim:
        assert qsc.expected_kernel(c.H, c.W, c.N, c.s, c.E, c.diag, c.lanes, c.path) == c.kernel
    assert any("primal_seq_kernel" in c.kernel for c in prim)
    assert len({grc._primal_ls(c) for c in prim if "primal_act_kernel" in c.kernel and not c.diag}) >= 2
    assert any(c.diag for c in prim)


# ------------------------------------------------------------------ episodes
@pytest.mark.parametrize("fc", SELECTED, ids=lambda fc: case_id(*fc))
def test_episodes_differ_pairwise(fc):
    """After step 0 and after the last step, every pair of A, B, C differs in pos, in one of
    reward / node / edge and in an output array: a graph that replays the actions (or the
    state) it saw at capture time cannot pass two replays.  B and C hold valid actions only;
    A is the table's episode, refused action included."""
    f, c = fc
    eps = episodes(f, c)
    assert [e.name for e in eps] == ["A", "B", "C"]
    for ea, eb in itertools.combinations(eps, 2):
        for k in (0, -1):
            names = set(differing(f, c, ea, eb, k))
            assert grc.separates(names), (ea.name, eb.name, k, sorted(names))
            assert names & set(OUTPUT_ARRAYS[f]), (ea.name, eb.name, k, sorted(names))
    for ep in eps[1:]:
        hi = (9 if c.diag else 5) if f == "primal" else 5
        assert ep.actions.min() >= 0 and ep.actions.max() < hi
        assert ep.bad is None
    if f == "mapf":
        assert (eps[0].bad is None) == (c.act == "gen")
        if c.act == "gen":          # the generator's actions are the call's: the starts differ
            assert all(np.array_equal(e.actions, eps[0].actions) for e in eps)
            assert all(not np.array_equal(x.start, y.start) for x, y in itertools.combinations(eps, 2))
        else:
            assert all(not np.array_equal(x.actions, y.actions) for x, y in itertools.combinations(eps, 2))
    if f == "partial" and grc.has_masked_reset(c):
        assert all(len(e.snaps) == c.T + 2 for e in eps)
        m = grc.reset_masks(c)
        assert m["A"].all() and not m["C"].any() and 0 < m["B"].sum() < c.E


def _device_shaped(f, c, ep, k):
    """An episode's snapshot after its call k as the device would hold it: (what `compare`
    takes first, the want it is checked against is another episode's)."""
    if f == "mapf":
        return grc.mapf_step_arrays(c, ep.snaps[k + 1])
    if f == "partial":
        return psc.as_device(c, ep.snaps[k + 1])
    got = {n: ep.snaps[n] for n in qsc.FIELDS}
    got["pos"], got["past"] = ep.snaps["pos"], ep.snaps["past"] if c.diag else None
    return got


def _compare(f, c, got, ep, k):
    if f == "mapf":
        return msc.compare(got, ep.snaps[k + 1], k)
    if f == "partial":
        return psc.compare(got[0], got[1], ep.snaps[k + 1], k)
    return qsc.compare(got, ep.snaps)


@pytest.mark.parametrize("fc", SELECTED, ids=lambda fc: case_id(*fc))
def test_compare_names_a_difference_between_episodes(fc):
    """Negative control: B's data in the device's shapes against A's snapshots is a Diff,
    against its own snapshots it is None."""
    f, c = fc
    a, b, _ = episodes(f, c)
    for k in (0,) if f == "primal" else (0, len(b.snaps) - 2):
        got = _device_shaped(f, c, b, k)
        assert _compare(f, c, got, b, k) is None
        d = _compare(f, c, got, a, k)
        assert d is not None and d.field in (msc.FIELDS + psc.FIELDS + qsc.FIELDS + ("pos", "past")), d


# ------------------------------------------------------------------ the helpers' code path
def test_episode_helpers_run_the_path_build_runs():
    """`episode` given a built case's own actions returns the built episode (MAPF: a
    generator case, whose actions hold no refused one; its `start` = init_pos changes nothing)."""
    c = next(c for c in of_family("mapf") if c.act == "gen")
    b = msc.build(c)
    snaps, final, bad = msc.episode(c, b, np.array(b["actions"]), start=b["init_pos"])
    assert bad is None and len(snaps) == len(b["snaps"])
    for k, (s, w) in enumerate(zip(snaps, b["snaps"])):
        assert msc.compare({f: s[f] for f in msc.FIELDS if f in s}, w, k) is None
    assert all(np.array_equal(final[f], b["final"][f]) for f in final)
    c = of_family("partial")[0]
    b = psc.build(c)
    for s, w in zip(psc.episode(c, b, np.array(b["actions"])), b["snaps"]):
        assert all(np.array_equal(s[f], w[f]) for f in w)
    c = of_family("primal")[0]
    b = qsc.build(c)
    again = qsc.episode(c, b, (b["ids"], b["actions"]))
    assert all(np.array_equal(again[f], b[f]) for f in again)


# ------------------------------------------------------------------ the carried-state form
@pytest.mark.parametrize("family", ["mapf", "partial"])
def test_carry_episode_ends_inside_the_second_replay(family):
    c, limit, ep = grc.carry_episode(family)
    T = c.T
    assert ep.actions.shape == (2 * T, c.E, c.N) and len(ep.snaps) == 2 * T + 1
    assert T < limit < 2 * T
    term = "term" if family == "mapf" else "terminated"
    assert not np.asarray(ep.snaps[T][term]).all()       # some env is live when the first replay ends
    assert np.asarray(ep.snaps[2 * T][term]).all()       # ... and every env has ended after the second
    own = episodes(family, c)[0]
    assert np.asarray(own.snaps[T][term]).all()          # at the case's own limit it would have ended
    assert np.array_equal(np.asarray(ep.snaps[T]["t"]), np.full(c.E, T))
