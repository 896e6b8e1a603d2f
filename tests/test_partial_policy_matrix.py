"""What tests/test_gpu_partial_policy_matrix.py and tests/test_gpu_runner_policy_matrix.py rely
on, from the restatement alone (tests/partial_policy_matrix.py) -- no GPU: the cases reach every
policy-mode kernel instance and no other, every case's own episode takes every branch of its
rule (the failed push and the three-deep chain of the priority-inheritance rule included), the
rule stays collision-free where the descent collides, and the collect cases still end early.
"""
import numpy as np
import pytest

import partial_policy_matrix as pm
from partial_step_cases import FAST_PAIRS, lane_group, table_bytes

PIBT_ALWAYS = ("push", "push_failed", "depth3", "skip_claimed", "skip_parent", "forced_stay")
PIBT_EXPLORE = ("explore_top", "explore_pushed")


# ------------------------------------------------------------------ 1: the instances
@pytest.mark.parametrize("rule", pm.RULES)
def test_rollout_cases_reach_exactly_the_domain(rule):
    domain = pm.rollout_domain(rule)
    assert len(domain) == 23
    by_instance = {}
    for name in pm.ROLLOUT:
        for obs in (True, False):
            by_instance.setdefault(pm.expected_kernel(name, obs, rule), []).append(name)
    assert set(by_instance) == domain, (sorted(domain - set(by_instance)), sorted(set(by_instance) - domain))
    # with the rows: one case per fast instance
    for k, names in by_instance.items():
        if k[1].endswith("true") and ",5," in k[1]:
            assert len(names) == 1, (k, names)


@pytest.mark.parametrize("rule", pm.RULES)
def test_collect_cases_reach_exactly_the_domain(rule):
    domain = pm.collect_domain(rule)
    assert len(domain) == 20
    got = {pm.expected_collect_kernel(pm.collect_shape(n), True, rule) for n in pm.COLLECT}
    assert len(got) == len(pm.COLLECT) == 16, "one case per instance with the rows"
    got |= {pm.expected_collect_kernel(pm.collect_shape(n), False, rule) for n in pm.COLLECT_NO_ROWS}
    assert got == domain, (sorted(domain - got), sorted(got - domain))


def test_int32_tables_are_outside_the_domain():
    """Both rules, rollout and collect, refuse int32 tables on the host (mapfx_partial_rollout,
    mapfx_partial_runner_rollout_offered): no case has them, the restated pick has no answer."""
    for s in list(pm.ROLLOUT.values()) + list(pm.COLLECT.values()):
        assert table_bytes(s.H, s.W) in (1, 2)
    with pytest.raises(KeyError):
        pm._gde(128, 256)
    assert pm._gde(127, 256) == 2 == pm._gde(181, 181) and table_bytes(128, 256) == 4


def test_run_time_shapes_of_the_generic_instances():
    gen = {n: s for n, s in pm.ROLLOUT.items()
           if not (s.K == 5 and (s.win, lane_group(s.N)) in FAST_PAIRS)}
    assert {s.win for s in gen.values()} == set(pm.WINDOWS)
    assert {lane_group(s.N) for s in gen.values()} == {1, 2, 4, 8, 16, 32, 64}
    tw = {(lane_group(s.N), table_bytes(s.H, s.W)) for s in gen.values()}
    assert (64, 2) in tw and any(L <= 4 and b == 2 for L, b in tw) and any(b == 1 for _, b in tw)
    assert any(s.K != 5 and lane_group(s.N) == 32 for s in gen.values())
    assert any(s.K > s.N for s in gen.values())
    # (every case runs with and without the rows: each of these does both)


def test_where_the_lanes_of_a_wave_disagree():
    specs = pm.ROLLOUT
    assert any(s.N == lane_group(s.N) >= 8 for s in specs.values())
    assert any(s.N == lane_group(s.N) // 2 + 1 and s.N >= 5 for s in specs.values())
    geo = {n: pm.geometry(n) for n in specs}
    for n, g in geo.items():        # a last wave with fewer envs than a wave holds, or one env per wave
        assert g["partial_last"] or g["EPW"] == 1, n
    assert sum(g["partial_last"] for g in geo.values()) >= 12
    assert any(g["waves"] > g["wpb"] for g in geo.values()), "more than one block"
    assert geo["f-w5-l16-i16"]["stage_lanes"] == 32 and (specs["f-w5-l16-i16"].H, specs["f-w5-l16-i16"].W) == (64, 60)
    cut = [n for n, g in geo.items() if g["EPW"] < g["full"]]
    assert "f-w7-l16-i16" in cut and "f-w5-l32-i16" in cut
    for n in cut:
        assert table_bytes(specs[n].H, specs[n].W) == 2 and geo[n]["waves"] > geo[n]["wpb"]
    assert all(s.T <= 12 for s in specs.values())


# ------------------------------------------------------------------ the maps
def test_pocket_maps_and_starts():
    shared = per_env = 0
    corners, orient = set(), set()
    for name, s in pm.ROLLOUT.items():
        b = pm.build_case(name)
        shared += s.shared
        per_env += not s.shared
        orient.add(np.sign(s.H - s.W))
        assert b["grids"].shape == ((1 if s.shared else s.E), s.H, s.W)
        for e in range(s.E):
            g = b["grids"][0 if s.shared else e]
            assert g[0, 0] != 0 and ((g[-1] == 0).any() or (g[:, -1] == 0).any()), name
            for arr in (b["starts"][e], b["goals"][e]):
                assert (g[arr[:, 0], arr[:, 1]] == 0).all(), (name, e)
            assert len({tuple(p) for p in b["goals"][e].tolist()}) == s.N
        assert pm.stacked_envs(name) == ([] if s.stacked is None else [s.stacked]), name
        if g[-1, -1] == 0:
            corners.add((s.H, s.W))
        if not s.shared:
            assert not np.array_equal(b["grids"][0], b["grids"][1])
    assert shared >= 6 and per_env >= 6
    assert orient == {-1, 0, 1}
    assert {(127, 256), (256, 127)} <= corners
    # one stacked case per lane group 8, 16, 32, 64 and one on a generic instance below 64
    assert {lane_group(pm.ROLLOUT[n].N) for n in pm.STACKED} == {8, 16, 32, 64}
    assert "g-w7-n7" in pm.STACKED and pm.expected_kernel("g-w7-n7", True, "pibt")[1] == "7,0,0,0,true"


# ------------------------------------------------------------------ 2, 5: the pibt branches
def _assert_pibt_counts(name, counts, eps_q, n_agents, stacked):
    if n_agents == 1:
        assert counts["push"] == 0 and counts["explore_top"] > 0, (name, counts)
        return
    if n_agents == 2:       # no chain of three, no failed push that leaves a second candidate
        assert counts["push"] > 0 and counts["skip_parent"] > 0, (name, counts)
        return
    for k in PIBT_ALWAYS + (PIBT_EXPLORE if eps_q > 0 else ()):
        assert counts[k] > 0, (name, k, counts)
    if stacked:
        assert counts["skip_multi"] > 0, (name, counts)


@pytest.mark.parametrize("name", list(pm.ROLLOUT))
def test_rollout_case_takes_every_pibt_branch(name, record_property):
    s = pm.ROLLOUT[name]
    assert (s.N <= 2) == (name in pm.NO_CHAIN)
    counts = pm.run(name, "pibt", pm.EPS, s.phase)["counts"]
    record_property("pibt_branch_counts", counts)
    print("%s pibt (eps 2^30, %s): %s" % (name, s.phase, counts))
    _assert_pibt_counts(name, counts, pm.EPS, s.N, s.stacked is not None)


@pytest.mark.parametrize("name", list(pm.COLLECT))
def test_collect_case_takes_every_pibt_branch(name, record_property):
    s = pm.COLLECT[name]
    assert (s.N <= 2) == (name in pm.COLLECT_NO_CHAIN)
    counts = pm.collect_reference(name, "pibt", pm.EPS)["counts"]
    record_property("pibt_branch_counts", counts)
    print("%s pibt collect (eps 2^30, two runs): %s" % (name, counts))
    _assert_pibt_counts(name, counts, pm.EPS, s.N, s.stacked)


def test_the_stacked_collect_cases():
    assert {lane_group(pm.COLLECT[n].N) for n in pm.COLLECT_STACKED} == {8, 16, 32, 64}
    assert pm.expected_collect_kernel(pm.collect_shape("cg-w5-n50"), True, "pibt")[1] == "5,0,0,0,true"


# ------------------------------------------------------------------ 3: no collision
@pytest.mark.parametrize("name", list(pm.ROLLOUT))
def test_pibt_is_collision_free_where_descent_collides(name):
    """Fresh episodes: under the rule no env without a stacked start shows a node or edge flag;
    under descent at eps 0 the same instances collide (N = 1 cannot)."""
    s = pm.ROLLOUT[name]
    clean = [e for e in range(s.E) if e != s.stacked]
    r = pm.run(name, "pibt", pm.EPS, "fresh")
    assert r["actions"].min() >= 0 and r["actions"].max() <= 4
    for k, snap in enumerate(r["snaps"]):
        assert not snap["node"][clean].any() and not snap["edge"][clean].any(), k
    assert not r["snaps"][-1]["total_coll"][clean].any()
    d = pm.run(name, "descent", 0, "fresh")
    assert (d["snaps"][-1]["total_coll"] > 0).any() == (s.N > 1)


@pytest.mark.parametrize("name", list(pm.COLLECT))
def test_pibt_collect_is_collision_free_in_the_clean_envs(name):
    """The rows' state column 0 is the env's collision total: 0 in every row of every env but
    the stacked one."""
    s = pm.COLLECT[name]
    ref = pm.collect_reference(name, "pibt", pm.EPS)
    stacked = pm.collect_pocket_envs(name)[0] if s.stacked else -1
    for run in ref["runs"]:
        for b in range(s.B):
            n = int(run["lengths"][b])
            if b != stacked:
                assert not run["batch"]["state"][b, :n + 1, 0].any(), (name, b)


# ------------------------------------------------------------------ 4, 5: the descent branches
@pytest.mark.parametrize("name", list(pm.ROLLOUT))
def test_rollout_case_takes_every_descent_branch(name, record_property):
    """Ties among the best neighbours, an unavailable neighbour that would have been best, an
    explore draw and a greedy stay (N = 1 included: its placements do produce ties)."""
    s = pm.ROLLOUT[name]
    counts = pm.run(name, "descent", pm.EPS, s.phase)["counts"]
    record_property("descent_branch_counts", counts)
    print("%s descent (eps 2^30, %s): %s" % (name, s.phase, counts))
    assert all(v > 0 for v in counts.values()), (name, counts)


@pytest.mark.parametrize("name", list(pm.COLLECT))
def test_collect_case_takes_every_descent_branch(name, record_property):
    counts = pm.collect_reference(name, "descent", pm.EPS)["counts"]
    record_property("descent_branch_counts", counts)
    print("%s descent collect (eps 2^30, two runs): %s" % (name, counts))
    assert all(v > 0 for v in counts.values()), (name, counts)


# ------------------------------------------------------------------ the extra eps, the ends
def test_eps_0_and_2_32_run_once_per_kernel_family():
    for runs, fast in ((pm.EXTRA_ROLLOUT, lambda n: n.startswith("f-")), (pm.EXTRA_COLLECT, lambda n: n.startswith("cf-"))):
        for eps_q in (0, 2 ** 32):
            names = [r[0] for r in runs if r[1] == eps_q]
            assert any(fast(n) for n in names) and any(not fast(n) for n in names)
    for name, eps_q, phase in pm.EXTRA_ROLLOUT:
        for rule in pm.RULES:
            acts = pm.run(name, rule, eps_q, phase)["actions"]
            assert (acts != 4).any()


@pytest.mark.parametrize("rule", pm.RULES)
@pytest.mark.parametrize("name,eps_q", pm.COLLECT_RUNS)
def test_collect_runs_still_end_early(name, eps_q, rule):
    """runner_collect_cases' scheme holds with the pocket in the field's place: envs end at
    several steps below the limit, one runs to the limit, the stale list is exercised -- in
    both runs (collect_unmet: the descent's and the pibt tests' own conditions)."""
    s = pm.COLLECT[name]
    ref = pm.collect_reference(name, rule, eps_q)
    assert pm.collect_unmet(name, rule, ref) == []
    assert ref["runs"][0]["pseed"] != ref["runs"][1]["pseed"]
    grid = pm.runner_ref.parse_map(ref["grid"])
    assert grid.shape == (s.H, s.W) and grid[-1, -1] == 0 and grid[0, 0] == 0
    for run in ref["runs"]:
        for b in range(s.B):
            st = run["starts"][b]
            assert (grid[st[:, 0], st[:, 1]] == 0).all()
            if pm.collect_kind(name, b) == "never":
                assert run["lengths"][b] == pm.COLLECT_LIMIT
