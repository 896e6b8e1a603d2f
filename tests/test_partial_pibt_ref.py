"""mapfx.rng.partial_policy_pibt_actions -- the definition of the collision-free on-device
policy (MAPFX_POLICY_PIBT, include/mapfx_partial.h) -- on the CPU: the rule on hand-written
instances, and, closed loop on the MARL_PARTIAL restatement, what the episodes that
tests/test_gpu_partial_pibt.py expects of the device show: no collision where descent
collides, every branch of the rule taken, envs that complete.
"""
import numpy as np
import pytest

import partial_pibt_cases as pc
from oracle.partial_oracle import PartialEnvState

UP, DOWN, LEFT, RIGHT, STAY = 0, 1, 2, 3, 4


def _env(rows, starts, goals):
    grid = np.array([[-1 if ch == "@" else 0 for ch in r] for r in rows], np.int64)
    return PartialEnvState(grid, starts, goals)


def _act(env, t=0, eps_q=0, seed=1):
    """(actions, branch counts by name) of one env (global id 0) at counter t."""
    from mapfx import rng
    stats = np.zeros(len(rng.PIBT_STATS), np.int64)
    a = pc.rule_actions("pibt", seed, np.array([0]), t, eps_q, [env], stats)
    assert a.dtype == np.int8 and a.shape == (1, env.n)
    return a[0].tolist(), dict(zip(rng.PIBT_STATS, stats.tolist()))


def _draws(seed, t, n):
    from mapfx import rng
    return [int(rng.gen_actions(seed, [0], [t], n)[0, 0, a]) for a in range(n)]


def _seed_with(t, want):
    """A seed whose draws u % 5 of agents 0.. at counter t satisfy the predicates `want`."""
    for seed in range(1, 4000):
        if all(w(d) for w, d in zip(want, _draws(seed, t, len(want)))):
            return seed
    raise AssertionError("no seed found")


def test_head_on_pair_in_a_corridor_never_swaps():
    # agent 1 has room behind it: it backs off before agent 0
    acts, st = _act(_env(["....."], [(0, 1), (0, 2)], [(0, 4), (0, 0)]))
    assert acts == [RIGHT, RIGHT] and st["skip_parent"] == 1 and st["push"] == 1 and st["push_failed"] == 0
    # agent 1 against the wall: its list runs out, agent 0 falls back to stay
    acts, st = _act(_env(["....."], [(0, 3), (0, 4)], [(0, 4), (0, 0)]))
    assert acts == [STAY, STAY] and st["push_failed"] == 1 and st["forced_stay"] == 1


def test_cycles_on_a_2x2_block_are_allowed():
    # a pair that wants to swap: the pushed agent goes round the block instead
    acts, _ = _act(_env(["..", ".."], [(0, 0), (0, 1)], [(0, 1), (0, 0)]))
    assert acts == [RIGHT, DOWN]
    # four agents rotate: the last of the chain takes the cell the first one leaves
    acts, st = _act(_env(["..", ".."], [(0, 0), (0, 1), (1, 1), (1, 0)], [(0, 1), (1, 1), (1, 0), (0, 0)]))
    assert acts == [RIGHT, DOWN, LEFT, UP] and st["push"] == 3 and st["depth3"] == 2


def test_an_agent_resting_on_its_goal_is_pushed_off():
    acts, st = _act(_env(["...", "..."], [(0, 0), (0, 1)], [(0, 2), (0, 1)]))
    assert acts == [RIGHT, DOWN] and st["skip_claimed"] == 1      # (its stay comes first, and is claimed)


def test_a_three_deep_chain_succeeds():
    acts, st = _act(_env(["....."], [(0, 0), (0, 1), (0, 2)], [(0, 4), (0, 1), (0, 2)]))
    assert acts == [RIGHT, RIGHT, RIGHT] and st["push"] == 2 and st["depth3"] == 1 and st["push_failed"] == 0


def test_a_failed_chain_backtracks_to_the_second_candidate():
    # up and right tie for agent 0 (up first).  Up: agent 1 rests there and is pushed; its
    # way up is agent 2 in the corner, pushed in turn, whose only other cell holds two agents;
    # agent 1's way right holds two agents too.  Both return false, agent 0 goes right.
    starts = [(2, 0), (1, 0), (0, 0), (0, 1), (0, 1), (1, 1), (1, 1)]
    acts, st = _act(_env(["...", "...", "..."], starts, [(0, 2)] + starts[1:]))
    assert acts == [RIGHT, STAY, STAY, STAY, RIGHT, STAY, RIGHT]
    assert st["push_failed"] == 2 and st["depth3"] == 1 and st["skip_multi"] == 3 and st["forced_stay"] == 2
    # the same with a wall instead: the second candidate is stay
    acts, st = _act(_env(["...", ".@."], [(0, 0), (1, 0)], [(1, 0), (1, 0)]))
    assert acts == [STAY, STAY] and st["push_failed"] == 1 and st["forced_stay"] == 1
    # a chain of three that fails at its end: everybody stays
    acts, st = _act(_env(["..."], [(0, 0), (0, 1), (0, 2)], [(0, 2), (0, 1), (0, 2)]))
    assert acts == [STAY, STAY, STAY] and st["push_failed"] == 2 and st["depth3"] == 1


def test_a_cell_with_two_undecided_occupants_is_skipped():
    acts, st = _act(_env(["..."], [(0, 0), (0, 1), (0, 1)], [(0, 2), (0, 1), (0, 1)]))
    assert acts[0] == STAY and st["skip_multi"] == 1 and st["push"] == 0


def test_stacked_starts():
    acts, _ = _act(_env(["..."], [(0, 1), (0, 1)], [(0, 0), (0, 2)]))
    assert acts == [LEFT, RIGHT]
    # both want to stay: the first keeps the cell, the second finds it claimed and leaves
    acts, st = _act(_env(["..."], [(0, 1), (0, 1)], [(0, 1), (0, 1)]))
    assert acts == [STAY, LEFT] and st["skip_claimed"] == 1
    # nowhere to go: the second stays on the claimed cell (the one node collision the rule allows)
    acts, st = _act(_env(["."], [(0, 0), (0, 0)], [(0, 0), (0, 0)]))
    assert acts == [STAY, STAY] and st["forced_stay"] == 1


def test_an_unreachable_goal_stays_even_when_exploring():
    env = _env([".@."], [(0, 0)], [(0, 2)])
    assert _act(env)[0] == [STAY]
    acts, st = _act(env, eps_q=2 ** 32)
    assert acts == [STAY] and st["explore_top"] == 0


def test_an_unavailable_explore_draw_becomes_stay():
    seed = _seed_with(0, [lambda d: d == UP])
    acts, st = _act(_env(["..", ".."], [(0, 0)], [(1, 1)]), eps_q=2 ** 32, seed=seed)
    assert acts == [STAY] and st["explore_top"] == 1
    assert _act(_env(["..", ".."], [(0, 0)], [(1, 1)]), eps_q=0, seed=seed)[0] == [DOWN]


def test_eps_2_32_is_not_mapfx_action():
    """The draw is taken when it is available and free -- and only then."""
    seed = _seed_with(0, [lambda d: d == RIGHT, lambda d: d == LEFT])
    env = _env(["...."], [(0, 0), (0, 3)], [(0, 0), (0, 3)])
    assert _act(env, eps_q=2 ** 32, seed=seed)[0] == [RIGHT, LEFT] == _draws(seed, 0, 2)
    env = _env(["..."], [(0, 0), (0, 2)], [(0, 0), (0, 2)])        # both draw the middle cell
    assert _act(env, eps_q=2 ** 32, seed=seed)[0] == [RIGHT, STAY]


def test_a_pushed_agent_uses_its_sorted_list_even_when_it_explores():
    seed = _seed_with(0, [lambda d: d == RIGHT, lambda d: d != RIGHT])
    acts, st = _act(_env(["...."], [(0, 0), (0, 1)], [(0, 2), (0, 3)]), eps_q=2 ** 32, seed=seed)
    assert acts == [RIGHT, RIGHT] and st["explore_top"] == 1 and st["explore_pushed"] == 1


def test_the_index_priority_rotates_with_t():
    env = _env(["..."], [(0, 0), (0, 2)], [(0, 2), (0, 0)])        # both want the middle cell
    assert _act(env, t=0)[0] == [RIGHT, STAY]
    assert _act(env, t=1)[0] == [STAY, LEFT]
    assert _act(env, t=2 ** 32)[0] == [RIGHT, STAY]               # t is an unsigned 32-bit value
    assert _act(env, t=-1)[0] == [STAY, LEFT]                      # ... 2^32 - 1 is odd
    # an agent on its goal is planned after the others, whatever the rotation says
    env = _env(["..."], [(0, 1), (0, 0)], [(0, 1), (0, 2)])
    for t in (0, 1):
        acts, st = _act(env, t=t)
        assert acts == [RIGHT, RIGHT] and st["push"] == 1


# ------------------------------------------------------------------ closed loop
@pytest.mark.parametrize("name", pc.CASES)
def test_no_collision_where_descent_collides(name):
    """Fresh episodes of every GPU case: under the rule no env without a stacked start ever
    shows a node or edge flag (total_coll 0 at the end); under descent at eps 0 the same
    instances collide."""
    assert pc.stacked_envs(name) == ([5] if name == "dense-6x6-n15" else [])     # the one stacked start
    clean = [e for e in range(pc.case_of(name).E) if e not in pc.stacked_envs(name)]
    for eps_q in pc.EPS:
        r = pc.run(name, eps_q, "fresh")
        assert r["actions"].min() >= 0 and r["actions"].max() <= 4
        for k, s in enumerate(r["snaps"]):
            assert not s["node"][clean].any() and not s["edge"][clean].any(), (eps_q, k)
        assert not r["snaps"][-1]["total_coll"][clean].any()
    d = pc.run(name, 0, "fresh", "descent")
    assert (d["snaps"][-1]["total_coll"] > 0).any()


def test_gpu_episodes_take_every_branch_and_some_complete(record_property):
    """Summed over the episodes the GPU tests expect, every branch counter of the rule is
    positive, and envs complete (every agent on its goal).  The completed share of the
    eps 0 fresh episodes is recorded, not asserted."""
    from mapfx import rng
    total = np.zeros(len(rng.PIBT_STATS), np.int64)
    done = n = 0
    for name in pc.CASES:
        for eps_q in pc.EPS:
            for phase in pc.PHASES:
                r = pc.run(name, eps_q, phase)
                total += r["stats"]
                if eps_q == 0 and phase == "fresh":
                    done += int(r["completed"].sum())
                    n += len(r["completed"])
    counts = dict(zip(rng.PIBT_STATS, total.tolist()))
    assert all(v > 0 for v in counts.values()), counts
    assert done > 0
    assert pc.run("dense-3x7-n5", 0, "fresh")["completed"].any()
    record_property("pibt_branch_counts", counts)
    record_property("pibt_completed_share_eps0", "%d / %d" % (done, n))
    print("pibt: branch counts %s; completed at eps 0: %d of %d envs" % (counts, done, n))


def test_the_deep_chains_are_in_the_64_agent_case():
    from mapfx import rng
    st = dict(zip(rng.PIBT_STATS, pc.run("dense-9x9-n64", 0, "fresh")["stats"].tolist()))
    assert st["depth3"] > 0 and st["push_failed"] > 0 and st["skip_multi"] == 0


def test_runner_reference_episodes_end_at_several_steps():
    """The collect() cases: under the rule envs still end early at distinct steps and one
    runs to the limit (what makes the stale rows and the waves that leave the loop)."""
    for name in pc.RUNNER_CASES_PIBT:
        for eps_q in pc.RUNNER_EPS:
            ref = pc.runner_reference(name, eps_q)
            limit = pc.RUNNER_CASES[name]["limit"]
            for run in ref["runs"]:
                lengths = run["lengths"]
                assert len(set(lengths[lengths < limit].tolist())) >= 2, (name, eps_q, lengths.tolist())
                assert (lengths == limit).any()
