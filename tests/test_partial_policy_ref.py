"""mapfx.rng.partial_policy_actions -- the numpy restatement of mapfx_partial_rollout's
on-device policy (include/mapfx_partial.h) -- on the CPU: its uniform limit against
mapfx_action / gen_actions, the descent rule on hand-written inputs, a closed-loop episode
of the MARL_PARTIAL restatement, and that the episodes tests/test_gpu_partial_rollout.py
expects of the device take every branch of the rule.
"""
import numpy as np

from partial_rollout_cases import (POLICY_CASES, POLICY_EPS, POLICY_PHASES, policy_episode, policy_run)
from partial_step_cases import BY_NAME, build, make_refs


def _one(avail, pd, d, eps_q=0, seed=1, env=0, t=0):
    from mapfx import rng
    return int(rng.partial_policy_actions(seed, [env], t, eps_q, np.array([[avail]]), np.array([[pd]]),
                                          np.array([[d]]))[0, 0])


def test_eps_2_32_is_mapfx_action():
    from mapfx import lib, rng
    seed, N = 0x1234ABCD5678, 7
    envs = [0, 1, 7, 4095, 123456789]
    junk = np.random.default_rng(0)
    for t in (0, 1, 99, 2 ** 31 - 1):
        avail = junk.integers(16, 32, size=(len(envs), N))
        pd = junk.integers(-1, 9, size=(len(envs), N))
        d = junk.integers(-1, 9, size=(len(envs), N, 4))
        got = rng.partial_policy_actions(seed, envs, t, 2 ** 32, avail, pd, d)
        assert got.dtype == np.int8
        assert np.array_equal(got, rng.gen_actions(seed, envs, [t], N)[0])
        for ei, e in enumerate(envs):
            for a in range(N):
                assert lib.mapfx_action(seed, e, t, a) == got[ei, a]


def test_descent_rule_by_hand():
    assert _one(0b11111, 5, [4, 6, 4, 6]) == 0          # a tie between up and left: the lower index
    assert _one(0b11111, 5, [6, 4, 6, 4]) == 1          # ... between down and right
    assert _one(0b11110, 5, [3, 6, 4, 6]) == 2          # the best (up) is unavailable: passed over
    assert _one(0b10000, 5, [3, 3, 3, 3]) == 4          # nothing available
    assert _one(0b11111, 5, [5, 6, 5, 7]) == 4          # no improving neighbour: stay
    assert _one(0b11111, 0, [1, 1, 1, 1]) == 4          # on the goal
    assert _one(0b11111, -1, [0, 1, 2, 3]) == 4         # pd < 0 stays
    # an obstacle with an agent standing on it: avail bit set, d = -1 -- not taken
    assert _one(0b11111, 5, [-1, 4, 6, 6]) == 1
    assert _one(0b11111, 5, [-1, -1, -1, -1]) == 4
    assert _one(0b11111, 5, [6, 6, 6, 4]) == 3


def test_explore_threshold_is_the_high_word():
    from mapfx import rng
    seed, envs, N, t = 99, np.arange(40), 5, 3
    u = rng.splitmix64(np.uint64(seed) ^ rng._mul(envs.astype(np.uint64)[:, None], rng.K_ENV)
                       ^ rng._mul(np.uint64(t), rng.K_T) ^ rng._mul(np.arange(N, dtype=np.uint64)[None], rng.K_AGENT))
    hi = (u >> np.uint64(32)).astype(np.int64)
    eps_q = int(np.median(hi))
    pd = np.full((40, N), 5)
    d = np.tile(np.array([6, 6, 6, 4]), (40, N, 1))
    got = rng.partial_policy_actions(seed, envs, t, eps_q, np.full((40, N), 31), pd, d)
    want = np.where(hi < eps_q, (u % np.uint64(5)).astype(np.int64), 3)
    assert (hi < eps_q).any() and not (hi < eps_q).all()
    assert np.array_equal(got, want)


def test_closed_loop_single_agent_walks_its_shortest_path():
    """gen-w1-n1 (one agent per env) under eps_q = 0: the env terminates -- its agent on the
    goal -- at t = the start's goal distance."""
    c = BY_NAME["gen-w1-n1"]
    b = build(c)
    envs = list(range(12))
    dist = [int(b["goal_dist"][e, 0][b["starts"][e, 0, 0] * c.W + b["starts"][e, 0, 1]]) for e in envs]
    assert min(dist) >= 1 and max(dist) > 2
    refs = [make_refs(c, b, limit=200)[e] for e in envs]
    done_at = {}
    for k in range(max(dist)):
        policy_episode(refs, 1, 0, 7, t0=k, env_ids=envs)
        for i, r in enumerate(refs):
            if r.terminated and i not in done_at:
                done_at[i] = r.t
    assert [done_at.get(i) for i in range(len(envs))] == dist


def test_gpu_policy_episodes_take_every_branch():
    """Over the episodes the GPU policy test expects (restatement alone): a tie among the
    best neighbours, an unavailable neighbour that would have been best (an off-grid one,
    fed as distance 0), an explore draw and a greedy stay each occur."""
    total = np.zeros(4, np.int64)
    for name in POLICY_CASES:
        for eps_q in POLICY_EPS:
            for phase in POLICY_PHASES:
                run = policy_run(name, eps_q, phase)
                total += run["counts"]
                acts = run["actions"]
                assert acts.shape == (run["T"], BY_NAME[name].E, BY_NAME[name].N)
                assert acts.min() >= 0 and acts.max() <= 4
    ties, passed, explore, stays = (int(v) for v in total)
    assert ties > 0 and passed > 0 and explore > 0 and stays > 0, total.tolist()
