"""tests/runner_ref.py (the restatement of the reference ParallelRunner loop that the
GPU runner's kernel-instance matrix is compared with) pinned on the CPU: it must
reproduce every field of every run of tests/golden/runner_*.npz -- written by the
reference runner itself -- byte for byte, with t_env and the three log arrays."""
import numpy as np
import pytest

import runner_ref
from conftest import load_fixture

REWARDS = dict(move_reward=0, stay_reward=-0.1, stay_goal_reward=1, node_collide_reward=-2000,
               edge_collide_reward=-2000, env_collide_reward=-2000, complete_reward=1000,
               complete_fac=1.5, gamma=0.99)
CASES = ["runner_open5_n2", "runner_wall6_n3", "runner_solo4_n1", "runner_fast8_n6",
         "runner_fast16_n12"]


def scripted_action(b, t, n, avail_row):
    """= gen_runner_fixtures.scripted_action"""
    a = (3 * b + 7 * t + 5 * n + (b * t) % 3) % 5
    return a if avail_row[a] else 4


def scripted_mac(batch, t_ep, bs):
    av = batch["avail_actions"][:, t_ep]
    return [[scripted_action(b, t_ep, n, av[b, n]) for n in range(av.shape[1])] for b in bs]


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference_runner(name):
    fx = load_fixture(name)
    B, N, limit = int(fx["B"]), int(fx["n_agents"]), int(fx["limit"])
    W, K = int(fx["obs_window"]), int(fx["obs_knn_agents"])
    grid = runner_ref.parse_map(fx["map"])
    ref = runner_ref.RefRunner(runner_log_interval=1)
    for r in range(int(fx["runs"])):
        i = r % fx["inst_starts"].shape[0]
        envs = runner_ref.make_envs(grid, np.repeat(fx["inst_starts"][i][None], B, 0),
                                    np.repeat(fx["inst_goals"][i][None], B, 0), obs_window=W,
                                    obs_knn_agents=K, episode_limit=limit, **REWARDS)
        batch = runner_ref.new_batch(B, limit + 1, N, 2 * W * W + 13 * K)
        batch, calls, _, _ = ref.run(envs, batch, scripted_mac)
        keys = sorted(k[len("run%d_" % r):] for k in fx if k.startswith("run%d_" % r))
        assert keys == sorted(list(batch) + ["t_env"])
        for k, got in batch.items():
            want = fx["run%d_%s" % (r, k)]
            assert got.shape == want.shape and got.dtype == want.dtype, (r, k)
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (r, k)
        assert ref.t_env == int(fx["run%d_t_env" % r])
        assert calls[0] == (0, tuple(range(B))) and [t for t, _ in calls] == list(range(len(calls)))
    assert [k for k, _, _ in ref.log] == fx["log_stats"].tolist()
    assert np.array_equal(np.array([v for _, v, _ in ref.log], np.float64).view(np.uint64),
                          fx["log_values"].view(np.uint64))
    assert [t for _, _, t in ref.log] == fx["log_t"].tolist()
