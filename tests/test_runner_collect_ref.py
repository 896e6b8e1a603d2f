"""What tests/test_gpu_runner_collect.py expects of ParallelRunner.collect, from the
restatement alone (tests/runner_ref.py with the restated policy as its MAC,
tests/runner_collect_cases.py) -- no GPU: every case has the terminations the device
comparison needs, the uniform limit of the MAC is gen_actions, and the per-run policy seed is
a stable pure function.
"""
import numpy as np
import pytest

import runner_collect_cases as cc
from test_gpu_runner_shapes import CASES, FILL


def _filled_rows(case, run):
    """The rows say what the lengths say: filled 0..n, terminated at n - 1, nothing after."""
    unwritten = int(np.full(8, FILL, np.uint8).view(np.int64)[0])
    for b, n in enumerate(run["lengths"]):
        assert run["batch"]["terminated"][b, n - 1, 0] == 1
        assert run["batch"]["filled"][b, :, 0].tolist() == [1] * (n + 1) + [unwritten] * (case["limit"] - n)


@pytest.mark.parametrize("eps_q", cc.EPS_QS)
@pytest.mark.parametrize("name", cc.POLICY_CASES)
def test_policy_cases_have_the_terminations(name, eps_q):
    """Per run: >= 3 distinct termination steps before the limit, an env that runs to the
    limit, two envs of one wave's group ending at different steps, a stale actions row."""
    case, ref = CASES[name], cc.policy_reference(name, eps_q)
    assert cc.unmet(case, ref) == []
    for run in ref["runs"]:
        _filled_rows(case, run)
        # the stale list: the MAC call after an env's last step still has it in bs, with the
        # action its resting state gives -- recorded in the actions row at that step
        assert len(run["calls"]) == run["lengths"].max() + 1
        for t, bs, a, done in run["macs"]:
            for j, b in enumerate(bs):
                assert done[j] == (run["lengths"][b] == t)
                assert np.array_equal(run["batch"]["actions"][b, t, :, 0], a[j])
    assert ref["runs"][0]["pseed"] != ref["runs"][1]["pseed"]


@pytest.mark.parametrize("name", cc.POLICY_CASES)
def test_uniform_limit_of_the_mac_is_gen_actions(name):
    """At eps_q = 2^32 every action of the MAC is mapfx_action's (rng.gen_actions)."""
    from mapfx import rng
    ref = cc.policy_reference(name, 2 ** 32)
    for run in ref["runs"]:
        for t, bs, a, _ in run["macs"]:
            assert np.array_equal(a, rng.gen_actions(run["pseed"], bs, [t], CASES[name]["N"])[0])


@pytest.mark.parametrize("name", cc.POLICY_CASES)
def test_policy_maps_hold_their_agents(name):
    """The built maps: a pen has no free neighbour, the corridor is closed, the field is large
    enough for N starts; early envs end after exactly d steps of pure descent."""
    case = CASES[name]
    grid = cc.runner_ref.parse_map(cc.policy_grid(case))
    assert grid.shape == (len(case["grid"]), len(case["grid"][0]))
    nr = cc.pen_rows(case)
    pad = np.pad(grid, 1, constant_values=-1)
    for r in range(0, 2 * nr, 2):
        for c in range(0, grid.shape[1], 2):
            assert grid[r, c] == 0
            assert [pad[r, c + 1], pad[r + 2, c + 1], pad[r + 1, c], pad[r + 1, c + 2]] == [-1] * 4
    assert grid[2 * nr, :5].tolist() == [0] * 5 and (grid[2 * nr, 5:] == -1).all()
    assert (grid[2 * nr + 1] == -1).all() and (2 * nr == 0 or (grid[2 * nr - 1] == -1).all())
    assert (grid[2 * nr + 2:] == 0).sum() >= case["N"]
    ref = cc.policy_reference(name, 0)
    for run in ref["runs"]:
        for b in range(case["B"]):
            kd = cc.kind(case, b)
            if kd == "never":
                assert run["lengths"][b] == case["limit"]
            elif kd != "field":
                assert run["lengths"][b] == kd[1]


@pytest.mark.parametrize("name", cc.GIVEN_CASES)
def test_given_cases_have_the_terminations(name):
    case, ref = CASES[name], cc.given_reference(name)
    assert cc.unmet(case, ref) == []
    for run in ref["runs"]:
        _filled_rows(case, run)
        assert (run["lengths"] == 1).any()         # an env that ends at step 0


def test_runner_policy_seed_is_a_stable_pure_function():
    from mapfx import rng
    assert rng.runner_policy_seed(5, 0) == 7134611160154358618
    assert rng.runner_policy_seed(5, 1) == 11764459695210290591
    seeds = {rng.runner_policy_seed(s, r) for s in range(4) for r in range(50)}
    assert len(seeds) == 200
    for s, r in ((0, 0), (7, 3), (2 ** 63 + 5, 2 ** 31)):
        want = int(rng.splitmix64(np.uint64(s) ^ rng._mul(np.uint64(r), rng.K_T)))
        assert rng.runner_policy_seed(s, r) == want == rng.runner_policy_seed(s, r)
