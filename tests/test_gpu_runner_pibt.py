"""ParallelRunner.collect(policy="pibt") / mapfx_runner_rollout under MAPFX_POLICY_PIBT -- the
partial_pibt_runner_rollout_kernel instances of csrc/partial.hip -- byte for byte against the
restated reference loop with the rule's definition as its MAC (tests/partial_pibt_cases.py
runner_reference) and against the step form on a second handle fed the rule's actions.
The runner, snapshot and comparison helpers are tests/test_gpu_runner_collect.py's.
"""
import numpy as np
import pytest

import partial_pibt_cases as pc
import test_gpu_runner_collect as rc
from test_gpu_runner_shapes import CASES, FILL

pytestmark = pytest.mark.gpu


def _kernel(printed):
    return pc.kernel_args(printed, "partial_pibt_runner_rollout_kernel")


def _want_kernel(name, obs=True):
    return ("partial_pibt_runner_rollout_kernel", rc._want_kernel(name, obs)[1])


@pytest.mark.parametrize("eps_q", pc.RUNNER_EPS, ids=["eps0", "eps2^31"])
@pytest.mark.parametrize("name", pc.RUNNER_CASES_PIBT)
def test_collect_pibt_matches_reference_loop(tmp_path, name, eps_q):
    """collect(eps, policy="pibt"), two runs: the batch, the returns, lengths, t_env and the
    logged stats of the reference loop whose MAC is the rule."""
    from mapfx import _abi
    ref = pc.runner_reference(name, eps_q)
    runner, logger = rc._runner(tmp_path, name, ref["grid"], ref["runs"], seed=ref["seed"])
    for r, run in enumerate(ref["runs"]):
        batch = runner.collect(eps=eps_q / 2.0 ** 32, policy="pibt")
        assert _kernel(_abi.last_kernel()) == _want_kernel(name), _abi.last_kernel()
        rc._assert_batch(batch, run["batch"], (name, eps_q, r))
        rc._assert_totals(runner, run, r)
    assert logger.stats == ref["log"]


def test_collect_alternates_rules_and_defaults_to_descent(tmp_path):
    """Run 0 under pibt, run 1 without the argument: descent, on the descent instance, the
    episode runner_collect_cases expects of run 1."""
    from mapfx import _abi
    import runner_collect_cases as cc
    name, eps_q = "fast8_n5", 2 ** 31
    want = cc.policy_reference(name, eps_q)
    ref = pc.runner_reference(name, eps_q, seed=want["seed"])
    runner, _ = rc._runner(tmp_path, name, ref["grid"], ref["runs"], seed=ref["seed"])
    batch = runner.collect(eps=0.5, policy="pibt")
    rc._assert_batch(batch, ref["runs"][0]["batch"], "pibt run")
    batch = runner.collect(eps=0.5)
    assert rc._kernel(_abi.last_kernel()) == rc._want_kernel(name), _abi.last_kernel()
    rc._assert_batch(batch, want["runs"][1]["batch"], "descent run")
    with pytest.raises(ValueError, match="policy must be"):
        runner.collect(policy="astar")


@pytest.mark.parametrize("name", ["fast8_n5", "fast16_n16", "gen_n3"])
def test_rollout_equals_the_step_form(tmp_path, name):
    """One call of T = max_t, and T = 3 continued by steps, against mapfx_runner_step calls on
    a second handle fed the rule's recorded actions (those of env bs[j] as it stands, stale
    envs included): the rows, the runner state and the env state."""
    import torch
    eps_q = 2 ** 31
    ref = pc.runner_reference(name, eps_q)
    max_t = CASES[name]["limit"] + 1
    one, _ = rc._runner(tmp_path, name, ref["grid"], ref["runs"], seed=ref["seed"], tag="a")
    two, _ = rc._runner(tmp_path, name, ref["grid"], ref["runs"], seed=ref["seed"], tag="b")
    one.env.set_policy_rule("pibt")
    for split, run in zip((max_t, 3), ref["runs"]):
        table = torch.as_tensor(run["table"], device="cuda")
        one.reset()
        two.reset()
        assert rc._rollout(one, 0, split, pol=(run["pseed"], eps_q, 0)) == 0
        rc._steps(two, 0, split, table)
        rc._assert_same(rc._snapshot(one, one.batch), rc._snapshot(two, two.batch), (name, "after", split))
        if split == max_t:
            rc._assert_batch(one.batch, run["batch"], (name, "one call"))
        else:
            rc._steps(one, split, max_t - split, table)
            rc._steps(two, split, max_t - split, table)
            rc._assert_same(rc._snapshot(one, one.batch), rc._snapshot(two, two.batch), (name, "continued"))
            rc._assert_batch(one.batch, run["batch"], (name, "continued"))


@pytest.mark.parametrize("chunk", [1, 2, (1, 4, 1)])
def test_chunked_calls_equal_one_call(tmp_path, chunk):
    name, eps_q = "fast16_n16", 2 ** 31
    ref = pc.runner_reference(name, eps_q)
    one, _ = rc._runner(tmp_path, name, ref["grid"], ref["runs"], seed=ref["seed"], tag="a")
    two, _ = rc._runner(tmp_path, name, ref["grid"], ref["runs"], seed=ref["seed"], tag="b")
    b1, b2 = one.collect(eps=0.5, policy="pibt"), two.collect(eps=0.5, policy="pibt", chunk=chunk)
    rc._assert_same(rc._snapshot(one, b1), rc._snapshot(two, b2), ("pibt", chunk))
    rc._assert_batch(b2, ref["runs"][0]["batch"], ("pibt", chunk))


def test_rows_without_obs(tmp_path):
    """rows->obs NULL under the rule: the instance without the rows; every other field as
    with them, the obs rows untouched."""
    from mapfx import _abi
    name, eps_q = "fast8_n5", 2 ** 31
    ref = pc.runner_reference(name, eps_q)
    run = ref["runs"][0]
    runner, _ = rc._runner(tmp_path, name, ref["grid"], ref["runs"], seed=ref["seed"])
    runner.env.set_policy_rule("pibt")
    runner.reset()
    obs0 = runner.batch["obs"].cpu().numpy().copy()
    rows = type(runner._erows).from_buffer_copy(runner._erows)
    rows.obs = None
    assert rc._rollout(runner, 0, 6, pol=(run["pseed"], eps_q, 0), rows=rows) == 0
    assert _kernel(_abi.last_kernel()) == _want_kernel(name, obs=False), _abi.last_kernel()
    rc._assert_batch(runner.batch, run["batch"], name, skip=("obs",))
    got = runner.batch["obs"].cpu().numpy()
    assert np.array_equal(got.view(np.uint8), obs0.view(np.uint8))
    assert (got[:, 1:].view(np.uint8) == FILL).all()
    assert np.array_equal(runner._ep_length.cpu().numpy(), run["lengths"])


def test_collect_pibt_is_refused_where_it_is_not_offered(tmp_path):
    """block200_n9 (int32 goal tables): the rule is not offered; collect raises before a reset."""
    import runner_collect_cases as cc
    name = "block200_n9"
    ref = cc.given_reference(name)
    runner, _ = rc._runner(tmp_path, name, ref["grid"], ref["runs"])
    t_env = runner.t_env
    with pytest.raises(ValueError, match="not offered"):
        runner.collect(eps=0.0, policy="pibt")
    assert runner.t_env == t_env
