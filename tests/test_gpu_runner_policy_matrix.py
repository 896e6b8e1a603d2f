"""ParallelRunner.collect in policy mode over every kernel instance that can run it -- the 20
partial_runner_rollout_kernel instances of the descent and the 20
partial_pibt_runner_rollout_kernel instances of the collision-free rule (csrc/partial.hip
pick_run_roll) -- byte for byte against the restated reference loop whose MAC is the rule
(tests/partial_policy_matrix.py collect_reference).  The envs that are not part of the
termination scheme play in a crowded pocket: tests/test_partial_policy_matrix.py holds the
branches they take.  The runner, snapshot and comparison helpers are
tests/test_gpu_runner_collect.py's.
"""
import numpy as np
import pytest

import partial_policy_matrix as pm
import test_gpu_runner_collect as rc
from test_gpu_runner_shapes import FILL

pytestmark = pytest.mark.gpu

EPS_IDS = {0: "eps0", 2 ** 30: "eps2^30", 2 ** 32: "eps2^32"}


def _kernel(printed, rule):
    return pm.pc.kernel_args(printed, pm.COLLECT_KERNEL[rule])


@pytest.mark.parametrize("rule", pm.RULES)
@pytest.mark.parametrize("name,eps_q", pm.COLLECT_RUNS, ids=["%s-%s" % (n, EPS_IDS[e]) for n, e in pm.COLLECT_RUNS])
def test_collect_instance_matches_reference_loop(tmp_path, name, eps_q, rule):
    """collect(eps, policy), two runs: the instance, the batch, the returns, lengths, t_env and
    the logged stats of the reference loop whose MAC is the rule."""
    from mapfx import _abi
    ref = pm.collect_reference(name, rule, eps_q)
    assert pm.collect_unmet(name, rule, ref) == []
    runner, logger = rc._runner(tmp_path, pm.collect_case(name), ref["grid"], ref["runs"], seed=ref["seed"])
    for r, run in enumerate(ref["runs"]):
        batch = runner.collect(eps=eps_q / 2.0 ** 32, policy=rule)
        kern = _abi.last_kernel()
        assert _kernel(kern, rule) == pm.expected_collect_kernel(pm.collect_shape(name), True, rule), kern
        rc._assert_batch(batch, run["batch"], (name, rule, eps_q, r))
        rc._assert_totals(runner, run, r)
    assert logger.stats == ref["log"]


@pytest.mark.parametrize("rule", pm.RULES)
@pytest.mark.parametrize("name", pm.COLLECT_NO_ROWS)
def test_collect_instance_without_the_rows(tmp_path, name, rule):
    """rows->obs NULL (the call of test_gpu_runner_collect.py's test_rows_without_obs): the
    instance without the rows; every other field as with them, the obs rows untouched."""
    from mapfx import _abi
    eps_q = pm.EPS
    ref = pm.collect_reference(name, rule, eps_q)
    run = ref["runs"][0]
    runner, _ = rc._runner(tmp_path, pm.collect_case(name), ref["grid"], ref["runs"], seed=ref["seed"])
    runner.env.set_policy_rule(rule)
    runner.reset()
    obs0 = runner.batch["obs"].cpu().numpy().copy()
    rows = type(runner._erows).from_buffer_copy(runner._erows)
    rows.obs = None
    assert rc._rollout(runner, 0, pm.COLLECT_LIMIT + 1, pol=(run["pseed"], eps_q, 0), rows=rows) == 0
    kern = _abi.last_kernel()
    assert _kernel(kern, rule) == pm.expected_collect_kernel(pm.collect_shape(name), False, rule), kern
    rc._assert_batch(runner.batch, run["batch"], (name, rule), skip=("obs",))
    got = runner.batch["obs"].cpu().numpy()
    assert np.array_equal(got.view(np.uint8), obs0.view(np.uint8))       # row 0 from reset, the rest fill
    assert (got[:, 1:].view(np.uint8) == FILL).all()
    assert np.array_equal(runner._ep_length.cpu().numpy(), run["lengths"])
    runner.env.check_err()
