"""MarlPartialBatch.rollout in policy mode over every kernel instance that can run it -- the 23
partial_rollout_kernel instances of the descent and the 23 partial_pibt_rollout_kernel instances
of the collision-free rule (csrc/partial.hip pick_roll) -- each on a crowded pocket map
(tests/partial_policy_matrix.py), bit for bit against the rule's definition stepped on the
restatement: the actions, every trajectory slot and every state array.
tests/test_partial_policy_matrix.py holds what the episodes cover: per case the failed pushes,
the three-deep chains and the other branches of the rule.
"""
import numpy as np
import pytest

import partial_policy_matrix as pm
from partial_rollout_cases import compare_slot
from partial_step_cases import compare, state_arrays

pytestmark = pytest.mark.gpu

EPS_IDS = {0: "eps0", 2 ** 30: "eps2^30", 2 ** 32: "eps2^32"}


@pytest.fixture(scope="module")
def mapfx_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mapfx
    return mapfx


def _np(t):
    return t.detach().cpu().numpy()


def _batch(mapfx_mod, name, envs=None, limit=pm.LIMIT, **kw):
    c, b = pm.case_of(name), pm.build_case(name)
    s = slice(None) if envs is None else envs
    grids = np.array(b["grids"]) if (c.shared or envs is None) else np.array(b["grids"])[s]
    return mapfx_mod.MarlPartialBatch(np.array(b["starts"])[s], np.array(b["goals"])[s], grids=grids,
                                      **dict(pm.params(name, limit), **kw))


def _dev(a, dtype):
    import torch
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


def _host_traj(traj):
    return {k: _np(v).copy() for k, v in traj.items()}


def _differ(a, b, keys=None):
    return [k for k in (keys or a) if not np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8),
                                                         np.ascontiguousarray(b[k]).view(np.uint8))]


def _kernel(printed, rule):
    return pm.pc.kernel_args(printed, pm.ROLLOUT_KERNEL[rule])


def _assert_episode(name, pb, traj, acts, snaps, obs=True):
    """The actions, every slot and the final state arrays against the restatement's episode."""
    got = _np(traj["actions"])
    bad = np.argwhere(got != acts)
    assert len(bad) == 0, "actions: first differing (step, env, agent) %s" % bad[:4].tolist()
    c, T = pm.case_of(name), len(snaps)
    for k in range(T):
        d = compare_slot(c, traj, k, snaps[k], obs=obs)
        assert d is None, d
    last = {f: traj[f][T - 1] for f in ("reward", "state", "avail")}
    last["obs"] = traj["obs"][T - 1] if obs else np.array(snaps[T - 1]["obs"])
    d = compare(pb, last, snaps[T - 1], "final state")
    assert d is None, d
    pb.check_err()


# ------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("rule", pm.RULES)
@pytest.mark.parametrize("name,eps_q,phase", pm.ROLLOUT_RUNS,
                         ids=["%s-%s-%s" % (n, EPS_IDS[e], p) for n, e, p in pm.ROLLOUT_RUNS])
def test_policy_instance_equals_the_restatement(mapfx_mod, name, eps_q, phase, rule):
    """One rollout(T, eps, seed, t0, obs, policy) with the rows and one without: the launched
    instance is the expected one, the episode is the restatement's."""
    import torch
    from mapfx import _abi
    c, b = pm.case_of(name), pm.build_case(name)
    run = pm.run(name, rule, eps_q, phase)
    for obs in (True, False):
        pb = _batch(mapfx_mod, name)
        pb.reset()
        if phase == "fresh":        # the carried distances become invalid: looked up
            pb.compute_goal_dist()
            assert int(pb.pdist.max().item()) == -2 ** 31
        for t in range(run["pre"]):
            pb.step(_dev(b["actions"][t], c.dtype))
        traj = pb.rollout(T=run["T"], eps=eps_q, seed=pm.SEED, t0=run["pre"], obs=obs, policy=rule)
        kern = _abi.last_kernel()
        torch.cuda.synchronize()
        assert _kernel(kern, rule) == pm.expected_kernel(name, obs, rule), kern
        assert ("obs" in traj) == obs
        _assert_episode(name, pb, traj, run["actions"], run["snaps"], obs=obs)


# ------------------------------------------------------------------ edges
@pytest.mark.parametrize("rule", pm.RULES)
@pytest.mark.parametrize("name", ["f-w3-l16-i16", "g-w3-n4"])
def test_autoreset_with_a_short_limit(mapfx_mod, name, rule):
    """Restarts inside the launch (int16 tables; the generic instance at lane group 4)."""
    limit, T, eps_q = 4, 12, 2 ** 30
    refs = pm.refs_of(name, limit)
    acts, snaps, _ = pm.rule_episode(rule, refs, T, eps_q, autoreset=True)
    assert max(int(s["t"].max()) for s in snaps) <= limit
    assert sum(int((s["t"] == 1).sum()) for s in snaps[1:]) >= 2 * len(refs), "too few restarts expected"
    pb = _batch(mapfx_mod, name, limit=limit)
    pb.reset()
    traj = pb.rollout(T=T, eps=eps_q, seed=pm.SEED, autoreset=True, policy=rule)
    _assert_episode(name, pb, traj, acts, snaps)


@pytest.mark.parametrize("rule", pm.RULES)
@pytest.mark.parametrize("name", ["f-w5-l8-i16", "f-w7-l16-u8"])
def test_two_calls_of_half_equal_one(mapfx_mod, name, rule):
    T, eps_q = pm.ROLLOUT[name].T, 2 ** 30
    one = _batch(mapfx_mod, name)
    one.reset()
    whole = _host_traj(one.rollout(T=T, eps=eps_q, seed=pm.SEED, policy=rule))
    two = _batch(mapfx_mod, name)
    two.reset()
    first = _host_traj(two.rollout(T=T // 2, eps=eps_q, seed=pm.SEED, policy=rule))
    second = _host_traj(two.rollout(T=T - T // 2, eps=eps_q, seed=pm.SEED, t0=T // 2, policy=rule))
    halves = {k: np.concatenate([first[k], second[k]]) for k in whole}
    assert _differ(halves, whole) == []
    assert _differ(state_arrays(two), state_arrays(one)) == []
    acts, _, _ = pm.rule_episode(rule, pm.refs_of(name), T, eps_q)
    assert np.array_equal(whole["actions"], acts)


def test_pibt_is_shard_invariant_with_int16_tables(mapfx_mod):
    name = "f-w5-l8-i16"            # per-env maps, 9 envs
    full = _batch(mapfx_mod, name)
    part = _batch(mapfx_mod, name, envs=slice(2, 7), env_offset=2)
    out = []
    for pb in (full, part):
        pb.reset()
        out.append(_host_traj(pb.rollout(T=8, eps=2 ** 30, seed=pm.SEED, t0=3, policy="pibt")))
    assert (out[0]["actions"] != 4).any()
    for k in out[0]:
        assert np.array_equal(out[0][k][:, 2:7], out[1][k]), k


def test_the_offered_limit(mapfx_mod):
    """H * W <= 32767: 127 x 256 (32512 cells, a matrix case) and 181 x 181 (32761) are offered
    and run; 128 x 256 (32768: int32 tables) is refused with nothing launched."""
    from mapfx._abi import MapfxError
    assert pm.case_of("f-w7-l16-i16")[1:3] == (127, 256)
    for name in ("f-w7-l16-i16", "edge-181x181"):
        pb = _batch(mapfx_mod, name)
        assert pb.policy_rule_offered("pibt") and pb.policy_rule_offered("descent")
        assert pb.goal_dist.element_size() == 2
    for rule in pm.RULES:
        T = pm.EDGE["edge-181x181"].T
        acts, snaps, _ = pm.rule_episode(rule, pm.refs_of("edge-181x181"), T, 2 ** 30)
        pb.reset()
        traj = pb.rollout(T=T, eps=2 ** 30, seed=pm.SEED, policy=rule)
        _assert_episode("edge-181x181", pb, traj, acts, snaps)
    pb = _batch(mapfx_mod, "edge-128x256")
    assert pb.goal_dist.element_size() == 4
    pb.reset()
    before = state_arrays(pb)
    assert pb.policy_rule_offered("descent") and not pb.policy_rule_offered("pibt")
    with pytest.raises(ValueError, match="not offered"):
        pb.rollout(T=2, eps=0.5, policy="pibt")
    with pytest.raises(MapfxError, match="on-device policy"):
        pb.rollout(T=2, eps=0.5)
    assert _differ(state_arrays(pb), before) == []
    pb.check_err()
