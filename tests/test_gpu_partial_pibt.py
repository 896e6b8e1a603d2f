"""MarlPartialBatch.rollout(policy="pibt") -- mapfx_partial_rollout under MAPFX_POLICY_PIBT, the
partial_pibt_rollout_kernel instances of csrc/partial.hip -- bit for bit against the episodes
of the rule's definition (mapfx.rng.partial_policy_pibt_actions stepped on the restatement,
tests/partial_pibt_cases.py): the actions, every trajectory slot and every state array.
tests/test_partial_pibt_ref.py holds what those episodes cover.
"""
import numpy as np
import pytest

import partial_pibt_cases as pc
from partial_rollout_cases import compare_slot, policy_run, rollout_kernel_args, POLICY_SEED
from partial_step_cases import BY_NAME, build, compare, expected_geometry, state_arrays

pytestmark = pytest.mark.gpu

FILL = 0xA5
EINVAL = -1


@pytest.fixture(scope="module")
def mapfx_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mapfx
    return mapfx


def _np(t):
    return t.detach().cpu().numpy()


def _batch(mapfx_mod, name, envs=None, limit=None, **kw):
    c, b = pc.case_of(name), pc.build_case(name)
    s = slice(None) if envs is None else envs
    grids = np.array(b["grids"]) if (c.shared or envs is None) else np.array(b["grids"])[s]
    return mapfx_mod.MarlPartialBatch(np.array(b["starts"])[s], np.array(b["goals"])[s], grids=grids,
                                      **dict(pc.params(name, limit), **kw))


def _dev(a, dtype):
    import torch
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


def _host_traj(traj):
    return {k: _np(v).copy() for k, v in traj.items()}


def _differ(a, b, keys=None):
    """The keys of two trajectory / state dicts whose bytes differ."""
    return [k for k in (keys or a) if not np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8),
                                                         np.ascontiguousarray(b[k]).view(np.uint8))]


def _assert_episode(name, pb, traj, acts, snaps, obs=True):
    got = _np(traj["actions"])
    bad = np.argwhere(got != acts)
    assert len(bad) == 0, "actions (step, env, agent) %s" % bad[:4].tolist()
    c, T = pc.case_of(name), len(snaps)
    for k in range(T):
        d = compare_slot(c, traj, k, snaps[k], obs=obs)
        assert d is None, d
    last = {f: traj[f][T - 1] for f in ("reward", "state", "avail")}
    last["obs"] = traj["obs"][T - 1] if obs else np.array(snaps[T - 1]["obs"])
    d = compare(pb, last, snaps[T - 1], "final state")
    assert d is None, d
    pb.check_err()


# ------------------------------------------------------------------ the episodes
@pytest.mark.parametrize("phase", pc.PHASES)
@pytest.mark.parametrize("eps_q", pc.EPS, ids=["eps0", "eps2^30", "eps2^32"])
@pytest.mark.parametrize("name", pc.CASES)
def test_pibt_episode_equals_the_restatement(mapfx_mod, name, eps_q, phase):
    """With and without the observation rows; fresh (the carried distances invalid: looked
    up) and after two given steps.  The last wave holds fewer envs than a wave takes
    (the 64-lane groups aside: one env per wave)."""
    import torch
    from mapfx import _abi
    c, b = pc.case_of(name), pc.build_case(name)
    epw = expected_geometry(c)["EPW"]
    assert c.E % epw != 0 or (epw == 1 and name == "dense-9x9-n64"), (name, epw)
    run = pc.run(name, eps_q, phase)
    for obs in (True, False):
        pb = _batch(mapfx_mod, name)
        pb.reset()
        if phase == "fresh":
            pb.compute_goal_dist()
            assert int(pb.pdist.max().item()) == -2 ** 31
        for t in range(run["pre"]):
            pb.step(_dev(b["actions"][t], c.dtype))
        traj = pb.rollout(T=run["T"], eps=eps_q, seed=pc.SEED, t0=run["pre"], obs=obs, policy="pibt")
        kern = _abi.last_kernel()
        torch.cuda.synchronize()
        assert pc.kernel_args(kern) == pc.expected_kernel(name, obs), kern
        assert ("obs" in traj) == obs
        _assert_episode(name, pb, traj, run["actions"], run["snaps"], obs=obs)


@pytest.mark.parametrize("name", ["dense-3x7-n5", "dense-6x6-n15"])
def test_autoreset_with_a_short_limit(mapfx_mod, name):
    limit, T, eps_q = 5, 16, 2 ** 30
    refs = pc.refs_of(name, limit)
    acts, snaps, _, _ = pc.episode(refs, T, eps_q, pc.SEED, autoreset=True)
    assert max(int(s["t"].max()) for s in snaps) <= limit
    assert sum(int((s["t"] == 1).sum()) for s in snaps[1:]) >= 2 * len(refs), "too few restarts expected"
    pb = _batch(mapfx_mod, name, limit=limit)
    pb.reset()
    traj = pb.rollout(T=T, eps=eps_q, seed=pc.SEED, autoreset=True, policy="pibt")
    _assert_episode(name, pb, traj, acts, snaps)


@pytest.mark.parametrize("name", ["dense-6x6-n15", "fast-w5-l8-i16"])
def test_two_calls_of_half_equal_one(mapfx_mod, name):
    c = pc.case_of(name)
    T, eps_q = c.T, 2 ** 30
    one = _batch(mapfx_mod, name)
    one.reset()
    whole = _host_traj(one.rollout(T=T, eps=eps_q, seed=pc.SEED, policy="pibt"))
    two = _batch(mapfx_mod, name)
    two.reset()
    first = _host_traj(two.rollout(T=T // 2, eps=eps_q, seed=pc.SEED, policy="pibt"))
    second = _host_traj(two.rollout(T=T - T // 2, eps=eps_q, seed=pc.SEED, t0=T // 2, policy="pibt"))
    halves = {k: np.concatenate([first[k], second[k]]) for k in whole}
    assert _differ(halves, whole) == []
    assert _differ(state_arrays(two), state_arrays(one)) == []
    run = pc.run(name, eps_q, "fresh")
    assert np.array_equal(whole["actions"], run["actions"])


def test_rules_alternate_on_one_handle(mapfx_mod):
    """pibt, descent, pibt in three calls of one batch: the rule is the call's."""
    import torch
    from mapfx import _abi
    name, eps_q = "dense-5x5-n20", 2 ** 30
    rules = ["pibt"] * 4 + ["descent"] * 4 + ["pibt"] * 4
    acts, snaps, _, _ = pc.episode(pc.refs_of(name), len(rules), eps_q, pc.SEED, rules=rules)
    assert int(snaps[7]["total_coll"].sum()) > int(snaps[3]["total_coll"].sum()) == 0
    pb = _batch(mapfx_mod, name)
    pb.reset()
    parts = []
    for i, (rule, kernel) in enumerate((("pibt", "partial_pibt_rollout_kernel"), ("descent", "partial_rollout_kernel"),
                                        ("pibt", "partial_pibt_rollout_kernel"))):
        parts.append(_host_traj(pb.rollout(T=4, eps=eps_q, seed=pc.SEED, t0=4 * i, policy=rule)))
        assert pc.kernel_args(_abi.last_kernel(), kernel) is not None, _abi.last_kernel()
    torch.cuda.synchronize()
    traj = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    _assert_episode(name, pb, {k: torch.as_tensor(v) for k, v in traj.items()}, acts, snaps)


@pytest.mark.parametrize("name", ["fast-w5-l16-u8t", "gen-w5-n3"])
def test_back_on_descent_the_output_is_the_descent_run(mapfx_mod, name):
    """mapfx_partial_policy_rule(h, MAPFX_POLICY_DESCENT) after a pibt call: the existing
    descent episode (tests/partial_rollout_cases.py policy_run), on the existing instance."""
    from mapfx import _abi
    from mapfx._abi import lib
    c, eps_q = BY_NAME[name], 2 ** 30
    run = policy_run(name, eps_q, "fresh")
    pb = _batch(mapfx_mod, name)
    pb.reset()
    pb.rollout(T=run["T"], eps=eps_q, seed=POLICY_SEED, policy="pibt")
    assert lib.mapfx_partial_policy_rule(pb._h, 1) == 0 and lib.mapfx_partial_policy_rule(pb._h, 0) == 0
    pb.reset()
    traj = pb.rollout(T=run["T"], eps=eps_q, seed=POLICY_SEED)       # (the default: descent)
    assert rollout_kernel_args(_abi.last_kernel()) is not None, _abi.last_kernel()
    assert np.array_equal(_np(traj["actions"]), run["actions"])
    for k in range(run["T"]):
        d = compare_slot(c, traj, k, run["snaps"][k])
        assert d is None, d


def test_pibt_is_shard_invariant(mapfx_mod):
    name = "dense-3x7-n5"
    full = _batch(mapfx_mod, name)
    part = _batch(mapfx_mod, name, envs=slice(3, 9), env_offset=3)
    out = []
    for pb in (full, part):
        pb.reset()
        out.append(_host_traj(pb.rollout(T=12, eps=2 ** 30, seed=pc.SEED, t0=3, policy="pibt")))
    assert (out[0]["actions"] != 4).any()
    for k in out[0]:
        assert np.array_equal(out[0][k][:, 3:9], out[1][k]), k


# ------------------------------------------------------------------ where it is not offered
@pytest.mark.parametrize("name", ["wg-w3-n70", "fast-w5-l16-i32"])
def test_pibt_is_refused_where_policy_mode_is_not_offered(mapfx_mod, name):
    from mapfx._abi import lib
    c = BY_NAME[name]
    b = build(c)
    pb = mapfx_mod.MarlPartialBatch(np.array(b["starts"]), np.array(b["goals"]), grids=np.array(b["grids"]),
                                    **pc.params(name))
    pb.reset()
    before = state_arrays(pb)
    assert lib.mapfx_partial_policy_rule_offered(pb._h, 0) == 1
    assert lib.mapfx_partial_policy_rule_offered(pb._h, 1) == 0
    assert lib.mapfx_partial_policy_rule(pb._h, 1) == EINVAL
    assert b"MAPFX_POLICY_PIBT" in lib.mapfx_last_error()
    with pytest.raises(ValueError, match="not offered"):
        pb.rollout(T=2, eps=0.5, policy="pibt")
    with pytest.raises(ValueError, match="not offered"):
        pb.rollout(_dev(b["actions"], "int8"), policy="pibt")
    assert _differ(state_arrays(pb), before) == []          # nothing was launched
    pb.rollout(_dev(b["actions"], "int8"))                   # given actions still run, rule descent
    pb.check_err()


def test_an_unknown_rule_is_refused_and_the_rule_stays(mapfx_mod):
    from mapfx import _abi
    from mapfx._abi import lib
    name, eps_q = "dense-3x7-n5", 0
    pb = _batch(mapfx_mod, name)
    pb.reset()
    before = state_arrays(pb)
    assert lib.mapfx_partial_policy_rule(pb._h, 1) == 0
    for rule in (2, -1, 7):
        assert lib.mapfx_partial_policy_rule_offered(pb._h, rule) == 0
        assert lib.mapfx_partial_policy_rule(pb._h, rule) == EINVAL
    assert lib.mapfx_partial_policy_rule(None, 0) == EINVAL
    assert lib.mapfx_partial_policy_rule_offered(None, 0) == 0
    with pytest.raises(ValueError, match="policy must be"):
        pb.rollout(T=2, eps=0, policy="cbs")
    assert _differ(state_arrays(pb), before) == []
    # the handle still holds pibt: a raw call (no setter) runs it
    import ctypes
    run = pc.run(name, eps_q, "fresh")
    out = pb._zeros_of(pb._traj_spec(run["T"], True, True))
    traj = _abi.PTraj(err=_abi.ptr(pb.err), **{k: _abi.ptr(out.get(k)) for k in pb.TRAJ_KEYS})
    pol = _abi.PPolicy(seed=pc.SEED, eps_q=eps_q, t0=0)
    _abi.check(pb._call(lib.mapfx_partial_rollout, pb._h, ctypes.byref(pb._state), run["T"], None, 0,
                        ctypes.byref(pol), 0, ctypes.byref(traj)), "mapfx_partial_rollout")
    assert pc.kernel_args(_abi.last_kernel()) == pc.expected_kernel(name, True)
    _assert_episode(name, pb, out, run["actions"], run["snaps"])


# ------------------------------------------------------------------ graph replay
def test_reset_and_rollout_as_one_graph(mapfx_mod):
    """[reset, rollout(pibt)] captured and replayed twice; the handle's rule is set back to
    descent before the replays: the captured launch keeps the rule it was enqueued with."""
    import torch
    from mapfx._abi import lib
    name, eps_q = "dense-6x6-n15", 2 ** 30
    c = pc.case_of(name)
    run = pc.run(name, eps_q, "fresh")
    pb = _batch(mapfx_mod, name)

    def call():
        pb.reset()
        return pb.rollout(T=c.T, eps=eps_q, seed=pc.SEED, policy="pibt")

    eager = _host_traj(call())
    assert np.array_equal(eager["actions"], run["actions"])
    end = state_arrays(pb)
    pb.reset()
    torch.cuda.synchronize()
    start = state_arrays(pb)

    def scrub():
        for v in pb._traj_cache.values():
            for t in v.values():
                t.view(torch.uint8).fill_(FILL)

    scrub()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        traj = call()
    torch.cuda.synchronize()
    assert _differ(state_arrays(pb), start) == [], "ran at capture time"
    assert bool((traj["actions"].view(torch.uint8) == FILL).all())
    assert lib.mapfx_partial_policy_rule(pb._h, 0) == 0
    for r in range(2):
        scrub()
        graph.replay()
        torch.cuda.synchronize()
        assert _differ(_host_traj(traj), eager) == [], "replay %d" % r
        assert _differ(state_arrays(pb), end) == [], "replay %d" % r
    del graph, side
    pb.check_err()
