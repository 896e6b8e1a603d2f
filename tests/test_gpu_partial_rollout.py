"""MarlPartialBatch.rollout -- mapfx_partial_rollout of csrc/partial.hip: T steps in one launch
of partial_rollout_kernel, with given actions or the on-device policy -- against the step path
(byte for byte) and the restatement (tests/partial_step_cases.py `compare`).  The expected
policy episodes and the autoreset host loop are tests/partial_rollout_cases.py's;
tests/test_partial_policy_ref.py holds what they cover.
"""
import numpy as np
import pytest

from partial_rollout_cases import (GIVEN_CASES, POLICY_CASES, POLICY_EPS, POLICY_PHASES, POLICY_SEED,
                                   autoreset_episode, compare_slot, expected_rollout_kernel,
                                   policy_run, rollout_kernel_args)
from partial_step_cases import (BY_NAME, build, compare, limit_of, make_refs, params, snapshot,
                                state_arrays)

pytestmark = pytest.mark.gpu

FILL = 0xA5
KEYS = ("reward", "obs", "state", "avail", "pos", "terminated")
_STEP_PATH = {}


@pytest.fixture(scope="module")
def mapfx_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mapfx
    return mapfx


def _np(t):
    return t.detach().cpu().numpy()


def _batch(mapfx_mod, c, b, envs=None, **kw):
    s = slice(None) if envs is None else envs
    grids = np.array(b["grids"]) if (c.shared or envs is None) else np.array(b["grids"])[s]
    return mapfx_mod.MarlPartialBatch(np.array(b["starts"])[s], np.array(b["goals"])[s], grids=grids,
                                      **dict(params(c), **kw))


def _dev(a, dtype):
    import torch
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


def _odd_rows(actions, dtype):
    """Rows 1.. of a [T + 1, E, N] tensor (row 0 holds 7s): with E * N odd the int8 rows start
    at odd byte offsets."""
    a = np.asarray(actions)
    return _dev(np.concatenate([np.full((1,) + a.shape[1:], 7), a]), dtype)[1:]


def _host_traj(traj):
    return {k: _np(v).copy() for k, v in traj.items()}


def _same(a, b, keys=None):
    """The keys of two trajectory / state dicts whose bytes differ."""
    return [k for k in (keys or a) if not np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8),
                                                         np.ascontiguousarray(b[k]).view(np.uint8))]


def _step_path(mapfx_mod, c, b, actions, dtype):
    """T step() calls: the trajectory they write, slot by slot, and the state arrays they
    leave."""
    import torch
    pb = _batch(mapfx_mod, c, b)
    pb.reset()
    acts = _dev(actions, dtype)
    slots = {k: [] for k in KEYS}
    for k in range(len(actions)):
        out = pb.step(acts[k])
        for f in ("reward", "obs", "state", "avail"):
            slots[f].append(_np(out[f]).copy())
        slots["pos"].append(_np(pb.pos).copy())
        slots["terminated"].append(_np(pb.terminated).copy())
    torch.cuda.synchronize()
    pb.err.zero_()
    return {k: np.stack(v) for k, v in slots.items()}, state_arrays(pb)


def _cached_step_path(mapfx_mod, c):
    if c.name not in _STEP_PATH:
        b = build(c)
        _STEP_PATH[c.name] = _step_path(mapfx_mod, c, b, b["actions"], c.dtype)
    return _STEP_PATH[c.name]


# ------------------------------------------------------------------ 1, 2: given actions
@pytest.mark.parametrize("obs", [True, False], ids=["obs", "noobs"])
@pytest.mark.parametrize("name", GIVEN_CASES)
def test_given_actions_equal_the_step_path_and_the_restatement(mapfx_mod, name, obs):
    import torch
    from mapfx import _abi
    c = BY_NAME[name]
    b = build(c)
    want_traj, want_state = _cached_step_path(mapfx_mod, c)
    pb = _batch(mapfx_mod, c, b)
    pb.reset()
    pb.out["obs"].view(torch.uint8).fill_(FILL)
    traj = pb.rollout(_dev(b["actions"], c.dtype), obs=obs)
    kern = _abi.last_kernel()
    torch.cuda.synchronize()
    want_kernel = expected_rollout_kernel(c, obs)
    assert pb.rollout_fused() == (want_kernel is not None)
    if want_kernel is not None:
        assert rollout_kernel_args(kern) == want_kernel, kern
    assert ("obs" in traj) == obs and "actions" not in traj
    assert bool((pb.out["obs"].view(torch.uint8) == FILL).all()), "the step's own obs buffer was written"
    for k in range(c.T):
        d = compare_slot(c, traj, k, b["snaps"][k + 1], obs=obs)
        assert d is None, d
    last = {f: traj[f][c.T - 1] for f in ("reward", "state", "avail")}
    last["obs"] = traj["obs"][c.T - 1] if obs else np.array(b["snaps"][c.T]["obs"])
    d = compare(pb, last, b["snaps"][c.T], "final state")
    assert d is None, d
    got = _host_traj(traj)
    assert _same(got, want_traj, [k for k in KEYS if k in got]) == []
    assert _same(state_arrays(pb), want_state) == []
    pb.check_err()


# ------------------------------------------------------------------ 3: T edges, chaining
@pytest.mark.parametrize("T", [1, 2, 3])
def test_short_rollouts(mapfx_mod, T):
    c = BY_NAME["act-fast"]
    b = build(c)
    pb = _batch(mapfx_mod, c, b)
    pb.reset()
    traj = pb.rollout(_odd_rows(b["actions"][:T], "int8"))
    assert traj["reward"].shape == (T, c.E)
    for k in range(T):
        d = compare_slot(c, traj, k, b["snaps"][k + 1])
        assert d is None, d
    pb.check_err()


@pytest.mark.parametrize("autoreset", [False, True], ids=["plain", "autoreset"])
@pytest.mark.parametrize("name", ["act-fast", "act-gen"])
def test_two_launches_of_4_equal_one_of_8(mapfx_mod, name, autoreset):
    c = BY_NAME[name]
    b = build(c)
    assert c.T == 8 and (c.E * c.N) % 2 == 1
    acts = _odd_rows(b["actions"], "int8")
    assert acts.storage_offset() % 2 == 1 and acts[4:].storage_offset() % 2 == 1    # odd row bases
    one =_batch(mapfx_mod, c, b)
    one.reset()
    whole = _host_traj(one.rollout(acts, autoreset=autoreset))
    two = _batch(mapfx_mod, c, b)
    two.reset()
    first = _host_traj(two.rollout(acts[:4], autoreset=autoreset))
    second = _host_traj(two.rollout(acts[4:], autoreset=autoreset))
    halves = {k: np.concatenate([first[k], second[k]]) for k in whole}
    assert _same(halves, whole) == []
    assert _same(state_arrays(two), state_arrays(one)) == []
    if not autoreset:
        for k in range(c.T):
            d = compare_slot(c, whole, k, b["snaps"][k + 1])
            assert d is None, d
    else:       # the completion env (1) restarted: it is past t = 1 again at the end
        snaps, restarts = autoreset_episode(c, b, np.asarray(b["actions"]), None)
        assert restarts[1]
        for k in range(c.T):
            d = compare_slot(c, whole, k, snaps[k])
            assert d is None, d


# ------------------------------------------------------------------ 4: autoreset
@pytest.mark.parametrize("name", ["act-fast", "act-gen", "act-wg"])
def test_autoreset_restarts_every_env(mapfx_mod, name):
    c = BY_NAME[name]
    b = build(c)
    actions = np.tile(np.asarray(b["actions"]), (3, 1, 1))
    T = 3 * (limit_of(c) + 2)
    assert actions.shape[0] == T
    snaps, restarts = autoreset_episode(c, b, actions, None)
    assert restarts[1] and restarts[2] and restarts[1][0] != restarts[2][0], restarts
    assert len(set(restarts[1]) | set(restarts[2])) >= 2
    assert all(s["t"].max() <= limit_of(c) for s in snaps)
    pb = _batch(mapfx_mod, c, b)
    pb.reset()
    traj = pb.rollout(_dev(actions, "int32"), autoreset=True)
    for k in range(T):
        d = compare_slot(c, traj, k, snaps[k])
        assert d is None, d
    last = {f: traj[f][T - 1] for f in ("reward", "obs", "state", "avail")}
    d = compare(pb, last, snaps[T - 1], "final state")
    assert d is None, d
    pb.check_err()


# ------------------------------------------------------------------ 5: an invalid action
@pytest.mark.parametrize("dtype", ["int8", "int32", "int64"])
@pytest.mark.parametrize("name", ["act-fast", "act-gen"])
def test_invalid_action_skips_one_env_for_one_step(mapfx_mod, name, dtype):
    c = BY_NAME[name]
    b = build(c)
    bad_env = c.E // 2
    a = np.array(b["actions"]).astype(np.int64)
    a[2, bad_env, c.N - 1] = 5
    refs = make_refs(c, b)
    snaps = []
    for k in range(c.T):
        for e, r in enumerate(refs):
            if k == 2 and e == bad_env:
                r.refuse()
            else:
                r.step(a[k, e])
        snaps.append(snapshot(refs))
    pb = _batch(mapfx_mod, c, b)
    pb.reset()
    traj = pb.rollout(_dev(a, dtype))
    for k in range(c.T):        # the other envs, and this one from slot 3 on, step normally
        d = compare_slot(c, traj, k, snaps[k])
        assert d is None, d
    got = _host_traj(traj)
    assert got["reward"][2, bad_env].view(np.uint64) == 0
    for f in ("pos", "state", "avail", "obs", "terminated"):
        assert np.array_equal(got[f][2, bad_env], got[f][1, bad_env]), f
    assert int(pb.err.item()) == 1 + bad_env
    with pytest.raises(AssertionError, match="invalid action"):
        pb.check_err()
    last = {f: traj[f][c.T - 1] for f in ("reward", "obs", "state", "avail")}
    d = compare(pb, last, snaps[-1], "final state")
    assert d is None, d


# ------------------------------------------------------------------ 6: the policy
@pytest.mark.parametrize("phase", POLICY_PHASES)
@pytest.mark.parametrize("eps_q", POLICY_EPS, ids=["eps0", "eps2^30", "eps2^32"])
@pytest.mark.parametrize("name", POLICY_CASES)
def test_policy_episode_equals_the_restatement(mapfx_mod, name, eps_q, phase):
    import torch
    from mapfx import _abi
    c = BY_NAME[name]
    b = build(c)
    run = policy_run(name, eps_q, phase)
    pb = _batch(mapfx_mod, c, b)
    pb.reset()
    if phase == "fresh":        # the carried distances become invalid: looked up
        pb.compute_goal_dist()
        assert int(pb.pdist.max().item()) == -2 ** 31
    for t in range(run["pre"]):
        pb.step(_dev(b["actions"][t], c.dtype))
    T = run["T"]
    traj = pb.rollout(T=T, eps=eps_q, seed=POLICY_SEED, t0=run["pre"])
    kern = _abi.last_kernel()
    torch.cuda.synchronize()
    assert rollout_kernel_args(kern) == expected_rollout_kernel(c, True), kern
    got = _np(traj["actions"])
    bad = np.argwhere(got != run["actions"])
    assert len(bad) == 0, "actions (step, env, agent) %s" % bad[:4].tolist()
    for k in range(T):
        d = compare_slot(c, traj, k, run["snaps"][k])
        assert d is None, d
    last = {f: traj[f][T - 1] for f in ("reward", "obs", "state", "avail")}
    d = compare(pb, last, run["snaps"][T - 1], "final state")
    assert d is None, d
    pb.check_err()


def test_policy_is_shard_invariant(mapfx_mod):
    c = BY_NAME["fast-w5-l16-u8t"]
    b = build(c)
    assert c.E == 21
    full = _batch(mapfx_mod, c, b)
    part = _batch(mapfx_mod, c, b, envs=slice(5, 13), env_offset=5)
    out = []
    for pb in (full, part):
        pb.reset()
        out.append(_host_traj(pb.rollout(T=c.T, eps=2 ** 30, seed=POLICY_SEED, t0=3)))
    assert (out[0]["actions"] != 4).any()
    for k in out[0]:
        assert np.array_equal(out[0][k][:, 5:13], out[1][k]), k


@pytest.mark.parametrize("name", ["fast-w5-l16-i32", "wg-w3-n70"])
def test_policy_is_refused_where_it_is_not_offered(mapfx_mod, name):
    from mapfx._abi import MapfxError
    c = BY_NAME[name]
    pb = _batch(mapfx_mod, c, build(c))
    pb.reset()
    before = state_arrays(pb)
    with pytest.raises(MapfxError, match="on-device policy"):
        pb.rollout(T=2, eps=0.5)
    assert _same(state_arrays(pb), before) == []


def test_bad_arguments_raise(mapfx_mod):
    import torch
    from mapfx._abi import MapfxError
    c = BY_NAME["act-fast"]
    b = build(c)
    pb = _batch(mapfx_mod, c, b)
    pb.reset()
    with pytest.raises(ValueError):
        pb.rollout()
    with pytest.raises(ValueError):
        pb.rollout(T=2, eps=1.5)
    with pytest.raises(AssertionError, match="actions must be"):
        pb.rollout(torch.zeros((2, c.E, c.N + 1), dtype=torch.int8).cuda())
    with pytest.raises(MapfxError, match="T must be"):
        pb.rollout(T=65537, eps=0, out={})
    with pytest.raises(MapfxError, match="T must be"):
        pb.rollout(T=0, eps=0, out={})


# ------------------------------------------------------------------ 7: guard bytes
def _guarded(shape, dtype, pool):
    """A 16-byte-aligned view of `shape` inside a longer buffer, 256 sentinel bytes (and the
    alignment slack) either side: slot T - 1 ends where the sentinels begin."""
    import torch
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((256 + 16 + n + 256,), FILL, dtype=torch.uint8, device="cuda")
    off = 256 + (-(buf.data_ptr() + 256)) % 16
    view = buf[off:off + n].view(dtype).view(shape)
    assert view.data_ptr() % 16 == 0
    pool.append((buf, off, n))
    return view


def _guards_intact(pool):
    return all(bool((buf[:off] == FILL).all()) and bool((buf[off + n:] == FILL).all()) for buf, off, n in pool)


@pytest.mark.parametrize("mode", ["given", "policy"])
def test_guard_bytes_and_the_clamped_action_fetch(mapfx_mod, mode):
    import torch
    c = BY_NAME["act-fast" if mode == "given" else "fast-w5-l16-i16"]
    b = build(c)
    T = c.T
    pb = _batch(mapfx_mod, c, b)
    pb.reset()
    pool = []
    spec = pb._traj_spec(T, True, mode == "policy")
    out = {k: _guarded(shape, dt, pool) for k, (shape, dt) in spec.items()}
    if mode == "given":
        # the int8 actions are the tail of their allocation: a fetch of a row past T - 1
        # would leave it (the kernel clamps the row it prefetches)
        n = T * c.E * c.N
        store = torch.full((4096 + n,), 7, dtype=torch.int8, device="cuda")
        acts = store[4096:].view(T, c.E, c.N)
        acts.copy_(_dev(b["actions"], "int8"))
        assert acts.data_ptr() + n == store.data_ptr() + store.numel()
        traj = pb.rollout(acts, out=out)
        for k in range(T):
            d = compare_slot(c, traj, k, b["snaps"][k + 1])
            assert d is None, d
    else:
        run = policy_run(c.name, 2 ** 30, "fresh")
        traj = pb.rollout(T=T, eps=2 ** 30, seed=POLICY_SEED, out=out)
        assert np.array_equal(_np(traj["actions"]), run["actions"])
    torch.cuda.synchronize()
    assert traj is out
    assert _guards_intact(pool)
    pb.check_err()


# ------------------------------------------------------------------ 8: graph replay
@pytest.mark.parametrize("mode", ["given", "policy"])
def test_graph_replay_equals_the_eager_call(mapfx_mod, mode):
    import torch
    c = BY_NAME["fast-w5-l16-u8t"]
    b = build(c)
    pb = _batch(mapfx_mod, c, b)
    acts = _dev(b["actions"], "int8")
    names = ("pos", "steps", "at_goal", "done", "goal_cost", "node", "edge", "t", "terminated",
             "total_coll", "pdist", "pnbr")

    def call():
        if mode == "given":
            return pb.rollout(acts)
        return pb.rollout(T=c.T, eps=2 ** 30, seed=POLICY_SEED)

    pb.reset()
    torch.cuda.synchronize()
    start = {n: getattr(pb, n).clone() for n in names}
    eager = _host_traj(call())
    end = state_arrays(pb)

    def restore():
        for n in names:
            getattr(pb, n).copy_(start[n])
        for v in pb._traj_cache.values():
            for t in v.values():
                t.view(torch.uint8).fill_(FILL)

    restore()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        traj = call()
    torch.cuda.synchronize()
    assert _same(state_arrays(pb), {n: _np(start[n]) for n in state_arrays(pb)}) == [], "ran at capture time"
    for r in range(2):
        restore()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(_host_traj(traj), eager) == [], "replay %d" % r
        assert _same(state_arrays(pb), end) == [], "replay %d" % r
    del graph, side
    pb.check_err()
