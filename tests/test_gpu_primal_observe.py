"""GPU parity of the PRIMAL read-only interface (mapfx_primal_observe, include/mapfx_primal.h;
PrimalBatch.observe, MAPFEnv._observe / _listNextValidActions / _complete): against the
reference's own snapshots (tests/golden/primal_observe/po_*.npz), against the CPU
restatement on random batches, and against mapfx_primal_act at the bench shape.
Everything bit-exact (goal vectors as fp64 bit patterns), and the worlds are bit-identical
before and after every query."""
import numpy as np
import pytest
import torch

from test_primal_observe_ref import FIXTURES, load_po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mapfx_mod():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mapfx
    return mapfx


def _np(t):
    return t.detach().cpu().numpy()


def _grab(o):
    return {k: _np(v).copy() for k, v in o.items()}


def _state(b):
    return _np(b.pos).copy(), (_np(b.past).copy() if b.past is not None else None)


def _same_state(b, st):
    pos, past = _state(b)
    return np.array_equal(pos, st[0]) and (past is None or np.array_equal(past, st[1]))


def _check_snapshot(b, fx, i, nact):
    """observe() and observe(ids, prev) over the full (agent, prev_action) grid against
    snapshot i of the reference; the world is left as it was."""
    n = len(fx["starts"])
    before = _state(b)
    assert np.array_equal(before[0][0], fx["pos"][i])
    if b.past is not None:
        assert np.array_equal(before[1][0], fx["past"][i])
    o = _grab(b.observe())
    assert _same_state(b, before)
    assert np.array_equal(o["obs"][0], fx["obs"][i])
    assert np.array_equal(o["vec"][0].view(np.uint64), fx["vec"][i].view(np.uint64))
    assert np.array_equal(o["next_mask"][0], fx["next_mask"][i, :, 0])
    assert np.array_equal(o["on_goal"][0].astype(bool), fx["on_goal"][i])
    assert (o["done"][0] == int(fx["done"][i])).all()
    ids = np.repeat(np.arange(1, n + 1), nact)[None]
    prev = np.tile(np.arange(nact), n)[None]
    o = _grab(b.observe(ids, prev))
    assert _same_state(b, before)
    assert np.array_equal(o["obs"][0], np.repeat(fx["obs"][i], nact, 0))
    assert np.array_equal(o["vec"][0].view(np.uint64), np.repeat(fx["vec"][i], nact, 0).view(np.uint64))
    assert np.array_equal(o["next_mask"][0], fx["next_mask"][i].reshape(-1))
    assert np.array_equal(o["on_goal"][0].astype(bool), np.repeat(fx["on_goal"][i], nact))
    assert (o["done"][0] == int(fx["done"][i])).all()


# the host's choice / one wave per query / one lane per query wherever its LDS fits
PATHS = ["", "waves", "lanes"]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", FIXTURES)
def test_observe_matches_reference_snapshots(mapfx_mod, monkeypatch, name, path):
    monkeypatch.setenv("MAPFX_PRIMAL_OBSERVE", path)
    fx = load_po(name)
    diag = bool(fx["diagonal"])
    mk = lambda: mapfx_mod.PrimalBatch(fx["starts"][None], fx["goals"][None], grids=fx["grid"][None],  # noqa: E731
                                       observation_size=int(fx["size"]), diagonal=diag)
    b, plain = mk(), mk()
    cuts = [int(k) for k in fx["snap_at"]]
    last = 0
    for i, k in enumerate(cuts):
        if k > last:
            b.act(fx["agent"][None, last:k], fx["action"][None, last:k])
            plain.act(fx["agent"][None, last:k], fx["action"][None, last:k])
        last = k
        _check_snapshot(b, fx, i, 9 if diag else 5)
    n = len(fx["agent"])
    if n > last:
        b.act(fx["agent"][None, last:n], fx["action"][None, last:n])
        plain.act(fx["agent"][None, last:n], fx["action"][None, last:n])
    b.check_err()
    # the same calls with no observe in between end in the same world
    assert _same_state(b, _state(plain))


def _fixture_env(mapfx_mod, fx):
    from mapfx.primal import MAPFEnv
    world = fx["grid"].astype(np.int64)
    gg = np.zeros_like(world)
    for a, ((r, c), (gr, gc)) in enumerate(zip(fx["starts"], fx["goals"])):
        world[r, c] = a + 1
        gg[gr, gc] = a + 1
    env = MAPFEnv(num_agents=len(fx["starts"]), observation_size=int(fx["size"]), world0=world,
                  goals0=gg, DIAGONAL_MOVEMENT=bool(fx["diagonal"]))
    return env, world, gg


@pytest.mark.parametrize("name", FIXTURES)
def test_dropin_matches_reference_snapshots(mapfx_mod, name):
    fx = load_po(name)
    env, _, _ = _fixture_env(mapfx_mod, fx)
    n, nact = len(fx["starts"]), 9 if bool(fx["diagonal"]) else 5
    snaps = {int(k): i for i, k in enumerate(fx["snap_at"])}
    for k in range(len(fx["agent"]) + 1):
        if k in snaps:
            i = snaps[k]
            for a in range(1, n + 1):
                maps, vec = env._observe(a)
                assert isinstance(maps, list) and len(maps) == 4 and isinstance(vec, list)
                assert np.array_equal(np.stack(maps), fx["obs"][i, a - 1])
                assert np.array_equal(np.array(vec).view(np.uint64), fx["vec"][i, a - 1].view(np.uint64))
                for p in range(nact):
                    nxt = env._listNextValidActions(a, p) if p else env._listNextValidActions(a)
                    assert nxt == sorted(nxt) and sum(1 << x for x in nxt) == int(fx["next_mask"][i, a - 1, p])
            assert env._complete() is bool(fx["done"][i])
            assert env.getPositions() == [tuple(p) for p in fx["pos"][i].tolist()]
            if env.batch.past is not None:
                assert np.array_equal(_np(env.batch.past)[0], fx["past"][i])
        if k < len(fx["agent"]):
            env._step((int(fx["agent"][k]), int(fx["action"][k])))
    with pytest.raises(AssertionError):
        env._observe(0)


def test_dropin_reset_is_a_query(mapfx_mod):
    """_reset(agent_id, world0, goals0) on a DIAGONAL_MOVEMENT world: the reference's return
    (snapshot 0 is the fresh world), and agents_past still equal to the starts."""
    fx = load_po("po_diag_crowd6_n14")
    assert int(fx["snap_at"][0]) == 0
    env, world, gg = _fixture_env(mapfx_mod, fx)
    for k in range(20):  # a used world: _reset builds a new one
        env._step((int(fx["agent"][k]), int(fx["action"][k])))
    for a in (1, 7, len(fx["starts"])):
        nxt, on_goal, blocking = env._reset(a, world0=world, goals0=gg)
        assert sum(1 << x for x in nxt) == int(fx["next_mask"][0, a - 1, 0]) and nxt == sorted(nxt)
        assert on_goal is bool(fx["on_goal"][0, a - 1]) and blocking is False
        assert np.array_equal(_np(env.batch.past)[0], fx["starts"])
        assert np.array_equal(_np(env.batch.pos)[0], fx["starts"])


# ---------------------------------------------------------------------------
# random batches against the restatement
# ---------------------------------------------------------------------------
def _random_worlds(rng, E, H, W, N, density, shared):
    n_maps = 1 if shared else E
    grids = np.where(rng.random((n_maps, H, W)) < density, -1, 0).astype(np.int8)
    starts = np.zeros((E, N, 2), np.int32)
    goals = np.zeros((E, N, 2), np.int32)
    for e in range(E):
        free = np.argwhere(grids[0 if shared else e] == 0)
        idx = rng.choice(len(free), size=2 * N, replace=False)
        starts[e] = free[idx[:N]]
        goals[e] = free[idx[N:]]
    return grids, starts, goals


class _Want:
    """The restatement's answers for one world as it stands, computed once per agent."""

    def __init__(self, w):
        from oracle.mapf_oracle import primal_obs
        self.w = w
        self.maps, self.vec = primal_obs(w.grid, w.pos, w.goals, w.size, agents=list(range(w.n)))
        self.done = w.done()
        self.masks = {}

    def mask(self, a, p):
        if (a, p) not in self.masks:
            self.masks[(a, p)] = self.w.next_mask(a, p)
        return self.masks[(a, p)]

    def check(self, o, e, ids, prev, skip=()):
        for q in range(len(ids)):
            if q in skip:
                continue
            a, p = int(ids[q]) - 1, int(prev[q])
            assert np.array_equal(o["obs"][e, q], self.maps[a]), (e, q)
            assert np.array_equal(o["vec"][e, q].view(np.uint64), self.vec[a].view(np.uint64)), (e, q)
            assert int(o["next_mask"][e, q]) == self.mask(a, p), (e, q)
            assert bool(o["on_goal"][e, q]) == (self.w.pos[a] == self.w.goals[a]), (e, q)
            assert bool(o["done"][e, q]) == self.done, (e, q)


def _driven(mapfx_mod, rng, E, H, W, N, s, shared, diag, density, K):
    """A batch after K random calls per world, and the restatement's worlds after the same."""
    from oracle.primal_dyn_oracle import PrimalWorld
    grids, starts, goals = _random_worlds(rng, E, H, W, N, density, shared)
    nact = 9 if diag else 5
    ids = rng.integers(1, N + 1, size=(E, K)).astype(np.int32)
    acts = rng.choice(nact, size=(E, K), p=[0.08] + [0.92 / (nact - 1)] * (nact - 1)).astype(np.int32)
    b = mapfx_mod.PrimalBatch(starts, goals, grids=grids, observation_size=s, diagonal=diag)
    b.act(ids, acts)
    b.check_err()
    worlds = []
    for e in range(E):
        w = PrimalWorld(grids[0 if shared else e], starts[e], goals[e], s, diagonal=diag)
        for k in range(K):
            w.move(int(ids[e, k]) - 1, int(acts[e, k]))
        worlds.append(w)
    assert np.array_equal(np.array([w.pos for w in worlds]), _np(b.pos))
    return b, worlds


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("diag", [False, True])
@pytest.mark.parametrize("E,H,W,N,s,shared,density", [
    (7, 12, 12, 10, 7, False, 0.2),
    (7, 9, 13, 30, 4, True, 0.1),         # a shared map, crowded, non-square
    (7, 40, 33, 100, 11, False, 0.15),    # N > 64: two rounds of agents, Q = N + 3 > 64
    (2, 128, 128, 255, 32, False, 0.1),   # the ABI limits: the largest LDS of either kernel
    (7, 2, 8000, 5, 3, False, 0.05),      # extreme aspect
    (7, 20, 20, 12, 1, False, 0.1),       # s = 1: a record is one dword
])
def test_observe_batch_matches_restatement(mapfx_mod, monkeypatch, E, H, W, N, s, shared, density, diag,
                                           path):
    monkeypatch.setenv("MAPFX_PRIMAL_OBSERVE", path)
    rng = np.random.default_rng(H * 1000 + N + (7 if diag else 0))
    nact = 9 if diag else 5
    b, worlds = _driven(mapfx_mod, rng, E, H, W, N, s, shared, diag, density, 3 * N)
    want = [_Want(w) for w in worlds]
    before = _state(b)
    all_ids, zeros = np.arange(1, N + 1), np.zeros(N, np.int64)
    # every agent
    o = _grab(b.observe())
    assert o["obs"].shape == (E, N, 4, s, s) and o["vec"].shape == (E, N, 3)
    for e in range(E):
        want[e].check(o, e, all_ids, zeros)
    # Q = 1
    ids = rng.integers(1, N + 1, size=(E, 1))
    prev = rng.integers(0, nact, size=(E, 1))
    o = _grab(b.observe(ids, prev))
    for e in range(E):
        want[e].check(o, e, ids[e], prev[e])
    # Q = N + 3, repeated ids, random previous actions (tensors on the device)
    ids = rng.integers(1, N + 1, size=(E, N + 3))
    ids[:, -3:] = ids[:, :3]
    prev = rng.integers(0, nact, size=(E, N + 3))
    o = _grab(b.observe(torch.from_numpy(ids).cuda(), torch.from_numpy(prev).cuda()))
    for e in range(E):
        want[e].check(o, e, ids[e], prev[e])
    # previous actions alone: every agent, Q = N
    prev = rng.integers(0, nact, size=(E, N))
    o = _grab(b.observe(None, prev))
    for e in range(E):
        want[e].check(o, e, all_ids, prev[e])
    b.check_err()
    assert _same_state(b, before)


@pytest.mark.parametrize("path", PATHS)
def test_observe_more_queries_than_a_workgroup_holds(mapfx_mod, monkeypatch, path):
    """Q = 200 > 64 on a small world: a world's queries span several waves (lane per
    query), or 13 workgroups per world, the last ones partly empty (wave per query)."""
    monkeypatch.setenv("MAPFX_PRIMAL_OBSERVE", path)
    rng = np.random.default_rng(5)
    E, N, Q = 7, 6, 200
    b, worlds = _driven(mapfx_mod, rng, E, 10, 11, N, 6, False, False, 0.15, 3 * N)
    ids = rng.integers(1, N + 1, size=(E, Q))
    prev = rng.integers(0, 5, size=(E, Q))
    o = _grab(b.observe(ids, prev))
    b.check_err()
    for e in range(E):
        _Want(worlds[e]).check(o, e, ids[e], prev[e])


def test_observe_keeps_act_result(mapfx_mod):
    """observe has its own buffers: the dict an act call returned stays valid."""
    rng = np.random.default_rng(9)
    b, _ = _driven(mapfx_mod, rng, 3, 8, 8, 5, 4, False, False, 0.1, 15)
    kept = _grab(b.out)
    o1 = b.observe()
    assert o1 is b.observe() and b.out is not o1
    for k, v in kept.items():
        assert np.array_equal(_np(b.out[k]), v), k


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("diag", [False, True])
def test_observe_bad_query_spares_the_rest(mapfx_mod, monkeypatch, diag, path):
    """World 2, query 3 is bad (an id of N + 1; DIAGONAL_MOVEMENT: a prev_action of 9):
    err names world 2, the query's own elements are untouched, every other query --
    world 2's others included -- is answered."""
    monkeypatch.setenv("MAPFX_PRIMAL_OBSERVE", path)
    rng = np.random.default_rng(11 + diag)
    E, N, Q, s = 5, 6, 8, (4 if diag else 5)
    nact = 9 if diag else 5
    b, worlds = _driven(mapfx_mod, rng, E, 9, 9, N, s, False, diag, 0.1, 3 * N)
    ids = rng.integers(1, N + 1, size=(E, Q))
    prev = rng.integers(0, nact, size=(E, Q))
    b.observe(ids, prev)  # the buffers for this Q
    for v in b.obs_out.values():
        v.view(torch.uint8).fill_(0xAB)
    if diag:
        prev[2, 3] = 9
    else:
        ids[2, 3] = N + 1
    o = _grab(b.observe(ids, prev))
    with pytest.raises(AssertionError, match="world 2"):
        b.check_err()
    b.check_err()  # reported once
    for k, v in o.items():
        assert (v[2, 3:4].view(np.uint8) == 0xAB).all(), k
    for e in range(E):
        _Want(worlds[e]).check(o, e, ids[e], prev[e], skip=(3,) if e == 2 else ())
    # without agent_ids every agent is queried: Q must be N
    with pytest.raises(AssertionError):
        b.observe(None, np.zeros((E, N + 1), np.int64))
    with pytest.raises(AssertionError):
        b.observe(ids[:E - 1], prev[:E - 1])
    with pytest.raises(AssertionError):
        b.observe(ids, prev[:, :Q - 1])
    from mapfx import _abi
    import ctypes
    assert _abi.lib.mapfx_primal_observe(b._h, ctypes.byref(b._state), None, None, N + 1,
                                         ctypes.byref(b._obs_out), None) != 0
    assert b"Q must equal" in _abi.lib.mapfx_last_error()
    assert _abi.lib.mapfx_primal_observe(b._h, ctypes.byref(b._state), None, None, -1,
                                         ctypes.byref(b._obs_out), None) != 0
    assert _abi.lib.mapfx_primal_observe(None, ctypes.byref(b._state), None, None, N, None, None) != 0
    assert _abi.lib.mapfx_primal_observe(b._h, None, None, None, N, None, None) != 0
    dev_ids = torch.from_numpy(ids).to(torch.int32).cuda()
    assert _abi.lib.mapfx_primal_observe(b._h, ctypes.byref(b._state), dev_ids.data_ptr(), None, 0,
                                         None, None) == 0  # Q == 0: nothing to do
    if diag:
        st = _abi.QState(pos=b._state.pos, goal=b._state.goal, map_bits=b._state.map_bits, past=None)
        assert _abi.lib.mapfx_primal_observe(b._h, ctypes.byref(st), None, None, N, None, None) != 0


def test_observe_bench_shape_equals_stay_calls(mapfx_mod):
    """bench.py --env primal's shape: 4096 worlds of 32 x 32, 16 agents, s = 10.  After 64
    random calls observe() of all 65,536 agents equals act(ids = 1..N, actions = 0) on a
    second, identically driven batch (a non-diagonal stay moves nothing)."""
    from mapfx.maps import synthetic_instances
    E, S, N, s, K = 4096, 32, 16, 10, 64
    inst = synthetic_instances(E, S, S, N, p_obstacle=0.10, seed=1)
    mk = lambda: mapfx_mod.PrimalBatch(inst["init_pos"], inst["goals"], bits=inst["bits"], hw=(S, S),  # noqa: E731
                                       observation_size=s)
    b, c = mk(), mk()
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, N + 1, (E, K), generator=g, dtype=torch.int32).cuda()
    acts = torch.randint(0, 5, (E, K), generator=g, dtype=torch.int32).cuda()
    b.act(ids, acts)
    c.act(ids, acts)
    pos = b.pos.clone()
    o = b.observe()
    stay = c.act(torch.arange(1, N + 1, dtype=torch.int32).repeat(E, 1).cuda(),
                 torch.zeros((E, N), dtype=torch.int32).cuda())
    b.check_err()
    c.check_err()
    assert torch.equal(b.pos, pos) and torch.equal(b.pos, c.pos)
    for k in ("obs", "on_goal", "done", "next_mask"):
        assert torch.equal(o[k], stay[k]), k
    assert torch.equal(o["vec"].view(torch.int64), stay["vec"].view(torch.int64))
    assert int(o["obs"].sum().item()) > 0
