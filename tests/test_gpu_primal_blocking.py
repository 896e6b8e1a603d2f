"""GPU parity of PRIMAL's stay-on-goal blocking penalty (mapfx_primal_blocking,
mapfx_primal_blocking_count; include/mapfx_primal.h): against the reference's own
outputs (tests/golden/primal_blocking/pb_*.npz, pbq_*.npz) and against the plain-Python restatement
(tests/primal_blocking_ref.py) on batched worlds.  Everything exact: rewards as fp64
bit patterns, counts, flags and positions.  Grids that fit 64 x 64 take the lane-per-row
kernel; MAPFX_PRIMAL_BLOCKING=flat pins the flat-set kernel of the larger grids there too."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from primal_blocking_ref import BlockingWorld, rooms_layout, rooms_script, rooms_world

pytestmark = pytest.mark.gpu

BLOCKING = os.path.join(GOLDEN, "primal_blocking")
PB = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(BLOCKING, "pb_*.npz")))
PBQ = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(BLOCKING, "pbq_*.npz")))
PATHS = ["", "flat"]  # the host's choice of kernel / the flat-set kernel at every shape
PD = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "pd_*.npz")))


@pytest.fixture(scope="module")
def mapfx_mod():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mapfx
    return mapfx


def _load(name):
    with np.load(os.path.join(GOLDEN if name.startswith("pd_") else BLOCKING, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def _np(t):
    return t.detach().cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- 1. blocking_count of every agent in every pbq state ----
@pytest.mark.parametrize("name", PBQ)
@pytest.mark.parametrize("path", PATHS)
def test_blocking_count_matches_reference(mapfx_mod, monkeypatch, path, name):
    monkeypatch.setenv("MAPFX_PRIMAL_BLOCKING", path)
    fx = _load(name)
    S, N = fx["counts"].shape
    starts = np.repeat(fx["states"], N, axis=0)            # world (state, agent)
    goals = np.repeat(fx["goals"][None], S * N, axis=0)
    ids = np.tile(np.arange(1, N + 1, dtype=np.int32), S)
    for blocking in (False, True):
        b = mapfx_mod.PrimalBatch(starts, goals, grids=fx["grid"][None], observation_size=int(fx["size"]),
                                  blocking=blocking)
        got = b.blocking_count(ids)
        assert got.dtype == torch.int32 and tuple(got.shape) == (S * N,)
        assert np.array_equal(_np(got).reshape(S, N), fx["counts"])
        assert np.array_equal(_np(b.pos), starts)


# ---- 2. the reference's call sequences through act(), in one launch or several ----
@pytest.mark.parametrize("name", PB)
@pytest.mark.parametrize("chunk", [0, 1, 7])
@pytest.mark.parametrize("path", PATHS)
def test_blocking_matches_reference_calls(mapfx_mod, monkeypatch, path, name, chunk):
    monkeypatch.setenv("MAPFX_PRIMAL_BLOCKING", path)
    fx = _load(name)
    b = mapfx_mod.PrimalBatch(fx["starts"][None], fx["goals"][None], grids=fx["grid"][None],
                              observation_size=int(fx["size"]), diagonal=bool(fx["diagonal"]),
                              blocking=True)
    n = len(fx["agent"])
    step = n if chunk == 0 else chunk
    for k0 in range(0, n, step):
        k1 = min(n, k0 + step)
        o = b.act(fx["agent"][None, k0:k1], fx["action"][None, k0:k1])
        sl = slice(k0, k1)
        assert np.array_equal(_bits(_np(o["reward"])[0]), _bits(fx["reward"][sl]))
        assert np.array_equal(_np(o["blocking"])[0].astype(bool), fx["blocking"][sl])
        assert np.array_equal(_np(o["n_blocking"])[0], fx["n_blocking"][sl])
        assert np.array_equal(_np(o["done"])[0].astype(bool), fx["done"][sl])
        assert np.array_equal(_np(o["next_mask"])[0], fx["next_mask"][sl])
        assert np.array_equal(_np(o["on_goal"])[0].astype(bool), fx["on_goal"][sl])
        assert np.array_equal(_np(o["valid"])[0].astype(bool), fx["valid"][sl])
        assert np.array_equal(_np(b.pos)[0], fx["pos"][k1 - 1])
    b.check_err()


# ---- 3. the dynamics fixtures: the pass changes nothing but the three blocking outputs ----
@pytest.mark.parametrize("name", PD)
def test_dynamics_goldens_with_and_without_blocking(mapfx_mod, name):
    fx = _load(name)
    diag = bool(fx.get("diagonal", False))
    stay_on_goal = (fx["action"] == 0) & fx["on_goal"]
    for blocking in (False, True):
        b = mapfx_mod.PrimalBatch(fx["starts"][None], fx["goals"][None], grids=fx["grid"][None],
                                  observation_size=int(fx["size"]), diagonal=diag, blocking=blocking)
        o = b.act(fx["agent"][None], fx["action"][None])
        assert ("blocking" in o) == blocking and ("n_blocking" in o) == blocking
        assert set(o) == {"reward", "done", "next_mask", "on_goal", "valid", "obs", "vec"} | \
            ({"blocking", "n_blocking"} if blocking else set())
        assert np.array_equal(_np(o["done"])[0].astype(bool), fx["done"])
        assert np.array_equal(_np(o["next_mask"])[0], fx["next_mask"])
        assert np.array_equal(_np(o["on_goal"])[0].astype(bool), fx["on_goal"])
        assert np.array_equal(_np(o["valid"])[0].astype(bool), fx["valid"])
        assert np.array_equal(_np(o["obs"])[0], fx["obs"])
        assert np.array_equal(_bits(_np(o["vec"])[0]), _bits(fx["vec"]))
        assert np.array_equal(_np(b.pos)[0], fx["pos"][-1])
        if diag:
            assert np.array_equal(_np(b.past)[0], fx["past"][-1])
        rw = _np(o["reward"])[0]
        if not blocking:
            assert np.array_equal(_bits(rw), _bits(fx["reward"]))
        else:  # the fixtures hold the term as 0: every other call's reward is theirs
            assert np.array_equal(_bits(rw[~stay_on_goal]), _bits(fx["reward"][~stay_on_goal]))
            nb = _np(o["n_blocking"])[0]
            assert np.array_equal(_bits(rw[stay_on_goal]), _bits(0.0 + nb[stay_on_goal] * -1.0))
            assert (nb[~stay_on_goal] == 0).all()
            assert np.array_equal(_np(o["blocking"])[0], (nb > 0).astype(np.uint8))


# ---- 4 / 5. batches against the restatement ----
def _restate(grids, starts, goals, s, diag, ids, acts):
    """The restatement of every world: reward bits, blocking, n, on_goal, valid, final positions."""
    E, K = ids.shape
    rew = np.zeros((E, K), np.float64)
    blk = np.zeros((E, K), np.uint8)
    cnt = np.zeros((E, K), np.int32)
    ong = np.zeros((E, K), np.uint8)
    val = np.zeros((E, K), np.uint8)
    pos = np.zeros(starts.shape, np.int32)
    for e in range(E):
        w = BlockingWorld(grids[e if len(grids) > 1 else 0], starts[e], goals[e], size=s, diagonal=diag)
        for k in range(K):
            _, _, r, _, _, on_goal, blocking, valid = w.step(int(ids[e, k]) - 1, int(acts[e, k]))
            rew[e, k], blk[e, k], cnt[e, k], ong[e, k], val[e, k] = r, blocking, w.last_n, on_goal, valid
        pos[e] = np.array(w.pos, dtype=np.int32)
    return rew, blk, cnt, ong, val, pos


def _check_batch(mapfx_mod, grids, starts, goals, s, diag, ids, acts):
    b = mapfx_mod.PrimalBatch(starts, goals, grids=grids, observation_size=s, diagonal=diag, blocking=True)
    o = b.act(ids, acts)
    b.check_err()
    rew, blk, cnt, ong, val, pos = _restate(grids, starts, goals, s, diag, ids, acts)
    assert np.array_equal(_np(o["on_goal"]), ong) and np.array_equal(_np(o["valid"]), val)
    assert np.array_equal(_np(b.pos), pos)
    assert np.array_equal(_np(o["n_blocking"]), cnt)
    assert np.array_equal(_np(o["blocking"]), blk)
    assert np.array_equal(_bits(_np(o["reward"])), _bits(rew))
    return cnt, ong


@pytest.fixture(scope="module")
def rooms_batch():
    """70 distinct rooms worlds (and 70 placements on one shared layout), N = 12, K = 65."""
    E, N, K, H, W = 70, 12, 65, 14, 14
    out = {}
    for i, (shared, diag) in enumerate(((False, False), (True, False), (False, True))):
        rng = np.random.default_rng(2024 + i)
        layout = rooms_layout(rng, H, W) if shared else None
        grids, starts, goals, doors, ids, acts = [], [], [], [], [], []
        for e in range(E):
            g, st, gl, da = rooms_world(rng, H, W, N, 5, layout=layout)
            calls = rooms_script(rng, N, da, 6, 9 if diag else 5)[:K]
            grids.append(g), starts.append(st), goals.append(gl), doors.append(da)
            ids.append([c[0] for c in calls]), acts.append([c[1] for c in calls])
        out[shared, diag] = (np.stack(grids[:1] if shared else grids), np.array(starts, np.int32),
                             np.array(goals, np.int32), doors, np.array(ids, np.int32),
                             np.array(acts, np.int32))
    return out


@pytest.mark.parametrize("shared,diag", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("path", PATHS)
def test_blocking_batch_matches_restatement(mapfx_mod, monkeypatch, rooms_batch, path, shared, diag):
    """E = 70 (no multiple of a worlds-per-wave count), K = 65 (crosses the step kernel's
    64-call block); the last agent sits in a doorway in some worlds and walks in others."""
    monkeypatch.setenv("MAPFX_PRIMAL_BLOCKING", path)
    grids, starts, goals, doors, ids, acts = rooms_batch[shared, diag]
    N = starts.shape[1]
    assert any(N - 1 in d for d in doors) and any(N - 1 not in d for d in doors)
    cnt, ong = _check_batch(mapfx_mod, grids, starts, goals, 10, diag, ids, acts)
    stays = (acts == 0) & (ong != 0)
    assert stays.sum() >= 500 and (cnt > 0).sum() >= 50 and cnt.max() >= 2
    last = ids == N  # the last agent as the sitter is penalised too (it examines 1 .. N - 1)
    assert (cnt[last] > 0).any()


def _serpentine(n):
    g = np.zeros((n, n), dtype=np.int8)
    for r in range(1, n, 2):
        g[r, :] = -1
        g[r, n - 1 if (r // 2) % 2 == 0 else 0] = 0
    return g


def _wide_shapes():
    """Grids with a side over 64, and the edges of the lane-per-row kernel (a side of
    exactly 64): (name, grids [E, H, W], starts, goals, s, calls per world)."""
    cases = []
    for h, w, n, nd, rounds, seed in ((64, 64, 60, 30, 2, 6468), (64, 17, 20, 10, 3, 6417),
                                      (17, 64, 20, 10, 3, 1764)):
        rng = np.random.default_rng(seed)
        gs, sts, gls, cl = [], [], [], []
        for e in range(5):
            gr, s0, g0, da = rooms_world(rng, h, w, n, nd)
            gs.append(gr), sts.append(s0), gls.append(g0), cl.append(rooms_script(rng, n, da, rounds))
        cases.append(("%dx%d" % (h, w), np.stack(gs), np.array(sts, np.int32), np.array(gls, np.int32), 10, cl))
    # the last row, lane and bit of the lane-per-row kernel: a wall in row 62 with doors at
    # columns 0 and 63; world 0's sitter stands in the door at column 63, world 1's at 0
    g = np.zeros((64, 64), dtype=np.int8)
    g[62, 1:63] = -1
    st = np.array([[(61, 63), (62, 63), (0, 0)], [(61, 0), (62, 0), (0, 0)]], np.int32)
    gl = np.array([[(63, 63), (62, 63), (0, 5)], [(63, 0), (62, 0), (0, 5)]], np.int32)
    calls = [(2, 0), (1, 4), (2, 0), (1, 2), (3, 1), (2, 0)]
    cases.append(("64x64_edge", np.stack([g, g]), st, gl, 10, [calls, calls]))
    cases.append(("64x64_edge_T", np.stack([g.T, g.T]), st[..., ::-1].copy(), gl[..., ::-1].copy(), 10,
                  [[(a, {0: 0, 1: 2, 2: 1, 4: 3}[c]) for a, c in calls]] * 2))
    # 3 x 130 and its transpose: a wall with doors at its two ends, the sitter in one;
    # world 0: detour 258 (blocked); world 1: the walker is already past the door
    g = np.zeros((3, 130), dtype=np.int8)
    g[1, 1:129] = -1
    st = np.array([[(0, 0), (1, 0), (2, 64)], [(2, 1), (1, 0), (0, 70)]], np.int32)
    gl = np.array([[(2, 0), (1, 0), (0, 64)], [(2, 129), (1, 0), (2, 70)]], np.int32)
    calls = [(2, 0), (1, 1), (2, 0), (1, 3), (3, 1), (2, 0)]
    cases.append(("3x130", np.stack([g, g]), st, gl, 10, [calls, calls]))
    cases.append(("130x3", np.stack([g.T, g.T]), st[..., ::-1].copy(), gl[..., ::-1].copy(), 10,
                  [[(a, {0: 0, 1: 2, 3: 4}[c]) for a, c in calls]] * 2))
    # 70 x 20 rooms, 20 agents, 10 of them in doors
    rng = np.random.default_rng(7023)
    gs, sts, gls, cl = [], [], [], []
    for e in range(6):
        gr, s0, g0, da = rooms_world(rng, 70, 20, 20, 10)
        gs.append(gr), sts.append(s0), gls.append(g0), cl.append(rooms_script(rng, 20, da, 3))
    cases.append(("70x20", np.stack(gs), np.array(sts, np.int32), np.array(gls, np.int32), 9, cl))
    # 128 x 128 serpentine, E = 2: paths of thousands of levels; world 1 has a by-pass of
    # detour 12 around the sitter (two gaps in the wall above its lane)
    g0 = _serpentine(128)
    g1 = g0.copy()
    g1[63, 50] = g1[63, 61] = 0
    st = np.array([[(64, 54), (64, 56), (0, 0)], [(64, 54), (64, 56), (0, 0)]], np.int32)
    gl = np.array([[(126, 3), (64, 56), (0, 9)], [(126, 3), (64, 56), (0, 9)]], np.int32)
    calls = [(2, 0), (1, 3), (2, 0), (3, 1), (2, 0)]
    cases.append(("serpentine128", np.stack([g0, g1]), st, gl, 10, [calls, calls]))
    return cases


@pytest.mark.parametrize("case", _wide_shapes(), ids=lambda c: c[0])
def test_blocking_wide_shapes_match_restatement(mapfx_mod, case):
    name, grids, starts, goals, s, calls = case
    ids = np.array([[c[0] for c in cl] for cl in calls], np.int32)
    acts = np.array([[c[1] for c in cl] for cl in calls], np.int32)
    cnt, _ = _check_batch(mapfx_mod, grids, starts, goals, s, False, ids, acts)
    assert (cnt > 0).any()
    if name == "serpentine128":  # world 1's by-pass: detour 12 from (64, 54), 10 one cell further west
        assert cnt[:, 0].tolist() == [1, 1] and cnt[:, 2].tolist() == [1, 0]
    # and the count entry point on the initial states, every agent
    E, N = starts.shape[:2]
    b = mapfx_mod.PrimalBatch(starts, goals, grids=grids, observation_size=s)
    for a in range(N):
        got = _np(b.blocking_count(np.full(E, a + 1, np.int32)))
        want = [BlockingWorld(grids[e], starts[e], goals[e], size=s).blocking_count(a) for e in range(E)]
        assert got.tolist() == want, a


# ---- 6. errors ----
def test_blocking_null_valid_is_einval(mapfx_mod):
    from mapfx import lib
    from mapfx._abi import ptr
    g = np.zeros((4, 4), np.int8)
    b = mapfx_mod.PrimalBatch([[[0, 0], [1, 1]]], [[[3, 3], [1, 1]]], grids=g, blocking=True)
    o = b.act([[2, 1]], [[0, 1]])
    ids = torch.tensor([[2, 1]], dtype=torch.int32, device=b.device)
    acts = torch.tensor([[0, 1]], dtype=torch.int32, device=b.device)
    stream = torch.cuda.current_stream().cuda_stream
    for valid, on_goal in ((None, o["on_goal"]), (o["valid"], None)):
        rc = lib.mapfx_primal_blocking(b._h, ctypes.byref(b._state), ptr(ids), ptr(acts), 2, ptr(valid),
                                       ptr(on_goal), ptr(o["reward"]), ptr(o["blocking"]),
                                       ptr(o["n_blocking"]), stream)
        assert rc == -1 and b"valid" in lib.mapfx_last_error()
    rc = lib.mapfx_primal_blocking(None, ctypes.byref(b._state), ptr(ids), ptr(acts), 2, ptr(o["valid"]),
                                   ptr(o["on_goal"]), None, None, None, stream)
    assert rc == -1 and b"handle" in lib.mapfx_last_error()
    rc = lib.mapfx_primal_blocking_count(b._h, None, ptr(ids), ptr(o["n_blocking"]), stream)
    assert rc == -1 and b"state" in lib.mapfx_last_error()


def test_blocking_stops_at_a_bad_call(mapfx_mod):
    """World 1 is given agent id N + 1 at call 3 of 8: its calls 3 .. 7 are not executed --
    reward untouched, blocking and n_blocking 0, although their stale valid / on_goal bytes
    and actions look like stays on a goal -- and its neighbours are computed as usual."""
    g = np.zeros((3, 7), dtype=np.int8)
    g[1, 1:6] = -1
    starts = np.repeat(np.array([[(0, 0), (1, 0)]], np.int32), 3, axis=0)
    goals = np.repeat(np.array([[(2, 0), (1, 0)]], np.int32), 3, axis=0)
    grids = np.stack([g] * 3)
    ids = np.tile(np.array([2, 1, 2, 2, 2, 1, 2, 2], np.int32), (3, 1))
    acts = np.tile(np.array([0, 1, 0, 0, 0, 3, 0, 0], np.int32), (3, 1))
    good_ids = ids.copy()
    ids[1, 3] = 3
    b = mapfx_mod.PrimalBatch(starts, goals, grids=grids, observation_size=10, blocking=True)
    b._alloc(8)
    b.out["reward"].fill_(7.0)
    b.out["valid"].fill_(1)
    b.out["on_goal"].fill_(1)
    b.out["blocking"].fill_(9)
    b.out["n_blocking"].fill_(9)
    o = b.act(ids, acts)
    with pytest.raises(AssertionError):
        b.check_err()
    rew, blk, cnt, ong, val, pos = _restate(grids, starts, goals, 10, False, good_ids, acts)
    assert cnt[0].tolist() == [1, 0, 0, 0, 0, 0, 1, 1]  # (the walker steps away and back)
    for e in (0, 2):
        assert np.array_equal(_bits(_np(o["reward"])[e]), _bits(rew[e]))
        assert np.array_equal(_np(o["n_blocking"])[e], cnt[e]) and np.array_equal(_np(o["blocking"])[e], blk[e])
        assert np.array_equal(_np(b.pos)[e], pos[e])
    assert np.array_equal(_bits(_np(o["reward"])[1, :3]), _bits(rew[1, :3]))
    assert np.array_equal(_np(o["n_blocking"])[1, :3], cnt[1, :3])
    assert (_np(o["reward"])[1, 3:] == 7.0).all()
    assert (_np(o["n_blocking"])[1, 3:] == 0).all() and (_np(o["blocking"])[1, 3:] == 0).all()
    assert _np(b.pos)[1].tolist() == [[0, 1], [1, 0]]  # as call 2 left it


# ---- the single-world drop-in ----
@pytest.mark.parametrize("name", ["pb_door7_undo", "pb_diag_door7"])
def test_dropin_returns_the_blocking_flag(mapfx_mod, name):
    from mapfx.primal import MAPFEnv
    fx = _load(name)
    world = fx["grid"].astype(np.int64)
    gg = np.zeros_like(world)
    for a, ((r, c), (gr, gc)) in enumerate(zip(fx["starts"], fx["goals"])):
        world[r, c] = a + 1
        gg[gr, gc] = a + 1
    kw = dict(num_agents=len(fx["starts"]), observation_size=int(fx["size"]), world0=world, goals0=gg,
              DIAGONAL_MOVEMENT=bool(fx["diagonal"]))
    env, plain = MAPFEnv(blocking=True, **kw), MAPFEnv(**kw)
    assert env._reset(1, world0=world, goals0=gg)[2] is False
    for k in range(len(fx["agent"])):
        call = (int(fx["agent"][k]), int(fx["action"][k]))
        if call[1] == 0 and fx["on_goal"][k]:  # the query, on the world the stay will see
            for e in (env, plain):
                x = e.get_blocking_reward(call[0])
                assert np.float64(x).view(np.uint64) == np.float64(fx["n_blocking"][k] * -1.0).view(np.uint64)
        _, r, done, nxt, on_goal, blocking, valid = env._step(call)
        assert np.float64(r).view(np.uint64) == fx["reward"][k].view(np.uint64)
        assert blocking is bool(fx["blocking"][k]) and valid == bool(fx["valid"][k])
        assert done == bool(fx["done"][k]) and on_goal == bool(fx["on_goal"][k])
        assert sum(1 << a for a in nxt) == int(fx["next_mask"][k])
        assert plain._step(call)[5] is False
        assert env.getPositions() == [tuple(p) for p in fx["pos"][k].tolist()]
