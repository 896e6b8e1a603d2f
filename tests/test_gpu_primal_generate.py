"""GPU parity of the device world generator (mapfx_primal_generate, include/mapfx_primal.h;
PrimalBatch.random / regenerate) with its plain restatement tests/primal_gen_ref.py:
map_bits, pos, goal, past and episode bit-exactly, the kernel named by mapfx_last_kernel,
and the worlds it draws played through act / observe against the reference-pinned
restatement of the dynamics on the cropped side x side grid."""
import ctypes

import numpy as np
import pytest
import torch

import primal_gen_ref as ref

pytestmark = pytest.mark.gpu

KERNEL = "primal_generate_kernel"
HALF = 1 << 31


@pytest.fixture(scope="module")
def mapfx_mod():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mapfx
    return mapfx


def _np(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def _dev_state(b):
    return {"bits": _np(b.bits), "pos": _np(b.pos), "goal": _np(b.goal), "past": _np(b.past),
            "episode": _np(b.episode)}


def _zero_state(E, N, H, W, diag):
    return {"bits": np.zeros((E, ref.stride(H, W)), dtype=np.uint8),
            "pos": np.zeros((E, N, 2), dtype=np.int32), "goal": np.zeros((E, N, 2), dtype=np.int32),
            "past": np.zeros((E, N, 2), dtype=np.int32) if diag else None,
            "episode": np.zeros(E, dtype=np.int32)}


def _same(got, want):
    for k in ("bits", "pos", "goal", "past", "episode"):
        if want[k] is None:
            assert got[k] is None
        else:
            assert np.array_equal(got[k], want[k]), k


def _luts(sides, probs):
    return np.array(sides, dtype=np.int32), np.array(probs, dtype=np.uint32)


def _last_kernel():
    from mapfx import _abi
    return _abi.last_kernel()


# E, N, (H, W), side table, density table, diagonal
CORNERS = {
    "side1_start_is_goal": (3, 1, (4, 5), [1], [HALF], False),
    "side64_full_width": (3, 8, (64, 64), [64], [int(.3 * 2 ** 32)], True),
    "13x7_rows_straddle_dwords": (130, 4, (13, 7), [5, 6, 7, 7], [0, HALF // 2, HALF, 3 * (HALF // 2)], True),
    "n255_on_16x16": (1, 255, (16, 16), [16], [0], False),
    "redraws_n60_side8": (3, 60, (8, 8), [8], [0xF0000000], True),
    "side40_in_40x40": (3, 16, (40, 40), [10, 10, 25, 40], [0, HALF // 2, HALF // 2, HALF], False),
}


@pytest.mark.parametrize("name", sorted(CORNERS))
def test_corner_cases(mapfx_mod, name):
    E, N, (H, W), sides, probs, diag = CORNERS[name]
    luts = _luts(sides, probs)
    b = mapfx_mod.PrimalBatch.random(E, N, (H, W), seed=0xABCDEF + E, luts=luts, diagonal=diag,
                                     env_offset=17)
    assert KERNEL in _last_kernel()
    b.check_err()
    want = _zero_state(E, N, H, W, diag)
    assert ref.generate(want, 0xABCDEF + E, 17, N, H, W, luts) == []
    got = _dev_state(b)
    _same(got, want)
    assert (got["episode"] == 1).all()
    if name == "side1_start_is_goal":
        assert (got["pos"] == 0).all() and (got["goal"] == 0).all()
    if name == "redraws_n60_side8":
        assert all(ref.world(0xABCDEF + E, 17 + e, 0, N, H, W, *luts)["attempts"] > 0 for e in range(E))
    if name == "n255_on_16x16":
        assert len({(int(r), int(c)) for r, c in got["pos"][0]}) == 255
        assert len({(int(r), int(c)) for r, c in got["goal"][0]}) == 255


def _patterned(mapfx_mod, E, N, H, W, luts, seed, diag=True):
    """A generated batch whose whole state is then overwritten, in place, with a pattern."""
    b = mapfx_mod.PrimalBatch.random(E, N, (H, W), seed=seed, luts=luts, diagonal=diag)
    b.bits.fill_(0xA5)
    b.pos.copy_(torch.arange(E * N * 2, dtype=torch.int32).reshape(E, N, 2) % 5)
    b.goal.fill_(3)
    b.past.fill_(2)
    b.episode.copy_(torch.arange(E, dtype=torch.int32) * 3 + 4)
    return b


def test_masked_reset(mapfx_mod):
    E, N, H, W, seed = 12, 4, 16, 16, 31337
    luts = _luts([5, 6, 7, 8, 9, 10, 11, 12], [0, HALF // 2, HALF, HALF // 4])
    mask = np.zeros(E, dtype=bool)
    mask[[0, 3, 4, 11]] = True
    for m in (torch.from_numpy(mask).cuda(), torch.from_numpy(mask.astype(np.uint8)).cuda(),
              torch.from_numpy(mask.astype(np.int64) * 7).cuda()):
        b = _patterned(mapfx_mod, E, N, H, W, luts, seed)
        before = _dev_state(b)
        want = {k: v.copy() for k, v in before.items()}
        b.regenerate(mask=m)
        assert KERNEL in _last_kernel()
        b.check_err()
        first = _dev_state(b)
        assert ref.generate(want, seed, 0, N, H, W, luts, mask=mask) == []
        _same(first, want)
        for k in before:  # untouched worlds byte for byte, touched worlds one episode on
            assert np.array_equal(first[k][~mask], before[k][~mask]), k
        assert np.array_equal(first["episode"][mask], before["episode"][mask] + 1)
        b.regenerate(mask=m)
        second = _dev_state(b)
        ref.generate(want, seed, 0, N, H, W, luts, mask=mask)
        _same(second, want)
        assert np.array_equal(second["episode"][mask], before["episode"][mask] + 2)
        for e in np.flatnonzero(mask):
            assert not (np.array_equal(second["pos"][e], first["pos"][e])
                        and np.array_equal(second["bits"][e], first["bits"][e])), e


def test_reset_on_done_mask(mapfx_mod):
    """out["done"][:, -1] as the mask: the one-cell worlds are done after a stay."""
    E, N, H, W, seed = 40, 1, 8, 8, 5
    luts = _luts([1, 1, 3, 4], [0, HALF])
    b = mapfx_mod.PrimalBatch.random(E, N, (H, W), seed=seed, luts=luts)
    want = _zero_state(E, N, H, W, False)
    ref.generate(want, seed, 0, N, H, W, luts)
    out = b.act(np.ones((E, 2), dtype=np.int32), np.zeros((E, 2), dtype=np.int32))
    b.regenerate(mask=out["done"][:, -1])
    done = _np(out["done"])[:, -1].astype(bool)
    assert np.array_equal(done, (want["pos"] == want["goal"]).all((1, 2))) and 5 < done.sum() < E
    ref.generate(want, seed, 0, N, H, W, luts, mask=done)
    _same(_dev_state(b), want)
    b.check_err()


def _serpentine(n=64):
    g = np.zeros((n, n), dtype=np.int8)
    for r in range(1, n, 2):
        g[r, :] = -1
        g[r, n - 1 if r % 4 == 1 else 0] = 0
    return g


def _row_major_free(grid, n):
    cells = np.argwhere(grid == 0)[:n]
    return cells.astype(np.int32)


def _two_region():
    g = np.zeros((6, 6), dtype=np.int8)
    g[:, 3] = -1
    return g


@pytest.mark.parametrize("case", ["serpentine", "two_region", "shared"])
def test_keep_map(mapfx_mod, case):
    if case == "serpentine":   # one region, a flood of about two thousand levels
        grid, E, N, shared = _serpentine(), 2, 4, False
    elif case == "two_region":
        grid, E, N, shared = _two_region(), 5, 2, False
    else:
        grid, E, N, shared = _serpentine(16), 4, 3, True
    H, W = grid.shape
    st = np.tile(_row_major_free(grid, N)[None], (E, 1, 1))
    grids = grid[None] if shared else np.tile(grid[None], (E, 1, 1))
    b = mapfx_mod.PrimalBatch(st, st, grids=grids, diagonal=True)
    assert b.map_shared == shared
    b.gen_seed, b.env_offset = 77, 3
    before = _dev_state(b)
    b.regenerate(keep_map=True)
    assert KERNEL in _last_kernel()
    b.check_err()
    want = {k: v.copy() for k, v in before.items()}
    assert ref.generate(want, 77, 3, N, H, W, keep_map=True) == []
    got = _dev_state(b)
    _same(got, want)
    assert np.array_equal(got["bits"], before["bits"]) and (got["episode"] == 1).all()
    if case == "two_region":
        assert ((got["pos"][..., 1] > 3) == (got["goal"][..., 1] > 3)).all()
    # the masked form on the same batch
    m = np.arange(E) % 2 == 0
    b.regenerate(mask=torch.from_numpy(m).cuda(), keep_map=True)
    ref.generate(want, 77, 3, N, H, W, mask=m, keep_map=True)
    _same(_dev_state(b), want)


def test_keep_map_too_few_free_cells(mapfx_mod):
    grid, E, N = _two_region(), 3, 2
    st = np.tile(_row_major_free(grid, N)[None], (E, 1, 1))
    b = mapfx_mod.PrimalBatch(st, st, grids=np.tile(grid[None], (E, 1, 1)))
    full = np.ones((6, 6), dtype=bool)
    full[2, 2] = False                                   # world 1: one free cell for two agents
    b.bits[1].copy_(torch.from_numpy(ref.pack(full)))
    before = _dev_state(b)
    b.regenerate(keep_map=True)
    with pytest.raises(AssertionError, match="world 1"):
        b.check_err()
    want = {k: (None if v is None else v.copy()) for k, v in before.items()}
    assert ref.generate(want, 0, 0, N, 6, 6, keep_map=True) == [1]
    got = _dev_state(b)
    _same(got, want)
    for k in ("bits", "pos", "goal", "episode"):
        assert np.array_equal(got[k][1], before[k][1]), k
    assert got["episode"].tolist() == [1, 0, 1]


def test_refusals_without_a_launch(mapfx_mod):
    from mapfx import _abi
    from mapfx._abi import MapfxError, lib, ptr
    grid = _two_region()
    st = np.tile(_row_major_free(grid, 2)[None], (4, 1, 1))
    b = mapfx_mod.PrimalBatch(st, st, grids=grid[None])
    assert b.map_shared
    before = _dev_state(b)
    marker = _last_kernel()
    with pytest.raises(ValueError, match="keep_map"):
        b.regenerate()
    side, prob = torch.tensor([4, 4], dtype=torch.int32).cuda(), torch.zeros(2, dtype=torch.int32).cuda()

    def raw(batch, **kw):
        f = dict(seed=1, env_offset=0, side_lut=ptr(side), n_side=2, prob_lut=ptr(prob), n_prob=2,
                 episode=ptr(batch.episode), mask=None, map_bits=ptr(batch.bits), keep_map=0,
                 err=ptr(batch.err))
        f.update(kw)
        gen = _abi.QGen(**f)
        rc = lib.mapfx_primal_generate(batch._h, ctypes.byref(batch._state), ctypes.byref(gen), None)
        return rc, lib.mapfx_last_error().decode()

    rc, msg = raw(b)                                     # a shared-map handle without keep_map
    assert rc == -1 and "keep_map" in msg
    per_world = mapfx_mod.PrimalBatch(st, st, grids=np.tile(grid[None], (4, 1, 1)))
    rc, msg = raw(per_world, n_side=3)                   # a table length of 3
    assert rc == -1 and "powers of two" in msg
    rc, msg = raw(per_world, n_prob=0)
    assert rc == -1 and "powers of two" in msg
    assert lib.mapfx_primal_generate(None, ctypes.byref(b._state), None, None) == -1
    assert _last_kernel() == marker
    torch.cuda.synchronize()
    _same(_dev_state(b), before)
    with pytest.raises(MapfxError, match="powers of two"):
        mapfx_mod.PrimalBatch.random(2, 1, (8, 8), seed=1, luts=_luts([4, 4, 4], [0]))
    with pytest.raises(MapfxError, match="64"):          # a 65 x 8 handle
        mapfx_mod.PrimalBatch.random(2, 1, (65, 8), seed=1, SIZE=(4, 8))
    with pytest.raises(ValueError, match="side"):        # the reference's sides reach 40 > 16
        mapfx_mod.PrimalBatch.random(2, 1, (16, 16), seed=1)
    with pytest.raises(ValueError, match="side"):        # 3 x 3 cells for 10 agents
        mapfx_mod.PrimalBatch.random(2, 10, (16, 16), seed=1, luts=_luts([3], [0]))


def test_bad_side_from_a_device_table(mapfx_mod):
    """Tables already on the device are not read back: the kernel reports the world."""
    E, N, H, W, seed = 24, 2, 16, 16, 11
    sides, probs = [4, 20, 4, 4], [0, HALF]
    dev = (torch.tensor(sides, dtype=torch.int32).cuda(), torch.tensor(probs, dtype=torch.int64).to(torch.int32).cuda())
    b = mapfx_mod.PrimalBatch.random(E, N, (H, W), seed=seed, luts=dev)
    want = _zero_state(E, N, H, W, False)
    bad = ref.generate(want, seed, 0, N, H, W, _luts(sides, probs))
    assert 0 < len(bad) < E
    with pytest.raises(AssertionError) as ei:
        b.check_err()
    assert int(str(ei.value).rsplit("world ", 1)[1]) in bad
    got = _dev_state(b)
    _same(got, want)
    assert (got["episode"][bad] == 0).all() and not got["bits"][bad].any()


def test_shard_invariance(mapfx_mod):
    kw = dict(N=8, hw=(40, 40), seed=2024, diagonal=True)
    whole = _dev_state(mapfx_mod.PrimalBatch.random(64, env_offset=0, **kw))
    lo = _dev_state(mapfx_mod.PrimalBatch.random(32, env_offset=0, **kw))
    hi = _dev_state(mapfx_mod.PrimalBatch.random(32, env_offset=32, **kw))
    for k in whole:
        assert np.array_equal(whole[k], np.concatenate([lo[k], hi[k]])), k
    from mapfx.maps import primal_gen_luts
    want = _zero_state(64, 8, 40, 40, True)
    assert ref.generate(want, 2024, 0, 8, 40, 40, primal_gen_luts()) == []
    _same(whole, want)


def _check_calls(w, o, e, ids, acts):
    for k in range(ids.shape[1]):
        maps, vec, r, done, mask, on_goal, _, valid = w.step(int(ids[e, k]) - 1, int(acts[e, k]))
        assert np.float64(r).view(np.uint64) == o["reward"][e, k].view(np.uint64), (e, k)
        assert done == bool(o["done"][e, k]) and mask == int(o["next_mask"][e, k]), (e, k)
        assert on_goal == bool(o["on_goal"][e, k]) and valid == bool(o["valid"][e, k]), (e, k)
        assert np.array_equal(maps, o["obs"][e, k]), (e, k)
        assert np.array_equal(vec.view(np.uint64), o["vec"][e, k].view(np.uint64)), (e, k)


@pytest.mark.parametrize("diag", [False, True])
def test_embedded_world_plays_like_the_cropped_world(mapfx_mod, diag):
    """A side x side world in the corner of a 16 x 16 handle, the rest walls, against the
    dynamics restatement on the side x side grid alone: no output can tell them apart."""
    from oracle.mapf_oracle import primal_obs
    from oracle.primal_dyn_oracle import PrimalWorld
    E, N, H, W, s, seed = 16, 4, 16, 16, 10, 404
    luts = _luts([5, 6, 7, 8, 9, 10, 11, 12], [0, HALF // 4, HALF // 2, HALF // 2])
    b = mapfx_mod.PrimalBatch.random(E, N, (H, W), seed=seed, luts=luts, diagonal=diag, observation_size=s)
    st = _dev_state(b)
    rng = np.random.default_rng(12 + diag)
    worlds = []
    for e in range(E):
        side = ref.world(seed, e, 0, N, H, W, *luts)["side"]
        grid = -ref.unpack(st["bits"][e], H, W)[:side, :side].astype(np.int64)
        worlds.append(PrimalWorld(grid, st["pos"][e], st["goal"][e], s, diagonal=diag))
    assert len({w.h for w in worlds}) > 3
    nact = 9 if diag else 5
    for _ in range(2):
        ids = rng.integers(1, N + 1, size=(E, 20)).astype(np.int32)
        acts = rng.integers(0, nact, size=(E, 20)).astype(np.int32)
        o = {k: _np(v) for k, v in b.act(ids, acts).items()}
        prev = rng.integers(0, nact, size=(E, N)).astype(np.int32)
        q = {k: _np(v) for k, v in b.observe(None, prev).items()}
        b.check_err()
        for e, w in enumerate(worlds):
            _check_calls(w, o, e, ids, acts)
            for a in range(N):
                maps, vec = primal_obs(w._world_grid(), w.pos, w.goals, s, agents=[a])
                assert np.array_equal(maps[a], q["obs"][e, a]), (e, a)
                assert np.array_equal(vec[a].view(np.uint64), q["vec"][e, a].view(np.uint64)), (e, a)
                assert w.next_mask(a, int(prev[e, a])) == int(q["next_mask"][e, a]), (e, a)
                assert (w.pos[a] == w.goals[a]) == bool(q["on_goal"][e, a]), (e, a)
                assert w.done() == bool(q["done"][e, a]), (e, a)


def test_reset_on_done_loop_without_host_sync(mapfx_mod):
    from oracle.primal_dyn_oracle import PrimalWorld
    E, N, H, W, s, seed, K = 48, 1, 8, 8, 4, 8080, 6
    luts = _luts([1, 2, 2, 3], [0, HALF // 2])
    rng = np.random.default_rng(3)
    ids = np.ones((2, E, K), dtype=np.int32)
    acts = rng.integers(0, 5, size=(2, E, K)).astype(np.int32)
    d_ids, d_acts = torch.from_numpy(ids).cuda(), torch.from_numpy(acts).cuda()
    side = torch.from_numpy(luts[0]).cuda()
    prob = torch.from_numpy(luts[1].view(np.int32)).cuda()
    torch.zeros(1).cuda()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")   # a synchronising torch call raises from here on
    try:
        b = mapfx_mod.PrimalBatch.random(E, N, (H, W), seed=seed, luts=(side, prob), observation_size=s)
        o1 = {k: v.clone() for k, v in b.act(d_ids[0], d_acts[0]).items()}
        b.regenerate(mask=o1["done"][:, -1])
        o2 = b.act(d_ids[1], d_acts[1])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    o1 = {k: _np(v) for k, v in o1.items()}
    o2 = {k: _np(v) for k, v in o2.items()}
    b.check_err()
    want = _zero_state(E, N, H, W, False)
    ref.generate(want, seed, 0, N, H, W, luts)

    def play(o, rnd):
        done = np.zeros(E, dtype=bool)
        for e in range(E):
            w = PrimalWorld(-ref.unpack(want["bits"][e], H, W).astype(np.int64), want["pos"][e],
                            want["goal"][e], s)
            _check_calls(w, o, e, ids[rnd], acts[rnd])
            want["pos"][e] = np.array(w.pos)
            done[e] = w.done()
        return done

    done = play(o1, 0)
    assert 3 < done.sum() < E
    ref.generate(want, seed, 0, N, H, W, luts, mask=done)
    play(o2, 1)
    _same(_dev_state(b), want)
    assert np.array_equal(want["episode"], 1 + done)
