"""CPU checks of the device world generator's rules (include/mapfx_primal.h,
mapfx_primal_generate) on their plain restatement tests/primal_gen_ref.py, and of the
host tables mapfx.maps.primal_gen_luts.  The GPU tests (test_gpu_primal_generate.py)
compare the kernel bit-exactly with the same restatement."""
import numpy as np
import pytest

import primal_gen_ref as ref

HALF = 1 << 31  # thresh = .5 * 2^32


def _labels(free):
    """Connected components of the free cells by union-find (independent of ref.region)."""
    H, W = free.shape
    parent = list(range(H * W))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for r in range(H):
        for c in range(W):
            if not free[r, c]:
                continue
            if r + 1 < H and free[r + 1, c]:
                parent[find(r * W + c)] = find((r + 1) * W + c)
            if c + 1 < W and free[r, c + 1]:
                parent[find(r * W + c)] = find(r * W + c + 1)
    return find


def _check_world(w, N, H, W, side):
    obst, pos, goal = w["obst"], w["pos"], w["goal"]
    assert obst.shape == (H, W)
    outside = np.ones((H, W), dtype=bool)
    outside[:side, :side] = False
    assert obst[outside].all()                                   # everything outside side x side is a wall
    for arr in (pos, goal):
        assert (arr >= 0).all() and (arr < side).all()           # inside side x side
        assert len({(int(r), int(c)) for r, c in arr}) == N      # distinct
        assert not obst[arr[:, 0], arr[:, 1]].any()              # on free cells
    find = _labels(~obst)
    for a in range(N):
        assert find(int(pos[a, 0]) * W + int(pos[a, 1])) == find(int(goal[a, 0]) * W + int(goal[a, 1]))


def _cases():
    out = []
    for th in (0, HALF):
        out += [(1, s, th) for s in range(1, 65)]
        out += [(8, s, th) for s in range(3, 65, 2)]
        out += [(64, s, th) for s in (8, 9, 13, 40, 64)]
    # thresholds that leave fewer than N free cells at first: redraw attempts t > 0
    out += [(60, 8, 0xF0000000), (64, 8, 0xFFFFFFFF), (8, 3, 0xC0000000), (1, 1, 0xFFFFFFFF),
            (8, 4, 0xE0000000), (64, 9, 0xD0000000)]
    return out


def test_invariants():
    cases = _cases()
    assert len(cases) > 200
    redrawn = 0
    for i, (N, side, th) in enumerate(cases):
        H = W = 64 if i % 2 else side
        w = ref.world(0xC0FFEE, 1000 + i, i % 5, N, H, W, [side], [th])
        assert w is not None and w["side"] == side
        _check_world(w, N, H, W, side)
        if th == 0:
            assert not w["obst"][:side, :side].any() and w["attempts"] == 0
        redrawn += w["attempts"] > 0
    assert redrawn >= 5
    # bad worlds: a side outside the grid, fewer cells than agents, too few free cells (keep_map)
    assert ref.world(1, 0, 0, 1, 8, 8, [9], [0]) is None
    assert ref.world(1, 0, 0, 1, 8, 8, [0], [0]) is None
    assert ref.world(1, 0, 0, 10, 8, 8, [3], [0]) is None
    full = np.ones((4, 4), dtype=bool)
    full[0, 0] = False
    assert ref.world(1, 0, 0, 2, 4, 4, obstacles=full) is None
    assert ref.world(1, 0, 0, 1, 4, 4, obstacles=full) is not None


def test_stream_ids():
    from mapfx import maps, rng
    ids = (rng.STREAM_GEN_WORLD, rng.STREAM_GEN_OBST, rng.STREAM_GEN_START, rng.STREAM_GEN_GOAL)
    assert ids == (ref.WORLD, ref.OBST, ref.START, ref.GOAL)
    used = {maps.STREAM_OBST, maps.STREAM_START, maps.STREAM_GOAL}
    mine = {ids[0], ids[2], ids[3]} | {ids[1] + t for t in range(33)}
    assert len(mine) == 36 and not (mine & used)
    assert (int(rng.K_ENV), int(rng.K_T), int(rng.K_CELL), int(rng.K_STREAM)) == \
        (ref.K_ENV, ref.K_T, ref.K_CELL, ref.K_STREAM)
    x = np.array([0, 1, 0xDEADBEEF, ref.M64], dtype=np.uint64)
    assert [int(v) for v in rng.splitmix64(x)] == [ref.mix(int(v)) for v in x]


def test_luts_follow_the_reference_distribution():
    from mapfx.maps import primal_gen_luts
    side, prob = primal_gen_luts((10, 40), (0, .5))
    assert side.dtype == np.int32 and side.tolist() == [10, 10, 25, 40]
    assert prob.dtype == np.uint32 and prob.shape == (256,)
    q = prob.astype(np.float64) / 2.0 ** 32
    assert (np.diff(q) >= 0).all() and q.min() >= 0 and q.max() <= .5
    mode = .33 * 0 + .66 * .5
    # mid-point quantiles of the triangular density at n_prob = 256: the mean is off by 1.7e-6
    assert abs(q.mean() - (0 + mode + .5) / 3) < 1e-3
    # the quantiles invert the triangular CDF
    u = (np.arange(256) + .5) / 256
    cdf = np.where(q < mode, q * q / (.5 * mode), 1 - (.5 - q) ** 2 / (.5 * (.5 - mode)))
    assert np.abs(cdf - u).max() < 1e-6
    s2, p2 = primal_gen_luts((8, 8), (.2, .2), n_prob=4)
    assert s2.tolist() == [8, 8, 8, 8] and p2.tolist() == [int(.2 * 2 ** 32)] * 4
    with pytest.raises(ValueError):
        primal_gen_luts(n_prob=3)


def two_region_world():
    """6 x 6, a wall down column 3: an 18-cell region on the left, 12 cells on the right."""
    obst = np.zeros((6, 6), dtype=bool)
    obst[:, 3] = True
    return obst


def test_starts_and_goals_are_uniform():
    obst = two_region_world()
    free = ~obst
    nfree = int(free.sum())
    episodes, N = 20000, 2
    starts = np.zeros((N, 6, 6), dtype=np.int64)
    goals = np.zeros((N, 2, 6, 6), dtype=np.int64)   # [agent][region of its start]
    for ep in range(episodes):
        w = ref.world(0x5EED, 7, ep, N, 6, 6, obstacles=obst)
        for a in range(N):
            r, c = w["pos"][a]
            starts[a, r, c] += 1
            goals[a, int(c > 3), w["goal"][a, 0], w["goal"][a, 1]] += 1
    for a in range(N):
        assert starts[a][obst].sum() == 0 and starts[a].sum() == episodes
        p = 1.0 / nfree
        sd = (episodes * p * (1 - p)) ** .5
        assert np.abs(starts[a][free] - episodes * p).max() <= 5 * sd, (a, starts[a])
        for side_, cols in ((0, slice(0, 3)), (1, slice(4, 6))):
            cnt = goals[a, side_]
            n = int(cnt.sum())
            cells = np.zeros((6, 6), dtype=bool)
            cells[:, cols] = True
            assert cnt[~cells].sum() == 0 and n > 5000          # goals never leave the start's region
            p = 1.0 / int(cells.sum())
            sd = (n * p * (1 - p)) ** .5
            assert np.abs(cnt[cells] - n * p).max() <= 5 * sd, (a, side_, cnt)


def _state(E, N, H, W, diag=True):
    return {"bits": np.zeros((E, ref.stride(H, W)), dtype=np.uint8),
            "pos": np.zeros((E, N, 2), dtype=np.int32), "goal": np.zeros((E, N, 2), dtype=np.int32),
            "past": np.zeros((E, N, 2), dtype=np.int32) if diag else None,
            "episode": np.zeros(E, dtype=np.int32)}


def test_world_is_independent_of_sharding_and_grid():
    from mapfx.maps import primal_gen_luts
    luts = primal_gen_luts((10, 40), (0, .5))
    N, seed = 8, 99
    whole = _state(64, N, 40, 40)
    assert ref.generate(whole, seed, 0, N, 40, 40, luts) == []
    lo, hi = _state(32, N, 40, 40), _state(32, N, 40, 40)
    ref.generate(lo, seed, 0, N, 40, 40, luts)
    ref.generate(hi, seed, 32, N, 40, 40, luts)
    for k in ("bits", "pos", "goal", "past", "episode"):
        assert np.array_equal(whole[k], np.concatenate([lo[k], hi[k]])), k
    assert (whole["episode"] == 1).all() and np.array_equal(whole["past"], whole["pos"])
    big = _state(64, N, 64, 64)
    ref.generate(big, seed, 0, N, 64, 64, luts)
    assert np.array_equal(big["pos"], whole["pos"]) and np.array_equal(big["goal"], whole["goal"])
    sides = set()
    for e in range(64):
        a, b = ref.unpack(whole["bits"][e], 40, 40), ref.unpack(big["bits"][e], 64, 64)
        assert np.array_equal(a, b[:40, :40]) and b[40:].all() and b[:, 40:].all()
        sides.add(int((~a).any(1).nonzero()[0].max()) + 1)
    assert sides <= {10, 25, 40} and len(sides) == 3
    # a second episode of the same worlds is another draw
    again = {k: (None if v is None else v.copy()) for k, v in whole.items()}
    ref.generate(again, seed, 0, N, 40, 40, luts)
    assert (again["episode"] == 2).all() and not np.array_equal(again["pos"], whole["pos"])
    # a masked-out world is untouched
    m = np.zeros(64, dtype=bool)
    m[5] = True
    third = {k: (None if v is None else v.copy()) for k, v in again.items()}
    ref.generate(third, seed, 0, N, 40, 40, luts, mask=m)
    for k in ("bits", "pos", "goal", "past", "episode"):
        assert np.array_equal(np.delete(third[k], 5, 0), np.delete(again[k], 5, 0)), k
    assert third["episode"][5] == 3
