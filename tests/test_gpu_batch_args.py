"""The batches' shared base on the device (mapfx._base.DeviceBatch): env masks are
checked before anything is launched and mean `!= 0` at every entry point,
PrimalBatch.__init__ and PrimalBatch.random build the same batch, and
MarlPartialBatch.rollout reuses its trajectory buffers.  E = 3, N = 2, an empty 8 x 8 grid."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E, N, H, W = 3, 2, 8, 8
STARTS = np.array([[[e, 0], [e, 2]] for e in range(E)], dtype=np.int32)
GOALS = np.array([[[7, 7 - e], [5, e]] for e in range(E)], dtype=np.int32)
GRID = np.zeros((H, W), dtype=np.int8)
# one scen file of 4 lines (start row, start col, goal row, goal col): more than N
SCEN = np.array([[[1, 1, 6, 6], [2, 3, 0, 7], [4, 4, 3, 0], [7, 1, 1, 5]]], dtype=np.int16)
MOVES = np.array([[1, 3]] * E, dtype=np.int8)          # every agent leaves its start
# the same envs three ways: only uint8 was read as intended before the shared env_mask
MASKS = {"uint8": torch.tensor([0, 1, 1], dtype=torch.uint8),
         "bool": torch.tensor([False, True, True]),
         "int64": torch.tensor([0, 256, 1], dtype=torch.int64)}


@pytest.fixture(scope="module")
def mapfx_mod():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mapfx
    return mapfx


def _grid_batch(m):
    b = m.MapfGridBatch(STARTS, GOALS, grids=GRID, episode_limit=50, device="cuda:0")
    b.reset()
    b.step(torch.from_numpy(MOVES).cuda())
    return b


def _partial_batch(m):
    b = m.MarlPartialBatch(STARTS, GOALS, grids=GRID, device="cuda:0")
    b.set_scenarios(SCEN, np.array([4], dtype=np.int32), seed=3)
    b.reset()
    b.step(torch.from_numpy(MOVES).cuda())
    return b


def _primal_batch(m):
    return m.PrimalBatch(STARTS, GOALS, grids=GRID, device="cuda:0")


def _state(b, names):
    torch.cuda.synchronize()
    return {k: getattr(b, k).cpu().numpy().copy() for k in names}


GRID_STATE = ("pos", "done", "t", "steps")
PARTIAL_STATE = ("pos", "init_pos", "goal", "goal_dist", "t", "terminated", "steps", "episode")
PRIMAL_STATE = ("pos", "goal", "bits", "episode")

ENTRY_POINTS = {
    "grid.reset": (_grid_batch, GRID_STATE, lambda b, m: b.reset(m)),
    "partial.reset": (_partial_batch, PARTIAL_STATE, lambda b, m: b.reset(m)),
    "partial.compute_goal_dist": (_partial_batch, PARTIAL_STATE,
                                  lambda b, m: b.compute_goal_dist(m)),
    "partial.redraw": (_partial_batch, PARTIAL_STATE, lambda b, m: b.redraw(m)),
    "primal.regenerate": (_primal_batch, PRIMAL_STATE,
                          lambda b, m: b.regenerate(m, keep_map=True)),
}


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_short_mask_is_refused_before_any_launch(mapfx_mod, name):
    make, names, call = ENTRY_POINTS[name]
    b = make(mapfx_mod)
    before = _state(b, names)
    for dt in (torch.uint8, torch.bool, torch.int64):
        with pytest.raises(AssertionError, match=r"mask must be \[E\]"):
            call(b, torch.ones(E - 1, dtype=dt, device="cuda:0"))
    after = _state(b, names)
    for k in names:
        assert before[k].tobytes() == after[k].tobytes(), k
    b.check_err()


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_masks_mean_nonzero(mapfx_mod, name):
    make, names, call = ENTRY_POINTS[name]
    got = {}
    for kind, mask in MASKS.items():
        b = make(mapfx_mod)
        before = _state(b, names)
        call(b, mask.cuda())
        got[kind] = _state(b, names)
        b.check_err()
    for kind in ("bool", "int64"):
        for k in names:
            assert got[kind][k].tobytes() == got["uint8"][k].tobytes(), (kind, k)
    # and the uint8 mask did what a mask does: env 0 as it was, envs 1 and 2 not
    changed = {"grid.reset": "pos", "partial.reset": "pos", "partial.redraw": "episode",
               "primal.regenerate": "episode"}.get(name)
    if changed is not None:
        b0, a0 = before[changed], got["uint8"][changed]
        assert np.array_equal(a0[0], b0[0])
        assert not np.array_equal(a0[1], b0[1]) and not np.array_equal(a0[2], b0[2])


@pytest.mark.parametrize("diagonal", [False, True])
def test_primal_init_and_random_build_the_same_batch(mapfx_mod, diagonal):
    # one map per world, as the generator makes them (a 2-d grid would be a shared map)
    a = mapfx_mod.PrimalBatch(STARTS, GOALS, grids=np.tile(GRID[None], (E, 1, 1)),
                              device="cuda:0", diagonal=diagonal, blocking=True)
    luts = (np.array([H], dtype=np.int32), np.array([0], dtype=np.uint32))
    r = mapfx_mod.PrimalBatch.random(E, N, (H, W), seed=5, luts=luts, device="cuda:0",
                                     diagonal=diagonal, blocking=True)
    for k in ("E", "N", "H", "W", "s", "n_actions", "map_shared", "diagonal", "blocking"):
        assert getattr(a, k) == getattr(r, k), k
    for k in ("pos", "goal", "bits", "past", "err", "episode"):
        x, y = getattr(a, k), getattr(r, k)
        assert (x is None) == (y is None), k
        if x is not None:
            assert x.shape == y.shape and x.dtype == y.dtype and x.device == y.device, k
    for k in ("pos", "goal", "bits") + (("past",) if diagonal else ()):
        getattr(r, k).copy_(getattr(a, k))
    ids = torch.tensor([[1, 2]] * E, dtype=torch.int32)
    acts = torch.tensor([[1, 3], [2, 0], [4, 1]], dtype=torch.int32)
    oa, orr = a.act(ids, acts), r.act(ids, acts)
    qa, qr = a.observe(), r.observe()
    torch.cuda.synchronize()
    for got, want in ((orr, oa), (qr, qa)):
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
    assert oa["valid"].cpu().numpy().any()          # the calls did move agents
    a.check_err()
    r.check_err()


def test_partial_rollout_reuses_its_buffers(mapfx_mod):
    b = mapfx_mod.MarlPartialBatch(STARTS, GOALS, grids=GRID, device="cuda:0")
    assert vars(b)["_traj_cache"] == {}
    b.reset()
    acts = torch.from_numpy(np.stack([MOVES, MOVES])).cuda()
    first = b.rollout(acts, obs=False)
    again = b.rollout(acts, obs=False)
    assert again is first and list(b._traj_cache) == [(2, False, False)]
    assert all(again[k] is first[k] for k in first)
    other = b.rollout(acts, obs=True)
    assert other is not first and "obs" in other and "obs" not in first
    assert b.rollout(acts, obs=True) is other and len(b._traj_cache) == 2
    b.check_err()
