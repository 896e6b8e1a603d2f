"""The split rollout's store path (mapfx.hip, split_store_wave_dbm): the window records leave
the two store waves as write-through 16-byte stores through a buffer resource, the per-agent
outputs (positions, node, edge, avail, done) as write-through stores of 8 or 1 bytes per
lane, while reward, t and term stay plain stores.

Every case runs the split instance (asserted through `_abi.last_kernel()`) into output
buffers that are 16-byte-aligned views inside larger allocations, 256 sentinel bytes either
side, and compares every output of every step and the final state bit for bit against the
C oracle (rewards as u64 patterns); after the launch every sentinel byte is intact.  The
guard cases pass a leading slice traj[:t] of buffers with more rows: the rows behind it
stay untouched as well.

Shapes as in test_gpu_rollout_action_staging.py: N = 16 on 12x12 maps with 20 % obstacles,
E = 4 (one workgroup) and 36 (several, across the XCD renumbering); N = 64 on 16x16 maps,
E = 1 and 9."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P_OBST = 0.2
GUARD = 256
LEAD = GUARD + 16          # the view starts 16-byte aligned, not 256-byte aligned
SENTINEL = 0xA5
OUTS = ("reward", "term", "node", "edge", "avail", "obs_window", "traj_pos", "traj_done", "traj_t")
SHAPES = {16: (12, 41), 64: (16, 43)}      # agents per env -> (map side, instance seed)


@pytest.fixture(scope="module")
def mapfx_mod():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mapfx
    return mapfx


def _u64(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _np(t):
    return t.detach().cpu().numpy()


_INST = {}


def _inst(E, n):
    from mapfx.maps import synthetic_instances
    s, seed = SHAPES[n]
    if (E, n) not in _INST:
        _INST[(E, n)] = synthetic_instances(E, s, s, n, p_obstacle=P_OBST, seed=seed)
    return _INST[(E, n)]


def _guarded(b, rows, outs):
    """{name: (raw uint8 allocation, [rows, ...] view at byte LEAD of it)}, all SENTINEL."""
    bufs = {}
    for name, (shape, dt) in b.out_spec(rows).items():
        if name not in outs:
            continue
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
        raw = torch.full((LEAD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=b.device)
        view = raw[LEAD:LEAD + nbytes].view(dt).view(shape)
        assert view.data_ptr() % 16 == 0 and view.data_ptr() % 256 != 0
        bufs[name] = (raw, view)
    return bufs


def _run(mapfx_mod, E, n, T, win, occ=False, autoreset=False, limit=2000, spare_rows=0):
    """One launch of T steps into guarded buffers of T + spare_rows rows; returns nothing,
    asserts everything."""
    from mapfx import _abi
    from mapfx.batch import window_planes
    from oracle import corc
    s, _ = SHAPES[n]
    inst = _inst(E, n)
    b = mapfx_mod.MapfGridBatch(inst["init_pos"], inst["goals"], bits=inst["bits"], hw=(s, s),
                                episode_limit=limit, obs=("window_occ",) if occ else ("window",),
                                window=win)
    b.reset()
    outs = tuple("obs_window_occ" if (occ and k == "obs_window") else k for k in OUTS)
    acts_np = np.random.RandomState(7 + 131 * T + E).randint(0, 5, size=(T, E, n)).astype(np.int8)
    bufs = _guarded(b, T + spare_rows, outs)
    traj = {k: v[:T] for k, (_, v) in bufs.items()}
    b.rollout(T, actions=torch.from_numpy(acts_np).cuda(), autoreset=autoreset, traj=traj, outputs=outs)
    want = "mapf_wave_kernel<%d, true, true, true, %d, true, %s, %d>" % (
        win, n, "true" if occ else "false", 8 if T <= 32 else 0)
    assert want in _abi.last_kernel(), _abi.last_kernel()
    torch.cuda.synchronize()
    b.check_err()

    # guard bytes, and the rows behind the launch's last
    for k, (raw, view) in bufs.items():
        r = _np(raw)
        used = T * (view[0].numel() * view.element_size())
        assert (r[:LEAD] == SENTINEL).all(), "%s: bytes before the buffer" % k
        tail = r[LEAD + used:]
        bad = np.flatnonzero(tail != SENTINEL)
        assert bad.size == 0, "%s: byte %d behind row %d written" % (k, bad[0], T)

    # every step against the oracle
    tr = {k: _np(v) for k, v in traj.items()}
    if occ:
        tr["obs_window"] = _np(window_planes(traj["obs_window_occ"]))
    ob = corc.OracleBatch(inst["bits"], inst["init_pos"], inst["goals"], s, s, limit=limit, nthreads=2)
    resets = 0
    for k in range(T):
        r = ob.step(acts_np[k].astype(np.int32))
        o = ob.observe(window=win, full=False)
        assert np.array_equal(_u64(tr["reward"][k]), _u64(r["reward"])), k
        assert np.array_equal(tr["node"][k], r["node"]), k
        assert np.array_equal(tr["edge"][k], r["edge"]), k
        assert np.array_equal(tr["avail"][k], o["avail"]), k
        assert np.array_equal(tr["term"][k], o["term"]), k
        assert np.array_equal(tr["obs_window"][k], o["obs_window"]), k
        assert np.array_equal(tr["traj_pos"][k], ob.pos), k
        assert np.array_equal(tr["traj_done"][k], ob.done), k
        assert np.array_equal(tr["traj_t"][k], ob.t), k
        if autoreset:   # the episode is over: back to init_pos (mapf_gridworld.py:70-83)
            m = o["term"].astype(bool)
            resets += int(m.sum())
            ob.pos[m] = ob.init_pos[m]
            ob.done[m] = 0
            ob.t[m] = 0
            ob.steps[m] = 0
    assert np.array_equal(_np(b.pos), ob.pos)
    assert np.array_equal(_np(b.t), ob.t)
    assert np.array_equal(_np(b.done), ob.done)
    return resets


# (T, window, occupancy records): pipeline fill and drain (1, 2, 3), the last-batch fold
# either side of a 16-step batch (15, 16, 17, 20), the 16-step action-block instance (33);
# windows 3, 5 and 7 with both record kinds (4 x record bytes is no multiple of 64 for any
# of them: the last 16-byte store of a wave's records is a partial one)
CASES = [(1, 5, False), (2, 3, True), (3, 7, False), (15, 3, False), (16, 5, True), (17, 7, True),
         (20, 3, True), (20, 5, False), (33, 5, False), (33, 7, True)]


def _ids(cases):
    return ["T%d-w%d-%s" % (t, w, "occ" if o else "planes") for t, w, o in cases]


@pytest.mark.parametrize("E", [4, 36])
@pytest.mark.parametrize("T,win,occ", CASES, ids=_ids(CASES))
def test_16_agents(mapfx_mod, T, win, occ, E):
    _run(mapfx_mod, E, 16, T, win, occ=occ)


CASES64 = [(3, 5, False), (16, 3, True), (20, 7, False), (33, 5, True)]


@pytest.mark.parametrize("E", [1, 9])
@pytest.mark.parametrize("T,win,occ", CASES64, ids=_ids(CASES64))
def test_64_agents(mapfx_mod, T, win, occ, E):
    _run(mapfx_mod, E, 64, T, win, occ=occ)


@pytest.mark.parametrize("E", [4, 36])
def test_autoreset(mapfx_mod, E):
    """Episode limit 6: every env resets several times inside a launch of T = 20."""
    resets = _run(mapfx_mod, E, 16, 20, 5, autoreset=True, limit=6)
    assert resets >= 3 * E


@pytest.mark.parametrize("occ", [False, True], ids=["planes", "occ"])
@pytest.mark.parametrize("n,E", [(16, 4), (16, 36), (64, 1), (64, 9)])
def test_guard_rows(mapfx_mod, n, E, occ):
    """T = 3 into the leading slice traj[:3] of five-row buffers: rows 3 and 4 and the
    sentinel bytes around every buffer stay as they were."""
    _run(mapfx_mod, E, n, 3, 3 if occ else 5, occ=occ, spare_rows=2)
