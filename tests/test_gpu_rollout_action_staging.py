"""The split rollout's action staging: a launch's int8 actions are fetched once into LDS
in the prologue (mapfx.hip, stage_issue / stage_commit) when the buffer is 16-byte aligned,
T <= 64 and the extra 16 + 64 T bytes of LDS leave the resident workgroups per CU (160 KB
of LDS, counted up to the four the kernel is built for) as they are; every other launch
reads them in register blocks.  `_abi.last_action_path()` tells which: 2 staged, 1 register
blocks, 0 device generator / another kernel.

Parity cases: N = 16 on 12x12 maps with 20 % obstacles, E = 4 (one workgroup) and 36
(several, spread over the XCD renumbering), runner output set, every step of every env
against the C oracle: reward bit patterns, node, edge, avail, term, window, positions,
dones, t and the final state."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S, N, P_OBST = 12, 16, 0.2
STAGE_MAX_T = 64
OUTS = ("reward", "term", "node", "edge", "avail", "obs_window", "traj_pos", "traj_done", "traj_t")


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


def _inst(E, s=S, n=N, seed=41):
    from mapfx.maps import synthetic_instances
    k = (E, s, n, seed)
    if k not in _INST:
        _INST[k] = synthetic_instances(E, s, s, n, p_obstacle=P_OBST, seed=seed)
    return _INST[k]


def _batch(mapfx_mod, inst, win=5, limit=2000, occ=False, s=S):
    b = mapfx_mod.MapfGridBatch(inst["init_pos"], inst["goals"], bits=inst["bits"], hw=(s, s),
                                episode_limit=limit, obs=("window_occ",) if occ else ("window",),
                                window=win)
    b.reset()
    return b


def _actions(T, E, n=N, seed=5):
    """[T, E, n] int8 in 0..4 on the host (seeded)."""
    return np.random.RandomState(seed + 131 * T + E).randint(0, 5, size=(T, E, n)).astype(np.int8)


def _path():
    from mapfx import _abi
    return _abi.last_action_path()


def _check_vs_oracle(b, traj, acts_np, inst, win=5, limit=2000, autoreset=False, occ=False, s=S,
                     ob=None, final=True):
    """Every step of every env against the oracle (which `ob` continues, if given)."""
    from mapfx.batch import window_planes
    from oracle import corc
    if ob is None:
        ob = corc.OracleBatch(inst["bits"], inst["init_pos"], inst["goals"], s, s, limit=limit,
                              nthreads=2)
    torch.cuda.synchronize()
    tr = {k: _np(v) for k, v in traj.items() if isinstance(v, torch.Tensor)}
    if occ:
        tr["obs_window"] = _np(window_planes(traj["obs_window_occ"]))
    resets = 0
    for k in range(acts_np.shape[0]):
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
    if final:
        assert np.array_equal(_np(b.pos), ob.pos) and np.array_equal(_np(b.t), ob.t)
        assert np.array_equal(_np(b.done), ob.done)
    return ob, resets


def _same_traj(t1, t2, keys):
    for k in keys:
        x, y = _np(t1[k]), _np(t2[k])
        if x.dtype == np.float64:
            assert np.array_equal(_u64(x), _u64(y)), k
        else:
            assert np.array_equal(x, y), k


def _same_state(b1, b2):
    for k in ("pos", "done", "t"):
        assert np.array_equal(_np(getattr(b1, k)), _np(getattr(b2, k))), k


# (T, window): pipeline fill and drain (1, 2, 3), both action-block instances either side of
# the 32-step threshold (32, 33), the preloaded "T >= 16" bit (16, 17), the 48-row staging
# passes and their partial last pass (47, 48, 49), the cap (64) and the register-block
# launches past it (65, 96, 97, 128, 129)
LENGTHS = [(1, 5), (2, 3), (3, 7), (8, 5), (9, 3), (16, 5), (17, 7), (20, 5), (32, 3), (33, 5),
           (47, 7), (48, 5), (49, 3), (64, 5), (65, 3), (96, 7), (97, 5), (128, 3), (129, 5)]


@pytest.mark.parametrize("E", [4, 36])
@pytest.mark.parametrize("T,win", LENGTHS, ids=["T%d-w%d" % x for x in LENGTHS])
def test_launch_lengths(mapfx_mod, T, win, E):
    from mapfx import _abi
    inst = _inst(E)
    b = _batch(mapfx_mod, inst, win=win)
    acts_np = _actions(T, E)
    acts = torch.from_numpy(acts_np).cuda()
    assert acts.data_ptr() % 16 == 0
    traj = b.rollout(T, actions=acts, outputs=OUTS)
    assert "mapf_wave_kernel<%d, true, true, true, 16, true, false, %d>" % (win, 8 if T <= 32 else 0) \
        in _abi.last_kernel(), _abi.last_kernel()
    assert _path() == (2 if T <= STAGE_MAX_T else 1)
    _check_vs_oracle(b, traj, acts_np, inst, win=win)
    b.check_err()


def _run_vs_steps(mapfx_mod, inst, acts_np, bad_envs):
    """A rollout of acts_np against single step() launches (a kernel the staging does not
    touch), step by step; the envs of `bad_envs[k]` skip step k and err is set."""
    T = acts_np.shape[0]
    b1 = _batch(mapfx_mod, inst)
    b2 = _batch(mapfx_mod, inst)
    acts = torch.from_numpy(acts_np).cuda()
    traj = b1.rollout(T, actions=acts)
    assert _path() == 2
    keys = ("reward", "reward_f32", "term", "node", "edge", "avail", "obs_window")
    for k in range(T):
        t_before = _np(b2.t).copy()
        out = b2.step(acts[k])
        _same_traj(out, {key: traj[key][k] for key in keys}, keys)
        assert np.array_equal(_np(traj["traj_pos"][k]), _np(b2.pos)), k
        assert np.array_equal(_np(traj["traj_done"][k]), _np(b2.done)), k
        assert np.array_equal(_np(traj["traj_t"][k]), _np(b2.t)), k
        skipped = np.flatnonzero(_np(b2.t) == t_before)
        assert sorted(skipped.tolist()) == sorted(bad_envs.get(k, [])), k
    _same_state(b1, b2)
    with pytest.raises(AssertionError):
        b1.check_err()
    with pytest.raises(AssertionError):
        b2.check_err()


@pytest.mark.parametrize("value", [5, 127, -1, -128])
def test_invalid_bytes(mapfx_mod, value):
    """An action outside 0..4 makes its env -- only that env -- skip the step and sets err:
    at (step 0, agent 0), at (last step, last agent of the last env), in rows 47 and 48
    (the last row of the first staging pass and the first of the second), and in one env
    only of a four-env wave."""
    E, T = 36, 50
    inst = _inst(E)
    acts_np = _actions(T, E, seed=9)
    acts_np[0, 0, 0] = value
    acts_np[T - 1, E - 1, N - 1] = value
    acts_np[47, 5, 3] = value
    acts_np[48, 6, 15] = value
    acts_np[20, 9, 7] = value          # env 9: the second of the four envs of wave 2
    _run_vs_steps(mapfx_mod, inst, acts_np, {0: [0], T - 1: [E - 1], 47: [5], 48: [6], 20: [9]})


@pytest.mark.parametrize("value", [5, -128])
def test_invalid_byte_single_workgroup(mapfx_mod, value):
    E, T = 4, 3
    inst = _inst(E)
    acts_np = _actions(T, E, seed=10)
    acts_np[0, 0, 0] = value
    acts_np[T - 1, E - 1, N - 1] = value
    _run_vs_steps(mapfx_mod, inst, acts_np, {0: [0], T - 1: [E - 1]})


@pytest.mark.parametrize("T", [3, 20, 47, 48])
def test_trailing_bytes(mapfx_mod, T):
    """A row behind the launch's last is never read: T + 1 rows with the last all 5, passed
    as acts[:T], give what an exact-size buffer gives, and err stays clear."""
    E = 36
    inst = _inst(E)
    acts_np = _actions(T, E, seed=11)
    big = torch.full((T + 1, E, N), 5, dtype=torch.int8, device="cuda")
    big[:T] = torch.from_numpy(acts_np).cuda()
    b1 = _batch(mapfx_mod, inst)
    b2 = _batch(mapfx_mod, inst)
    t1 = b1.rollout(T, actions=big[:T], outputs=OUTS)
    assert _path() == 2
    t2 = b2.rollout(T, actions=torch.from_numpy(acts_np).cuda(), outputs=OUTS)
    assert _path() == 2
    torch.cuda.synchronize()
    _same_traj(t1, t2, OUTS)
    _same_state(b1, b2)
    b1.check_err()
    b2.check_err()


@pytest.mark.parametrize("E,T", [(4, 20), (36, 20), (36, 64)])
def test_fallback_triggers(mapfx_mod, E, T):
    """Launches the staging does not take give the staged launch's outputs: int32 and int64
    action tensors and an int8 view at byte offset 1 of a flat buffer (register blocks, path
    1), and the device generator (path 0) on the actions it generates."""
    inst = _inst(E)
    seed = 77
    b0 = _batch(mapfx_mod, inst)
    acts = b0.gen_actions(T, seed)            # what the device generator draws in the kernel
    ref = b0.rollout(T, actions=acts, outputs=OUTS)
    assert _path() == 2
    flat = torch.zeros(T * E * N + 16, dtype=torch.int8, device="cuda")
    off1 = flat[1:1 + T * E * N].view(T, E, N)
    off1.copy_(acts)
    assert off1.data_ptr() % 16 == 1
    for a, path in ((acts.to(torch.int32), 1), (acts.to(torch.int64), 1), (off1, 1), (None, 0)):
        b = _batch(mapfx_mod, inst)
        t = b.rollout(T, actions=a, seed=seed, outputs=OUTS)
        assert _path() == path, (None if a is None else a.dtype, path)
        torch.cuda.synchronize()
        _same_traj(t, ref, OUTS)
        _same_state(b, b0)


def test_chained_launches(mapfx_mod):
    """Three launches of T = 5 enqueued back to back with no host wait (each stages its own
    rows) equal one oracle rollout of 15 steps."""
    E, T, L = 36, 5, 3
    inst = _inst(E)
    b = _batch(mapfx_mod, inst)
    acts_np = _actions(T * L, E, seed=12)
    acts = torch.from_numpy(acts_np).cuda()
    trajs = []
    for i in range(L):
        trajs.append(b.rollout(T, actions=acts[i * T:(i + 1) * T], outputs=OUTS))
        assert _path() == 2
    ob = None
    for i in range(L):
        ob, _ = _check_vs_oracle(b, trajs[i], acts_np[i * T:(i + 1) * T], inst, ob=ob,
                                 final=i == L - 1)


@pytest.mark.parametrize("E", [4, 36])
def test_autoreset(mapfx_mod, E):
    """Episode limit 6: every env resets several times inside a launch of T = 20."""
    T, limit = 20, 6
    inst = _inst(E)
    b = _batch(mapfx_mod, inst, limit=limit)
    acts_np = _actions(T, E, seed=13)
    traj = b.rollout(T, actions=torch.from_numpy(acts_np).cuda(), autoreset=True, outputs=OUTS)
    assert _path() == 2
    _, resets = _check_vs_oracle(b, traj, acts_np, inst, limit=limit, autoreset=True)
    assert resets >= 3 * E


def test_occupancy_window(mapfx_mod):
    from mapfx import _abi
    E, T = 36, 20
    inst = _inst(E)
    b = _batch(mapfx_mod, inst, occ=True)
    acts_np = _actions(T, E, seed=14)
    outs = tuple("obs_window_occ" if k == "obs_window" else k for k in OUTS)
    traj = b.rollout(T, actions=torch.from_numpy(acts_np).cuda(), outputs=outs)
    assert "mapf_wave_kernel<5, true, true, true, 16, true, true, 8>" in _abi.last_kernel()
    assert _path() == 2
    _check_vs_oracle(b, traj, acts_np, inst, occ=True)


def _split_lds(s, n, win):
    """LDS bytes of the split kernel without staged actions (layout() / pick_wave() in
    mapfx.hip) for an s x s grid with n = 16 or 64 agents per env: per env of the wave the two
    count maps and the move map of the padded grid, the wave's two reward rows, the info
    and edge rings, the two store waves' staged records, the reward-code table and ring."""
    def up(x, m):
        return (x + m - 1) // m * m
    pad = max(1, win // 2, win - 1 - win // 2)
    pitch = up(up(pad, 4) + s + pad, 8)
    map_env = up((s + 2 * pad) * pitch, 16)
    epw = 64 // n
    rew_row = n + 2
    wave = 2 * epw * map_env + 2 * up(epw * rew_row * 8, 16)
    fold = 1024 * 8 + 32 * 64 * 2 if n > 16 else 256 * 8 + 32 * 64
    return wave + epw * map_env + 2 * 64 * 16 + 3 * 64 + 2 * 64 * 2 * win * win + fold


def test_split_lds_formula():
    assert _split_lds(32, 16, 5) == 31168      # the bench's C2 shape


@pytest.mark.parametrize("T", [8, 64])
def test_64_agents(mapfx_mod, T):
    """16x16, two envs of 64 agents (one env per workgroup): parity whichever way the
    actions come, and the way is the one the LDS rule gives: staged iff 16 + 64 T more
    bytes stay within 64 KB and leave min(4, 160 KB / LDS per workgroup) unchanged."""
    from mapfx import _abi
    E, s, n = 2, 16, 64
    inst = _inst(E, s=s, n=n, seed=43)
    b = _batch(mapfx_mod, inst, s=s)
    acts_np = _actions(T, E, n=n, seed=15)
    traj = b.rollout(T, actions=torch.from_numpy(acts_np).cuda(), outputs=OUTS)
    assert "mapf_wave_kernel<5, true, true, true, 64, true, false, %d>" % (8 if T <= 32 else 0) \
        in _abi.last_kernel(), _abi.last_kernel()
    split_lds = _split_lds(s, n, 5)
    assert split_lds == 23424
    staged_lds = split_lds + 16 + 64 * T
    rule = staged_lds <= 64 * 1024 and \
        min(4, 160 * 1024 // staged_lds) == min(4, 160 * 1024 // split_lds)
    assert rule                                # six workgroups' LDS per CU at T = 8, five at T = 64
    assert _path() == (2 if rule else 1), (split_lds, staged_lds)
    _check_vs_oracle(b, traj, acts_np, inst, s=s)
