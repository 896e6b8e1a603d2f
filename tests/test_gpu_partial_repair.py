"""GPU tests of output mode's device collision repair (mapfx_partial_repair,
include/mapfx_partial.h): MarlPartialBatch(output=True) against the CPU play of
tests/partial_repair_cases.py (oracle.partial_oracle.PartialEnvState for the raw step,
mapfx.rng.partial_repair for the repair) bit for bit after every step, the raw C ABI on
guarded buffers, graph replay and the drop-in env's repair="device"."""
import ctypes

import numpy as np
import pytest
import torch

import partial_repair_cases as C

pytestmark = pytest.mark.gpu


def _batch(name, output=True):
    from mapfx.partial import MarlPartialBatch
    H, W, N, E, _, envmaps, off, rounds = C.CASES[name]
    grids, init, goals = C.case_instance(name)
    kw = dict(C.KW)
    if output:
        kw.update(output=True, repair_seed=C.REPAIR_SEED, repair_rounds=rounds)
    return MarlPartialBatch(init, goals, grids=(grids != 0).astype(np.uint8), env_offset=off, **kw)


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_equals_restatement(name):
    x = C.expected(name)
    b = _batch(name)
    b.reset()
    acts = torch.as_tensor(C.case_actions(name)).cuda()
    for k in range(C.T_STEPS):
        out = b.step(acts[k])
        torch.cuda.synchronize()
        # (the reward of step k + 1 reads the carried pdist / pnbr the repair of step k refreshed)
        assert np.array_equal(_np(out["reward"]).view(np.uint64), x["reward"][k].view(np.uint64)), k
        assert np.array_equal(_np(b.pos), x["pos"][k]), k
        assert np.array_equal(_np(b.node), x["node"][k]), k
        assert np.array_equal(_np(b.edge), x["edge"][k]), k
        assert np.array_equal(_np(b.repair_flags), x["flags"][k]), k
        assert np.array_equal(_np(b.repair_rounds_used), x["rounds"][k]), k
        assert np.array_equal(_np(out["obs"]).view(np.uint32), x["obs"][k].view(np.uint32)), k
        assert np.array_equal(_np(out["state"]), x["state"][k]), k
        assert np.array_equal(_np(out["avail"]), x["avail"][k]), k
        assert np.array_equal(_np(b.terminated), x["terminated"][k]), k
        assert np.array_equal(_np(b.at_goal), x["at_goal"][k]), k
        assert np.array_equal(_np(b.goal_cost), x["goal_cost"][k]), k
        assert np.array_equal(_np(b.total_coll), x["total_coll"][k]), k
    from mapfx import _abi
    b.check_err()
    assert "partial_repair_kernel" in _abi.last_kernel()


def test_graph_replay_equals_eager():
    name = "m6_n12_envmaps"
    x = C.expected(name)
    b = _batch(name)
    b.reset()
    acts = torch.as_tensor(C.case_actions(name)).cuda()
    a = acts[0].clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b.step(a)               # warm-up on the capture stream: step 0
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            b.step(a)
    torch.cuda.synchronize()
    b.reset()
    for k in range(8):
        a.copy_(acts[k])
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_np(b.pos), x["pos"][k]), k
        assert np.array_equal(_np(b.repair_flags), x["flags"][k]), k
        assert np.array_equal(_np(b.out["obs"]).view(np.uint32), x["obs"][k].view(np.uint32)), k
        assert np.array_equal(_np(b.out["reward"]).view(np.uint64), x["reward"][k].view(np.uint64)), k


PAD, SENT = 64, 0xA5


def test_abi_on_guarded_buffers():
    from mapfx import _abi
    lib = _abi.lib
    name = "m4_n10"
    x = C.expected(name)
    _, _, N, E, _, _, _, _ = C.CASES[name]
    b = _batch(name, output=False)
    b.reset()
    acts = C.case_actions(name)[0].copy()
    bad_env = 3
    old = b.pos.clone()
    flags = torch.full((PAD + E + PAD,), SENT, dtype=torch.uint8, device="cuda")
    rounds = torch.full((PAD + E * 8 + PAD,), SENT, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def args(a, **kw):
        d = dict(seed=C.REPAIR_SEED, old_pos=old.data_ptr(), actions=a.data_ptr(), action_dtype=_abi.MAPFX_I8,
                 max_rounds=16, flags=flags.data_ptr() + PAD, rounds=rounds.data_ptr() + PAD)
        d.update(kw)
        return _abi.PRepair(**d)

    # every refusal, before any launch
    a_ok = torch.as_tensor(acts).cuda()
    st = ctypes.byref(b._state)
    for bad in (dict(old_pos=None), dict(actions=None), dict(flags=None), dict(action_dtype=7),
                dict(max_rounds=0), dict(max_rounds=17)):
        assert lib.mapfx_partial_repair(b._h, st, ctypes.byref(args(a_ok, **bad)), None, stream) == -1, bad
    assert lib.mapfx_partial_repair(None, st, ctypes.byref(args(a_ok)), None, stream) == -1
    assert lib.mapfx_partial_repair(b._h, None, ctypes.byref(args(a_ok)), None, stream) == -1
    assert lib.mapfx_partial_repair(b._h, st, None, None, stream) == -1
    torch.cuda.synchronize()
    assert (_np(flags) == SENT).all() and (_np(rounds) == SENT).all()
    assert lib.mapfx_partial_repair_offered(b._h) == 1

    # one env given an action outside 0..4: the step skips it, the repair leaves it alone
    acts_bad = acts.copy()
    acts_bad[bad_env, 0] = 9
    a_bad = torch.as_tensor(acts_bad).cuda()
    b.step(a_bad)
    b.err.zero_()
    obs0 = b.out["obs"].clone()
    b.out["obs"].fill_(-7.0)
    assert lib.mapfx_partial_repair(b._h, st, ctypes.byref(args(a_bad)), None, stream) == 0
    torch.cuda.synchronize()
    assert (_np(b.out["obs"]) == -7.0).all()          # out == NULL: no observation written
    b.out["obs"].copy_(obs0)
    f, r = _np(flags), _np(rounds)
    assert (f[:PAD] == SENT).all() and (f[PAD + E:] == SENT).all()
    assert (r[:PAD] == SENT).all() and (r[PAD + E * 8:] == SENT).all()
    want = np.delete(x["flags"][0], bad_env)
    assert np.array_equal(np.delete(f[PAD:PAD + E], bad_env), want) and f[PAD + bad_env] == 0
    assert (r[PAD + bad_env * 8:PAD + bad_env * 8 + 8] == SENT).all()
    assert np.array_equal(np.delete(_np(b.pos), bad_env, 0), np.delete(x["pos"][0], bad_env, 0))
    assert np.array_equal(_np(b.pos)[bad_env], _np(old)[bad_env])
    assert want.any()


def test_not_offered():
    from mapfx import _abi
    from mapfx.partial import MarlPartialBatch
    rs = np.random.RandomState(1)
    grid = np.zeros((1, 12, 12), dtype=np.uint8)
    cells = C.random_cells(rs, grid[0], 65)
    big = MarlPartialBatch(np.array([cells]), np.array([cells]), grids=grid, **C.KW)
    assert _abi.lib.mapfx_partial_repair_offered(big._h) == 0
    fl = torch.zeros(1, dtype=torch.uint8, device="cuda")
    a = torch.zeros((1, 65), dtype=torch.int8, device="cuda")
    ra = _abi.PRepair(seed=0, old_pos=big.pos.data_ptr(), actions=a.data_ptr(), action_dtype=_abi.MAPFX_I8,
                      max_rounds=16, flags=fl.data_ptr(), rounds=None)
    assert _abi.lib.mapfx_partial_repair(big._h, ctypes.byref(big._state), ctypes.byref(ra), None, None) == -1
    with pytest.raises(ValueError):
        MarlPartialBatch(np.array([cells]), np.array([cells]), grids=grid, output=True, **C.KW)
    with pytest.raises(ValueError):
        _batch("m5_n1").rollout(torch.zeros((2, 24, 1), dtype=torch.int8, device="cuda"))


def test_no_envs():
    """E == 0: MAPFX_OK with no launch."""
    from mapfx import _abi
    cfg = _abi.PCfg(H=4, W=4, n_agents=3, n_envs=0, env_offset=0, episode_limit=10, obs_window=5,
                    obs_knn_agents=5, map_shared=1, move_reward=-0.01, stay_reward=-0.02,
                    stay_goal_reward=0.0, node_collide_reward=-1.0, edge_collide_reward=-1.0,
                    env_collide_reward=-1.0, complete_reward=1000.0, complete_fac=1.5, gamma=0.99)
    h = ctypes.c_void_p()
    _abi.check(_abi.lib.mapfx_partial_create(ctypes.byref(cfg), ctypes.byref(h)), "create")
    dummy = torch.full((64,), SENT, dtype=torch.uint8, device="cuda")
    st = _abi.PState(**{k: dummy.data_ptr() for k, _ in _abi.PState._fields_})
    ra = _abi.PRepair(seed=0, old_pos=dummy.data_ptr(), actions=dummy.data_ptr(), action_dtype=_abi.MAPFX_I8,
                      max_rounds=16, flags=dummy.data_ptr(), rounds=dummy.data_ptr())
    try:
        assert _abi.lib.mapfx_partial_repair_offered(h) == 1
        assert _abi.lib.mapfx_partial_repair(h, ctypes.byref(st), ctypes.byref(ra), None, None) == 0
        torch.cuda.synchronize()
        assert (_np(dummy) == SENT).all()
    finally:
        _abi.lib.mapfx_partial_destroy(h)


def test_dropin_device_repair(tmp_path):
    """REGISTRY["marl_partial"](output=True, repair="device") on the mp_out8_n5 instance
    equals a MarlPartialBatch(output=True) of one env with the seed the env drew: one step
    call and one pull per step."""
    import random
    from conftest import load_fixture
    from mapfx.envs import REGISTRY
    from mapfx.partial import MarlPartialBatch
    from test_partial_output_mode import KW
    fx = load_fixture("mp_out8_n5")
    grid = fx["grid"]
    s = grid.shape[0]
    mp = tmp_path / "m.map"
    mp.write_text("type octile\nheight %d\nwidth %d\nmap\n" % (s, s) +
                  "\n".join("".join("." if v == 0 else "@" for v in row) for row in grid) + "\n")
    rows = ["0\tm.map\t%d\t%d\t%d\t%d\t%d\t%d\t0" % (s, s, a[1], a[0], b[1], b[0])
            for a, b in zip(fx["scen_starts"], fx["scen_goals"])]
    rows.append(rows[0])
    for k in range(1, 26):
        (tmp_path / ("m-random-%d.scen" % k)).write_text("version 1\n" + "\n".join(rows) + "\n")
    kw = {k: fx["meta_" + k].item() for k in KW}
    n = int(fx["init_pos"].shape[0])
    random.seed(int(fx["meta_py_seed"]))
    env = REGISTRY["marl_partial"](grid_file_path=str(mp), agents_path=str(tmp_path / "m-random-"),
                                   n_agents=n, output=True, repair="device", **kw)
    random.seed(int(fx["meta_py_seed"]))     # the seed is one more draw after the existing ones
    random.randint(0, 9999)
    random.randint(1, 25)
    random.sample(range(len(rows)), n)
    assert env._repair_seed == random.randint(0, 2 ** 63 - 1)
    random.seed(int(fx["meta_reset_seed"]))
    obs = env.reset()
    assert np.array_equal(obs, fx["obs0"].astype(np.float32))
    b = MarlPartialBatch(fx["init_pos"][None], fx["goals"][None], grids=(grid != 0).astype(np.uint8)[None],
                         output=True, repair_seed=env._repair_seed, **kw)
    b.reset()
    repaired = 0
    for t in range(fx["actions"].shape[0]):
        a = [int(v) for v in fx["actions"][t]]
        r, term, _ = env.step(a)
        out = b.step(torch.as_tensor(np.array([a], dtype=np.int8)).cuda())
        torch.cuda.synchronize()
        repaired += int(_np(b.repair_flags)[0] != 0)
        assert np.float64(r).view(np.uint64) == _np(out["reward"]).view(np.uint64)[0], t
        assert term == bool(_np(b.terminated)[0]), t
        assert [env.agent_pos(i) for i in range(n)] == [tuple(p) for p in _np(b.pos)[0].tolist()], t
        assert np.array_equal(env.get_obs().view(np.uint32), _np(out["obs"])[0].view(np.uint32)), t
        assert np.array_equal(env.get_state(), _np(out["state"])[0].astype(np.int64)), t
    assert repaired >= 5
    # repair="device" without output=True is accepted and does nothing
    random.seed(1)
    plain = REGISTRY["marl_partial"](grid_file_path=str(mp), agents_path=str(tmp_path / "m-random-"),
                                     n_agents=n, repair="device", **kw)
    assert plain._repair_seed == 0 and not plain._device_repair
