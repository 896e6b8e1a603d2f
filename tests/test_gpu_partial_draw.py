"""GPU tests of the device scenario draw (mapfx_partial_draw, include/mapfx_partial.h):
the kernel equals its numpy restatement (mapfx.rng.scen_draw) bit for bit through the raw
C ABI -- every sort size and both workgroup shapes, masks, bad envs, shards, the argument
checks -- and through MarlPartialBatch.redraw and the runner's args.runner_device_draw."""
import ctypes
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = 256           # sentinel bytes either side of every written buffer
SENT, OLD = 0xA5, 0x5B
MIXED = [17, 33, 461, 1000, 100, 65, 999, 18, 257, 513, 31, 64, 129, 700, 21, 345, 77, 901, 150,
         47, 260, 19, 600, 35, 810]


def _handle(E, N, env_offset=0, H=64, W=64):
    from mapfx import _abi
    cfg = _abi.PCfg(H=H, W=W, n_agents=N, n_envs=E, env_offset=env_offset, episode_limit=10,
                    obs_window=5, obs_knn_agents=5, map_shared=1, move_reward=-0.01,
                    stay_reward=-0.02, stay_goal_reward=0.0, node_collide_reward=-1.0,
                    edge_collide_reward=-1.0, env_collide_reward=-1.0, complete_reward=1000.0,
                    complete_fac=1.5, gamma=0.99)
    h = ctypes.c_void_p()
    _abi.check(_abi.lib.mapfx_partial_create(ctypes.byref(cfg), ctypes.byref(h)), "create")
    return h


def _table(lengths, seed=1, side=64):
    rs = np.random.RandomState(seed)
    lines = rs.randint(0, side, size=(len(lengths), max(lengths), 4)).astype(np.int16)
    for k, L in enumerate(lengths):
        lines[k, L:] = 0
    return lines, np.array(lengths, dtype=np.int32)


class Raw:
    """One handle and its draw struct over sentinel-guarded buffers."""

    def __init__(self, E, N, lines, n_lines, seed, env_offset=0, episode0=None):
        from mapfx import _abi
        self.E, self.N, self.seed, self.env_offset = E, N, seed, env_offset
        self.lines, self.n_lines = lines, n_lines
        self.h = _handle(E, N, env_offset)
        self.d_lines = torch.as_tensor(lines).cuda()
        self.d_n = torch.as_tensor(n_lines).cuda()
        self.sizes = {"init_pos": E * N * 8, "goal": E * N * 8, "episode": E * 4, "err": 4}
        self.host0, self.buf = {}, {}
        for k, nb in self.sizes.items():
            b = np.full(PAD + nb + PAD, SENT, dtype=np.uint8)
            b[PAD:PAD + nb] = OLD if k in ("init_pos", "goal") else 0
            if k == "episode" and episode0 is not None:
                b[PAD:PAD + nb] = np.asarray(episode0, dtype=np.int32).view(np.uint8)
            self.host0[k] = b
            self.buf[k] = torch.as_tensor(b.copy()).cuda()
        p = {k: self.buf[k].data_ptr() + PAD for k in self.sizes}
        self.sc = _abi.PScen(seed=seed, lines=self.d_lines.data_ptr(), n_lines=self.d_n.data_ptr(),
                             n_files=lines.shape[0], l_max=lines.shape[1], init_pos=p["init_pos"],
                             goal=p["goal"], episode=p["episode"], mask=None, err=p["err"])

    def draw(self, mask=None, sc=None, h="self"):
        from mapfx import _abi
        m = None if mask is None else torch.as_tensor(np.asarray(mask, dtype=np.uint8)).cuda()
        self.sc.mask = None if m is None else m.data_ptr()
        rc = _abi.lib.mapfx_partial_draw(self.h if h == "self" else h,
                                         ctypes.byref(self.sc) if sc is None else sc,
                                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    def get(self, k):
        raw = self.buf[k].cpu().numpy()
        nb = self.sizes[k]
        assert (raw[:PAD] == SENT).all() and (raw[PAD + nb:] == SENT).all(), "sentinels of " + k
        body = raw[PAD:PAD + nb]
        if k in ("init_pos", "goal"):
            return body.view(np.int32).reshape(self.E, self.N, 2)
        return body.view(np.int32)

    def untouched(self):
        return all(np.array_equal(self.buf[k].cpu().numpy(), self.host0[k]) for k in self.sizes)

    def close(self):
        from mapfx import _abi
        _abi.lib.mapfx_partial_destroy(self.h)


def _expect(r, episodes, ip, gl):
    """Apply the restatement's draw with per-env counters `episodes` (-1: not drawn) to ip / gl."""
    from mapfx import rng
    ids = np.arange(r.env_offset, r.env_offset + r.E)
    f, ln = rng.scen_draw(r.seed, ids, np.maximum(episodes, 0), r.n_lines, r.N)
    bad = np.zeros(r.E, dtype=bool)
    for e in range(r.E):
        if episodes[e] < 0:
            continue
        if ln[e, 0] < 0:
            bad[e] = True
            continue
        rows = r.lines[f[e], ln[e]].astype(np.int32)
        ip[e], gl[e] = rows[:, :2], rows[:, 2:]
    return bad


SHAPES = [(1, 1, [2]), (5, 16, MIXED), (7, 64, [65, 1000]), (3, 63, [64, 64, 100]),
          (2, 1024, [4096]), (2, 200, [1025, 2047])]


@pytest.mark.parametrize("E,N,lengths", SHAPES, ids=["L2", "mixed25", "n64", "n63", "l4096", "wg2047"])
def test_kernel_equals_restatement(E, N, lengths):
    assert len(MIXED) == 25 and min(MIXED) == 17 and max(MIXED) == 1000
    lines, n_lines = _table(lengths, seed=E + N)
    r = Raw(E, N, lines, n_lines, seed=0xC0FFEE00 + N)
    ip = np.full((E, N, 2), 0x5B5B5B5B, dtype=np.int32)
    gl = ip.copy()
    for ep in (0, 1):
        assert r.draw() == 0
        assert not _expect(r, np.full(E, ep), ip, gl).any()
        assert np.array_equal(r.get("init_pos"), ip), ep
        assert np.array_equal(r.get("goal"), gl), ep
        assert (r.get("episode") == ep + 1).all() and r.get("err")[0] == 0
    r.close()


def test_mask_leaves_envs_alone():
    lines, n_lines = _table(MIXED, seed=9)
    E, N = 9, 16
    r = Raw(E, N, lines, n_lines, seed=77, episode0=np.arange(E) * 3)
    mask = np.array([1, 0, 0, 1, 1, 0, 1, 0, 2], dtype=np.uint8)
    ip = np.full((E, N, 2), 0x5B5B5B5B, dtype=np.int32)
    gl = ip.copy()
    assert r.draw(mask) == 0
    _expect(r, np.where(mask != 0, np.arange(E) * 3, -1), ip, gl)
    assert np.array_equal(r.get("init_pos"), ip) and np.array_equal(r.get("goal"), gl)
    assert (ip[mask == 0] == 0x5B5B5B5B).all()                # masked out: the old bytes
    assert np.array_equal(r.get("episode"), np.arange(E) * 3 + (mask != 0))
    assert r.draw(np.zeros(E, dtype=np.uint8)) == 0           # nothing selected: nothing written
    assert np.array_equal(r.get("init_pos"), ip) and np.array_equal(r.get("goal"), gl)
    r.close()


def test_bad_envs_are_reported_and_untouched():
    E, N = 24, 16
    lines, n_lines = _table([40, 16, 17, 500], seed=4)        # file 1 has L == N
    r = Raw(E, N, lines, n_lines, seed=5)
    ip = np.full((E, N, 2), 0x5B5B5B5B, dtype=np.int32)
    gl = ip.copy()
    assert r.draw() == 0
    bad = _expect(r, np.zeros(E, dtype=np.int64), ip, gl)
    assert bad.any() and not bad.all()
    assert int(r.get("err")[0]) - 1 in np.flatnonzero(bad).tolist()
    assert np.array_equal(r.get("init_pos"), ip) and np.array_equal(r.get("goal"), gl)
    assert (r.get("init_pos")[bad] == 0x5B5B5B5B).all() and (r.get("goal")[bad] == 0x5B5B5B5B).all()
    assert np.array_equal(r.get("episode"), (~bad).astype(np.int32))
    r.close()


def test_shards_draw_what_the_whole_batch_draws():
    lines, n_lines = _table(MIXED, seed=2)
    N, seed = 16, 0xABCDEF
    whole = Raw(8, N, lines, n_lines, seed)
    parts = [Raw(4, N, lines, n_lines, seed, env_offset=o) for o in (0, 4)]
    for ep in range(2):
        for r in [whole] + parts:
            assert r.draw() == 0
        for k in ("init_pos", "goal", "episode"):
            assert np.array_equal(whole.get(k), np.concatenate([p.get(k) for p in parts])), (ep, k)
    far = Raw(4, N, lines, n_lines, seed, env_offset=(1 << 33) + 5)   # ids past 2^32
    assert far.draw() == 0
    ip = np.zeros((4, N, 2), dtype=np.int32)
    gl = ip.copy()
    assert not _expect(far, np.zeros(4, dtype=np.int64), ip, gl).any()
    assert np.array_equal(far.get("init_pos"), ip) and np.array_equal(far.get("goal"), gl)
    for r in [whole, far] + parts:
        r.close()


def test_invalid_arguments_launch_nothing():
    from mapfx import _abi
    lines, n_lines = _table([40, 50], seed=1)
    r = Raw(4, 8, lines, n_lines, seed=3)
    EINVAL = -1
    assert r.draw(h=None) == EINVAL
    assert r.draw(sc=ctypes.POINTER(_abi.PScen)()) == EINVAL
    for field in ("lines", "n_lines", "init_pos", "goal", "episode", "err"):
        keep = getattr(r.sc, field)
        setattr(r.sc, field, None)
        assert r.draw() == EINVAL, field
        assert field.encode() in _abi.lib.mapfx_last_error()
        setattr(r.sc, field, keep)
    for field, vals in (("n_files", (0, -1)), ("l_max", (0, -5, 4097))):
        keep = getattr(r.sc, field)
        for v in vals:
            setattr(r.sc, field, v)
            assert r.draw() == EINVAL, (field, v)
        setattr(r.sc, field, keep)
    assert r.untouched()
    assert r.draw() == 0 and not r.untouched()                # the struct itself was fine
    r.close()
    empty = Raw(0, 8, lines, n_lines, seed=3)                 # E == 0: OK, no launch
    assert empty.draw() == 0 and empty.untouched()
    empty.close()


# ------------------------------------------------------------------ MarlPartialBatch
def _world(tmp_path, side, p_obstacle, lengths, seed):
    """A synthetic map file, its 25 scen files and their table."""
    from mapfx.maps import load_scen_table, synthetic_instances, write_synthetic_scen
    grid = synthetic_instances(1, side, side, 2, p_obstacle=p_obstacle, seed=seed)["grid"][0]
    mp = tmp_path / "w.map"
    mp.write_text("type octile\nheight %d\nwidth %d\nmap\n%s\n" % (
        side, side, "\n".join("".join("." if c == 0 else "@" for c in row) for row in grid)))
    prefix = str(tmp_path / "w-random-")
    assert max(lengths) <= (grid == 0).sum()                  # so a file's lines start on distinct cells
    assert not any(L & (L - 1) == 0 for L in lengths) and len(set(lengths)) == 25
    write_synthetic_scen(prefix, grid, lengths, seed=seed + 1)
    lines, n_lines = load_scen_table(prefix, side, side)
    return grid, str(mp), prefix, lines, n_lines


def _instances(lines, n_lines, seed, ids, episodes, N):
    from mapfx import rng
    f, ln = rng.scen_draw(seed, ids, episodes, n_lines, N)
    assert (ln >= 0).all()
    rows = lines[f[:, None], ln].astype(np.int32)
    return np.ascontiguousarray(rows[..., :2]), np.ascontiguousarray(rows[..., 2:])


def _same_outputs(a, b, what):
    torch.cuda.synchronize()
    for k in ("obs", "state", "avail", "reward"):
        x, y = a.out[k].cpu().numpy(), b.out[k].cpu().numpy()
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k)
    for k in ("pos", "done", "terminated", "t"):
        assert torch.equal(getattr(a, k), getattr(b, k)), (what, k)


def test_redraw_reset_step_chain(tmp_path):
    from mapfx import MarlPartialBatch, rng
    E, N, seed = 6, 16, 0x51CE
    lengths = [300 + 20 * k + (k % 3) for k in range(25)]    # unequal, none a power of two
    grid, _, _, lines, n_lines = _world(tmp_path, 32, 0.1, lengths, seed=3)
    ph = _instances(lines, n_lines, 1, np.arange(E), 0, N)    # any valid placeholder
    a = MarlPartialBatch(ph[0], ph[1], grids=grid[None], episode_limit=30)
    a.set_scenarios(lines, n_lines, seed=seed)
    acts = torch.as_tensor(rng.gen_actions(9, np.arange(E), np.arange(10), N)).cuda()
    a.redraw()
    a.reset()
    st, gl = _instances(lines, n_lines, seed, np.arange(E), 0, N)
    assert np.array_equal(a.init_pos.cpu().numpy(), st) and np.array_equal(a.goal.cpu().numpy(), gl)
    b = MarlPartialBatch(st, gl, grids=grid[None], episode_limit=30)
    b.reset()
    assert torch.equal(a.goal_dist, b.goal_dist)
    _same_outputs(a, b, "reset")
    for t in range(5):
        a.step(acts[t])
        b.step(acts[t])
        _same_outputs(a, b, t)
    # masked re-draw in mid-episode: the others keep their instance, tables and carried state
    mask = np.array([1, 0, 1, 1, 0, 0], dtype=np.uint8)
    a.redraw(mask)
    a.reset(mask)
    st1, gl1 = _instances(lines, n_lines, seed, np.arange(E), 1, N)
    b.set_agents(np.where(mask[:, None, None] != 0, st1, st), np.where(mask[:, None, None] != 0, gl1, gl),
                 mask)
    b.reset(mask)
    assert np.array_equal(a.episode.cpu().numpy(), 1 + (mask != 0))
    assert torch.equal(a.init_pos, b.init_pos) and torch.equal(a.goal, b.goal)
    assert torch.equal(a.goal_dist, b.goal_dist)
    _same_outputs(a, b, "masked reset")
    for t in range(5, 10):
        a.step(acts[t])
        b.step(acts[t])
        _same_outputs(a, b, t)
    a.check_err()
    # the masked envs alone against a batch built fresh from the restatement's instances
    c = MarlPartialBatch(st1, gl1, grids=grid[None], episode_limit=30)
    m = torch.as_tensor(mask != 0).cuda()
    assert torch.equal(a.goal_dist[m], c.goal_dist[m])


def test_check_err_names_the_bad_env(tmp_path):
    from mapfx import MarlPartialBatch
    E, N = 12, 8
    grid = np.zeros((8, 8), dtype=np.int8)
    lines, n_lines = _table([30, 8], seed=6, side=8)          # file 1: L == N
    a = MarlPartialBatch(np.zeros((E, N, 2), np.int32), np.zeros((E, N, 2), np.int32), grids=grid[None])
    a.set_scenarios(lines, n_lines, seed=21)
    r = types.SimpleNamespace(seed=21, env_offset=0, E=E, N=N, lines=lines, n_lines=n_lines)
    bad = _expect(r, np.zeros(E, dtype=np.int64), np.zeros((E, N, 2), np.int32), np.zeros((E, N, 2), np.int32))
    assert bad.any()
    a.redraw()
    with pytest.raises(AssertionError, match=r"no more than n_agents lines drawn for env (\d+)") as ei:
        a.check_err()
    assert int(str(ei.value).rsplit(" ", 1)[1]) in np.flatnonzero(bad).tolist()
    a.check_err()                                             # reported once
    with pytest.raises(RuntimeError, match="set_scenarios"):
        MarlPartialBatch(np.zeros((1, 1, 2), np.int32), np.zeros((1, 1, 2), np.int32),
                         grids=grid[None]).redraw()


# ------------------------------------------------------------------ runner
def _runner(tmp_path, mp, prefix, B, N, mac, instance_fn=None, **extra):
    from mapfx.episode import DeviceEpisodeBatch, OneHot
    from mapfx.runners import ParallelRunner
    from test_gpu_runner import REWARDS
    args = types.SimpleNamespace(
        env="marl_partial", batch_size_run=B, device="cuda", seed=11,
        env_args=dict(REWARDS, grid_file_path=mp, agents_path=prefix, n_agents=N, episode_limit=12),
        episode_batch_cls=DeviceEpisodeBatch, test_nepisode=B, runner_log_interval=1 << 62, **extra)
    runner = ParallelRunner(args, None, instance_fn=instance_fn)
    info = runner.get_env_info()
    scheme = {"state": {"vshape": info["state_shape"]},
              "obs": {"vshape": info["obs_shape"], "group": "agents"},
              "actions": {"vshape": (1,), "group": "agents", "dtype": torch.long},
              "avail_actions": {"vshape": (info["n_actions"],), "group": "agents", "dtype": torch.int},
              "reward": {"vshape": (1,)}, "terminated": {"vshape": (1,), "dtype": torch.uint8}}
    runner.setup(scheme, {"agents": N}, {"actions": ("actions_onehot", [OneHot(out_dim=5)])}, mac)
    return runner


def test_runner_device_draw_plays_the_restatements_instances(tmp_path):
    from test_gpu_runner import ScriptedMAC
    B, N = 6, 4
    lengths = [5 + 2 * k for k in range(25)]                  # 5 .. 53, unequal, none a power of two
    _, mp, prefix, lines, n_lines = _world(tmp_path, 8, 0.1, lengths, seed=8)
    dev = _runner(tmp_path, mp, prefix, B, N, ScriptedMAC(), runner_device_draw=True)
    calls = []

    def instance_fn(ep):
        calls.append(ep)
        return _instances(lines, n_lines, 11, np.arange(B), ep, N)

    ref = _runner(tmp_path, mp, prefix, B, N, ScriptedMAC(), instance_fn=instance_fn)
    assert (dev.env.episode == 0).all()                       # the placeholder used no episode
    for r in range(2):
        got, exp = dev.run(test_mode=False), ref.run(test_mode=False)
        assert (dev.env.episode == r + 1).all()
        st, gl = _instances(lines, n_lines, 11, np.arange(B), r, N)
        assert np.array_equal(dev.env.init_pos.cpu().numpy(), st)
        assert np.array_equal(dev.env.goal.cpu().numpy(), gl)
        for k, v in exp.data.transition_data.items():
            x = got.data.transition_data[k].cpu().numpy()
            assert np.array_equal(x.view(np.uint8), v.cpu().numpy().view(np.uint8)), (r, k)
        assert dev.t_env == ref.t_env and dev.t_env > 0
    assert calls == [0, 0, 1]
    with pytest.raises(ValueError, match="instance_fn"):
        _runner(tmp_path, mp, prefix, B, N, ScriptedMAC(), instance_fn=instance_fn,
                runner_device_draw=True)
