"""CPU-side checks of the C-ABI library: it loads, exports every symbol the
header declares, and its host-only helpers agree with the Python host code."""
import os
import re
import subprocess

import numpy as np

from conftest import REPO

HEADERS = [os.path.join(REPO, "include", h) for h in ("mapfx.h", "mapfx_partial.h", "mapfx_primal.h", "mapfx_runner.h")]


def _declared():
    out = set()
    for hdr in HEADERS:
        text = open(hdr).read()
        out |= set(re.findall(r"^\s*(?:[A-Za-z_][\w\s\*]*?)\b(mapfx_\w+)\s*\(", text, re.M))
    return sorted(out)


def test_library_exports_every_declared_symbol():
    import mapfx
    from mapfx import _abi
    declared = _declared()
    assert set(declared) == set(_abi.EXPORTS), declared
    nm = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], stdout=subprocess.PIPE,
                        text=True, check=True).stdout
    exported = set(re.findall(r"\bT (mapfx_\w+)", nm))
    missing = set(declared) - exported
    assert not missing, missing
    assert mapfx.lib.mapfx_abi_version() == 6
    bid = _abi.build_id()
    assert bid.startswith("src=") and " git=" in bid and "unknown" not in bid, bid


def test_host_helpers():
    from mapfx import lib, maps
    for h, w in ((8, 8), (32, 32), (13, 7), (128, 128), (64, 64)):
        assert lib.mapfx_map_stride(h, w) == maps.map_stride(h, w)
    assert lib.mapfx_obs_elem_size(16) == 1
    assert lib.mapfx_obs_elem_size(127) == 1
    assert lib.mapfx_obs_elem_size(128) == 2
    # an edge count is at most N - 1: exact in u8 up to N = 256, u16 above
    assert lib.mapfx_edge_elem_size(256) == 1
    assert lib.mapfx_edge_elem_size(257) == 2


def test_action_generator_host_vs_numpy():
    from mapfx import lib, rng
    seed = 0x1234ABCD5678
    envs = [0, 1, 7, 4095, 32767, 123456789]
    ts = [0, 1, 99, 2 ** 31 - 1]
    ref = rng.gen_actions(seed, envs, ts, 17)
    for ti, t in enumerate(ts):
        for ei, e in enumerate(envs):
            for a in range(17):
                assert lib.mapfx_action(seed, e, t, a) == ref[ti, ei, a]
    # uniform-ish over {0..4}
    big = rng.gen_actions(3, np.arange(512), np.arange(8), 16)
    counts = np.bincount(big.reshape(-1), minlength=5)
    assert counts.min() > 0.18 * big.size and counts.max() < 0.22 * big.size


def test_oracle_generator_matches():
    from mapfx import lib
    from oracle import corc
    for e in (0, 5, 99999):
        for t in (0, 3):
            for a in (0, 15):
                assert corc.lib().orc_action(77, e, t, a) == lib.mapfx_action(77, e, t, a)


def test_synthetic_instances_shard_invariant():
    from mapfx.maps import synthetic_instances
    full = synthetic_instances(64, 16, 16, 8, p_obstacle=0.15, seed=9)
    a = synthetic_instances(32, 16, 16, 8, p_obstacle=0.15, seed=9, env_offset=0)
    b = synthetic_instances(32, 16, 16, 8, p_obstacle=0.15, seed=9, env_offset=32)
    for k in ("grid", "bits", "init_pos", "goals"):
        assert np.array_equal(full[k], np.concatenate([a[k], b[k]]))
    g = full["grid"]
    ip = full["init_pos"]
    for e in range(64):
        cells = ip[e, :, 0] * 16 + ip[e, :, 1]
        assert len(set(cells.tolist())) == 8                       # distinct starts
        assert (g[e].reshape(-1)[cells] == 0).all()                 # on free cells
    frac = (g != 0).mean()
    assert 0.12 < frac < 0.18


def test_bits_roundtrip():
    from mapfx.maps import pack_bits, unpack_bits, warehouse_grid
    rs = np.random.RandomState(0)
    g = -(rs.random_sample((5, 13, 7)) < 0.3).astype(np.int8)
    assert np.array_equal(unpack_bits(pack_bits(g), 13, 7), g)
    w = warehouse_grid(64)
    assert w.shape == (64, 64) and (w[0] == -1).all() and 0.3 < (w != 0).mean() < 0.6


def test_create_rejects_out_of_range_configs():
    """mapfx_create validates its configuration before any HIP call (no GPU needed):
    the grid size of a launch travels in 26 bits of a preloaded kernel argument
    (MAPFX_HOT_ARGS), so n_envs is limited to 2^26 - 1 envs per handle."""
    import ctypes
    from mapfx import lib
    from mapfx._abi import Cfg

    def create(**kw):
        c = Cfg(H=8, W=8, n_agents=2, n_envs=4, env_offset=0, episode_limit=100,
                step_reward=-0.01, collide_reward=-10.0, obs_mode=0, window=5,
                primal_size=5, map_shared=0)
        for k, v in kw.items():
            setattr(c, k, v)
        h = ctypes.c_void_p()
        return lib.mapfx_create(ctypes.byref(c), ctypes.byref(h)), lib.mapfx_last_error()

    for kw, what in (({"n_envs": 1 << 26}, b"n_envs"), ({"n_envs": -1}, b"n_envs"),
                     ({"n_agents": 0}, b"n_agents"), ({"n_agents": 1025}, b"n_agents"),
                     ({"H": 0}, b"grid"), ({"W": 4097}, b"grid"),
                     # 256 envs per block x 16 MB of map: the LDS sum passes 2^31 before the refusal
                     ({"H": 4096, "W": 4096, "n_agents": 1}, b"one env needs")):
        rc, msg = create(**kw)
        assert rc == -1 and what in msg, (kw, rc, msg)


def test_create_layout_matches_restated_geometry():
    """mapfx_create's layout is a plain function of the configuration (csrc/mapfx.hip layout()),
    and without a PRIMAL observation (no device LUT) and within 64 KB of LDS (no function
    attribute) mapfx_create makes no HIP call that matters: for every distinct configuration
    of the MAPF step cases, mapfx_query equals the restated geometry on the fields
    tests/test_gpu_mapf_step_shapes.py compares -- here without a GPU, and with no launch."""
    import ctypes
    from mapf_step_cases import CASES, OBS_PRIMAL, case_geometry, limit_of, mode_of
    from mapfx import lib
    from mapfx._abi import Cfg, Info

    configs = {}
    for c in CASES:
        configs.setdefault((c.H, c.W, c.N, c.window, c.psize, mode_of(c.obs), c.rewards), c)
    checked = 0
    for (H, W, N, window, psize, mode, rewards), c in configs.items():
        g = case_geometry(c)
        assert g is not None, c.name
        if mode & OBS_PRIMAL or g.gen_lds > 64 * 1024:
            continue
        cfg = Cfg(H=H, W=W, n_agents=N, n_envs=c.E, env_offset=c.env_offset, episode_limit=limit_of(c),
                  step_reward=rewards[0], collide_reward=rewards[1], obs_mode=mode, window=window,
                  primal_size=psize, map_shared=0)
        h = ctypes.c_void_p()
        assert lib.mapfx_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, (c.name, lib.mapfx_last_error())
        try:
            inf = Info()
            assert lib.mapfx_query(h, ctypes.byref(inf)) == 0, c.name
            got = {k: getattr(inf, k) for k, _ in Info._fields_}
        finally:
            lib.mapfx_destroy(h)
        assert got == dict(lanes_per_env=g.L, agents_per_lane=g.apl, envs_per_block=g.EPB,
                           block_threads=g.BT, lds_bytes=g.gen_lds, cell_bytes=g.es, pad=g.P), c.name
        checked += 1
    assert checked >= 140, (checked, len(configs))   # a skip rule cannot quietly empty the test
