"""Cases of output mode's device collision repair (mapfx_partial_repair), shared by the CPU
rule tests (tests/test_partial_repair_rule.py) and the GPU tests
(tests/test_gpu_partial_repair.py).

A case is E envs stepped T times with uniform random actions (rng.gen_actions); `expected`
plays it on the CPU -- oracle.partial_oracle.PartialEnvState for the raw step,
mapfx.rng.partial_repair for the repair -- once per process, and the tests only read the
result."""
import functools
import random

import numpy as np

from conftest import load_fixture

T_STEPS = 25
KW = dict(obs_window=5, obs_knn_agents=5, episode_limit=100, move_reward=-0.01, stay_reward=-0.02,
          stay_goal_reward=0, node_collide_reward=-1, edge_collide_reward=-1, env_collide_reward=-1,
          complete_reward=1000, complete_fac=1.5, gamma=0.99)

# name -> (H, W, N, E, obstacle share, per-env maps, env_offset, repair_rounds)
CASES = {
    "fix8_n5": (8, 8, 5, 24, None, False, 0, 16),        # the grid of mp_out8_n5
    "m6_n12_envmaps": (6, 6, 12, 32, 0.10, True, 0, 16),
    "m4_n10": (4, 4, 10, 24, 0.0, False, 0, 16),
    "m16_n64": (16, 16, 64, 24, 0.10, False, 0, 16),     # a full wave
    "m5_n1": (5, 5, 1, 24, 0.10, False, 0, 16),          # nothing to repair
    "m3_n2_off1000": (3, 3, 2, 24, 0.0, False, 1000, 16),
    "m6_n12_cap1": (6, 6, 12, 24, 0.10, False, 0, 1),    # the cap path
}
ACT_SEED, REPAIR_SEED = 0x5EED0001, 0xA11CE5


def random_map(rs, H, W, share):
    """[H, W] int64, -1 obstacle / 0 free, about `share` of the cells obstacles."""
    return -(rs.random_sample((H, W)) < share).astype(np.int64)


def random_cells(rs, grid, n):
    """n distinct free cells."""
    free = np.argwhere(grid == 0)
    return [tuple(int(v) for v in free[i]) for i in rs.permutation(len(free))[:n]]


def case_instance(name):
    """(grids [E | 1, H, W] int64 with -1 obstacles, init [E, N, 2], goals [E, N, 2])."""
    H, W, N, E, share, envmaps, _, _ = CASES[name]
    rs = np.random.RandomState(sum(name.encode()))
    if share is None:
        grids = np.asarray(load_fixture("mp_out8_n5")["grid"], dtype=np.int64)[None]
    else:
        grids = np.stack([random_map(rs, H, W, share) for _ in range(E if envmaps else 1)])
        for g in grids:
            while (g == 0).sum() < N:          # room for distinct starts (N <= H * W)
                g[tuple(rs.randint(0, s) for s in g.shape)] = 0
    init = np.zeros((E, N, 2), dtype=np.int32)
    goals = np.zeros((E, N, 2), dtype=np.int32)
    for e in range(E):
        g = grids[e if envmaps else 0]
        init[e] = random_cells(rs, g, N)
        goals[e] = random_cells(rs, g, N)
    return grids, init, goals


def case_actions(name):
    """int8 [T, E, N]: rng.gen_actions keyed by the GLOBAL env ids."""
    from mapfx import rng
    _, _, N, E, _, _, off, _ = CASES[name]
    return rng.gen_actions(ACT_SEED, np.arange(off, off + E), np.arange(T_STEPS), N)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The case played on the CPU.  Per step k (arrays [T, E, ...]): pos, node, edge, flags,
    rounds, obs (float32), state (float32), avail (5-bit masks), reward (float64), terminated,
    at_goal, goal_cost, total_coll; `raw` (the positions the raw step left, before the repair),
    `needed` [T, E] (the raw step had a collision) and `counters` (rng.REPAIR_COUNTERS,
    summed)."""
    from mapfx import rng
    from oracle.partial_oracle import PartialEnvState
    H, W, N, E, _, envmaps, off, rounds = CASES[name]
    grids, init, goals = case_instance(name)
    acts = case_actions(name)
    envs = [PartialEnvState(grids[e if envmaps else 0], init[e], goals[e], **KW) for e in range(E)]
    D = 2 * KW["obs_window"] ** 2 + 13 * KW["obs_knn_agents"]
    out = dict(pos=np.zeros((T_STEPS, E, N, 2), np.int32), raw=np.zeros((T_STEPS, E, N, 2), np.int32),
               node=np.zeros((T_STEPS, E, N), np.uint8),
               edge=np.zeros((T_STEPS, E, N), np.int32), flags=np.zeros((T_STEPS, E), np.uint8),
               rounds=np.zeros((T_STEPS, E, 2), np.int32), obs=np.zeros((T_STEPS, E, N, D), np.float32),
               state=np.zeros((T_STEPS, E, 3), np.float32), avail=np.zeros((T_STEPS, E, N), np.uint8),
               reward=np.zeros((T_STEPS, E), np.float64), terminated=np.zeros((T_STEPS, E), np.uint8),
               at_goal=np.zeros((T_STEPS, E, N), np.uint8), goal_cost=np.zeros((T_STEPS, E, N), np.int32),
               total_coll=np.zeros((T_STEPS, E), np.int32), needed=np.zeros((T_STEPS, E), bool))
    cnt = {}
    for k in range(T_STEPS):
        for e, env in enumerate(envs):
            old = list(env.pos)
            out["reward"][k, e], _ = env.step(acts[k, e])
            out["needed"][k, e] = bool(sum(env.node) + sum(env.edge))
            out["raw"][k, e] = env.pos
            pos, nv, ev, fl, rd = rng.partial_repair_env(old, env.pos, acts[k, e], env.grid, env.t, off + e,
                                                         REPAIR_SEED, rounds, counters=cnt)
            env.pos, env.node, env.edge = [tuple(p) for p in pos], list(nv), list(ev)
            env._refresh()
            out["pos"][k, e], out["node"][k, e], out["edge"][k, e] = pos, nv, ev
            out["flags"][k, e], out["rounds"][k, e] = fl, rd
            out["obs"][k, e] = env.obs().astype(np.float32)
            out["state"][k, e] = env.state().astype(np.float32)
            out["avail"][k, e] = (env.avail().astype(np.int64) << np.arange(5)).sum(-1)
            out["terminated"][k, e] = env.terminated
            out["at_goal"][k, e] = env.at_goal
            out["goal_cost"][k, e] = env.goal_cost
            out["total_coll"][k, e] = env.total_collisions
    out["counters"] = np.array([cnt.get(c, 0) for c in rng.REPAIR_COUNTERS], dtype=np.int64)
    return out


def shuffle_order(site, r, owner, items):
    """The reference's own shuffles: random.shuffle on the global stream."""
    items = list(items)
    random.shuffle(items)
    return items
