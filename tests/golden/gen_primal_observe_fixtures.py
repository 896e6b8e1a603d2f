#!/usr/bin/env python3
"""Golden vectors of PRIMAL's read-only interface by RUNNING THE REFERENCE (build
container only).

Drives MAPFEnv._step((agent_id, action)) (MARL-curve-main/src/envs/mapf_primal.py:549-637)
through scripted or random calls and, every few calls, takes a SNAPSHOT of the world
without stepping it: positions and agents_past, and for EVERY agent a
  _observe(a)                      (:343-386)
  _listNextValidActions(a, p)      (:639-667) for every previous action p in range(nact)
  on_goal                          (:633)
and _complete() (:404-405).  Written as `primal_observe/po_*.npz` (a subdirectory:
files directly under tests/golden/ are globbed as step fixtures).

Per file: grid, starts, goals, size, diagonal; the calls agent[K], action[K];
snap_at[S] = number of calls made before snapshot i (0 = the fresh world); pos / past
[S, N, 2]; obs [S, N, 4, s, s] u8; vec [S, N, 3] f64; next_mask [S, N, nact] (bit a =
action a listed, column p = previous action p); on_goal [S, N]; done [S].

Usage:  python tests/golden/gen_primal_observe_fixtures.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_fixtures as G  # noqa: E402  (installs the reference stubs)
from gen_primal_dyn_fixtures import free_pick, make_env  # noqa: E402

OUT_DIR = os.path.join(G.OUT_DIR, "primal_observe")
DIRS = {1: (0, 1), 2: (1, 0), 3: (0, -1), 4: (-1, 0), 5: (1, 1), 6: (1, -1), 7: (-1, -1), 8: (-1, 1)}


def snapshot(env, n, nact):
    obs, vec, masks, on_goal = [], [], [], []
    for a in range(1, n + 1):
        m, v = env._observe(a)
        obs.append(np.stack([np.asarray(x) for x in m]).astype(np.uint8))
        vec.append(np.array(v, dtype=np.float64))
        row = []
        for p in range(nact):
            mask = 0
            for x in env._listNextValidActions(a, p):
                mask |= 1 << int(x)
            row.append(mask)
        masks.append(row)
        on_goal.append(env.world.getPos(a) == env.world.getGoal(a))
    return {"pos": np.array(env.getPositions(), dtype=np.int32),
            "past": np.array(env.world.agents_past, dtype=np.int32),
            "obs": np.stack(obs), "vec": np.stack(vec), "next_mask": np.array(masks, dtype=np.int32),
            "on_goal": np.array(on_goal), "done": bool(env._complete())}


def plain_mask(env, a, nact):
    """_listNextValidActions(a, 0) by the NON-diagonal rule (bounds, wall, robot only)."""
    ax, ay = env.world.getPos(a)
    st = env.world.state
    mask = 1
    for act in range(1, nact):
        x, y = ax + DIRS[act][0], ay + DIRS[act][1]
        if 0 <= x < st.shape[0] and 0 <= y < st.shape[1] and st[x, y] == 0:
            mask |= 1 << act
    return mask


def run(name, grid, starts, goals, size, script, every, diagonal=False, snap_at=None):
    env = make_env(grid, starts, goals, size, diagonal)
    n, nact = len(starts), 9 if diagonal else 5
    at = set(range(0, len(script) + 1, every)) if snap_at is None else set(snap_at)
    snaps, where = [], []
    moved_past = refused = 0
    for k in range(len(script) + 1):
        if k in at:
            snaps.append(snapshot(env, n, nact))
            where.append(k)
            if diagonal:
                s = snaps[-1]
                moved_past = max(moved_past, int((s["pos"] != s["past"]).any(1).sum()))
                refused += sum(plain_mask(env, a, nact) != int(s["next_mask"][a - 1, 0])
                               for a in range(1, n + 1))
        if k < len(script):
            env._step(script[k])
    if diagonal:
        # the masks hold diagonal-collision refusals, taken with several agents mid-move
        assert moved_past >= 3 and refused >= 1, (name, moved_past, refused)
    out = {"grid": grid.astype(np.int8), "starts": np.array(starts, dtype=np.int32),
           "goals": np.array(goals, dtype=np.int32), "size": np.array(size),
           "diagonal": np.array(bool(diagonal)),
           "agent": np.array([c[0] for c in script], dtype=np.int32),
           "action": np.array([c[1] for c in script], dtype=np.int32),
           "snap_at": np.array(where, dtype=np.int32)}
    for key in snaps[0]:
        out[key] = np.array([s[key] for s in snaps])
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, "po_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(where), "snapshots, done in",
          int(out["done"].sum()), "diag refusals", refused)
    return out


def rand_script(rng, n, rounds, nact, perm=False):
    return [(int(a) + 1, int(rng.integers(0, nact))) for _ in range(rounds)
            for a in (rng.permutation(n) if perm else range(n))]


def main():
    rng = np.random.default_rng(4242)
    # 1. 10x10, 20 % walls, 8 agents, s = 10
    g = (rng.random((10, 10)) < 0.2).astype(np.int8) * -1
    cells = free_pick(rng, g, 16)
    run("rand10_n8", g, cells[:8], cells[8:], 10, rand_script(rng, 8, 8, 5), 9)
    # 2. crowded 6x6, 12 agents, s = 5 (odd): windows mostly outside the grid, the other
    #    agents' goals clamped onto the window edge
    g = np.zeros((6, 6), dtype=np.int8)
    g[2, 2] = g[3, 4] = -1
    cells = free_pick(rng, g, 24)
    run("crowd6_n12", g, cells[:12], cells[12:], 5, rand_script(rng, 12, 6, 5), 11)
    # 3. non-square 5x9, 4 agents, s = 4
    g = np.zeros((5, 9), dtype=np.int8)
    g[1, 3] = g[3, 6] = g[2, 0] = -1
    cells = free_pick(rng, g, 8)
    run("rect5x9_n4", g, cells[:4], cells[4:], 4, rand_script(rng, 4, 12, 5), 5)
    # 4. 16x16, 20 agents, s = 9, random order of agents
    g = (rng.random((16, 16)) < 0.15).astype(np.int8) * -1
    cells = free_pick(rng, g, 40)
    run("rand16_n20", g, cells[:20], cells[20:], 9, rand_script(rng, 20, 4, 5, perm=True), 13)
    # 5. DIAGONAL_MOVEMENT: crowded 6x6, 14 agents, s = 4; snapshots between the calls of
    #    a round, where several agents' past differs from their position
    g = np.zeros((6, 6), dtype=np.int8)
    g[0, 5] = -1
    cells = free_pick(rng, g, 28)
    run("diag_crowd6_n14", g, cells[:14], cells[14:], 4, rand_script(rng, 14, 6, 9), 9, diagonal=True)
    # 6. DIAGONAL_MOVEMENT: 16x16, 20 agents, s = 7 (odd)
    g = (rng.random((16, 16)) < 0.15).astype(np.int8) * -1
    cells = free_pick(rng, g, 40)
    run("diag_rand16_n20", g, cells[:20], cells[20:], 7, rand_script(rng, 20, 5, 9, perm=True), 13,
        diagonal=True)
    # 7. scripted: agent 1 steps onto agent 2's goal (snapshot), then onto its own; agent 2
    #    walks round to its goal; agent 3 starts on its goal: every agent on its goal, done
    g = np.zeros((5, 5), dtype=np.int8)
    g[3, 1] = -1
    starts, goals = [(0, 0), (2, 2), (4, 4)], [(0, 2), (0, 1), (4, 4)]
    script = [(1, 1), (1, 1), (2, 4), (2, 3), (2, 4), (3, 0)]
    out = run("script_goals", g, starts, goals, 3, script, 1, snap_at=[0, 1, 2, 4, 5, 6])
    assert tuple(out["pos"][1, 0]) == (0, 1) and not out["on_goal"][1, 0]   # on agent 2's goal
    assert out["done"].tolist() == [False, False, False, False, True, True]


if __name__ == "__main__":
    main()
