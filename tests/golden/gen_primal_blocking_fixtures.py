#!/usr/bin/env python3
"""Golden vectors of PRIMAL's stay-on-goal blocking penalty by RUNNING THE REFERENCE
(build container only).

Drives the unmodified MAPFEnv._step (MARL-curve-main/src/envs/mapf_primal.py:549-637)
and MAPFEnv.get_blocking_reward (:513-546).  The one thing the reference cannot run
here is its planner, od_mstar3.cpp_mstar.find_path, which get_blocking_reward calls
only as `find_path(world, [start], [goal], 1, 5)` (:506) and of whose result it uses
only `len(path)` and NoSolutionError.  It is replaced by the BFS stand-in below, written
for this project: 4-connected, a list of dist + 1 entries, NoSolutionError when the
start or goal cell is non-zero or the goal is unreachable -- what an optimal
single-robot planner at inflation 1 returns.  So these fixtures pin the term "up to the
planner".  The planner's time limit is not modelled.

Writes primal_blocking/pb_*.npz (call sequences) and pbq_*.npz (states + the count of
every agent);
the observations are left out (tests/golden/pd_*.npz pin them).  Every scripted case
asserts its intended outcome, so a fixture cannot go vacuous.

Usage:  python tests/golden/gen_primal_blocking_fixtures.py
"""
from __future__ import annotations

import os
import sys
from collections import deque

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import gen_fixtures as G  # noqa: E402  (installs the reference stubs)
from primal_blocking_ref import rooms_script, rooms_world  # noqa: E402

PR = G.PR
# a directory of their own: tests/conftest.py takes every other *.npz directly under
# tests/golden/ for a MAPF_GRID step fixture
OUT_DIR = os.path.join(G.OUT_DIR, "primal_blocking")


def bfs_find_path(world, starts, goals, inflation, time_limit):
    """Stand-in for od_mstar3.cpp_mstar.find_path with one robot."""
    assert len(starts) == 1 and len(goals) == 1 and inflation == 1
    world = np.asarray(world)
    h, w = world.shape
    start, goal = tuple(int(v) for v in starts[0]), tuple(int(v) for v in goals[0])
    if world[start] != 0 or world[goal] != 0:
        raise PR.NoSolutionError()
    prev = {start: None}
    q = deque([start])
    while q:
        cell = q.popleft()
        if cell == goal:
            path = []
            while cell is not None:
                path.append((cell,))
                cell = prev[cell]
            return path[::-1]
        r, c = cell
        for nxt in ((r, c + 1), (r + 1, c), (r, c - 1), (r - 1, c)):
            if 0 <= nxt[0] < h and 0 <= nxt[1] < w and world[nxt] == 0 and nxt not in prev:
                prev[nxt] = cell
                q.append(nxt)
    raise PR.NoSolutionError()


PR.cpp_mstar.find_path = bfs_find_path


def make_env(grid, starts, goals, size, diagonal=False):
    world = grid.astype(np.int64).copy()
    gg = np.zeros(grid.shape, dtype=np.int64)
    for a, ((r, c), (gr, gc)) in enumerate(zip(starts, goals)):
        world[r, c] = a + 1
        gg[gr, gc] = a + 1
    return PR.MAPFEnv(num_agents=len(starts), observation_size=size, world0=world, goals0=gg,
                      DIAGONAL_MOVEMENT=diagonal)


def count_of(x):
    n = x / PR.BLOCKING_COST
    assert n == int(n) and n >= 0
    return int(n)


def base(grid, starts, goals, size, diagonal):
    return {"grid": np.asarray(grid, dtype=np.int8), "starts": np.array(starts, dtype=np.int32),
            "goals": np.array(goals, dtype=np.int32), "size": np.array(size),
            "diagonal": np.array(bool(diagonal))}


def run(name, grid, starts, goals, size, script, diagonal=False):
    """The script through the reference's _step; returns the recorded arrays."""
    env = make_env(grid, starts, goals, size, diagonal)
    seen = []
    inner = env.get_blocking_reward

    def recording(agent_id):  # the unmodified method; only its return value is noted
        x = inner(agent_id)
        seen.append(x)
        return x

    env.get_blocking_reward = recording
    rec = {k: [] for k in ("agent", "action", "reward", "blocking", "n_blocking", "done", "next_mask",
                           "on_goal", "valid", "pos")}
    for aid, act in script:
        del seen[:]
        state, reward, done, nxt, on_goal, blocking, valid = env._step((aid, act))
        mask = 0
        for x in nxt:
            mask |= 1 << int(x)
        rec["agent"].append(aid)
        rec["action"].append(act)
        rec["reward"].append(float(reward))
        rec["blocking"].append(bool(blocking))
        rec["n_blocking"].append(count_of(seen[0]) if seen else 0)
        rec["done"].append(bool(done))
        rec["next_mask"].append(mask)
        rec["on_goal"].append(bool(on_goal))
        rec["valid"].append(bool(valid))
        rec["pos"].append(np.array(env.getPositions(), dtype=np.int32))
    out = base(grid, starts, goals, size, diagonal)
    for k, v in rec.items():
        out[k] = np.array(v)
    out["reward"] = out["reward"].astype(np.float64)
    out["n_blocking"] = out["n_blocking"].astype(np.int32)
    path = os.path.join(OUT_DIR, "pb_%s.npz" % name)
    np.savez_compressed(path, **out)
    stays = (out["action"] == 0) & out["on_goal"]
    print("wrote %-34s %5.1f KB  %4d calls, %3d stays on goal, %3d penalised"
          % (os.path.basename(path), os.path.getsize(path) / 1024.0, len(script), int(stays.sum()),
             int(out["blocking"].sum())))
    return out


def single(name, grid, starts, goals, size, call, reward, n, diagonal=False):
    out = run(name, grid, starts, goals, size, [call], diagonal)
    assert out["reward"][0] == reward and int(out["n_blocking"][0]) == n, (name, out["reward"], out["n_blocking"])
    assert bool(out["blocking"][0]) == (n > 0) and bool(out["on_goal"][0]) and bool(out["valid"][0]), name
    return out


def query(name, grid, goals, size, states, diagonal=False):
    """get_blocking_reward(a) / BLOCKING_COST of EVERY agent a in every state."""
    counts = []
    for pos in states:
        env = make_env(grid, pos, goals, size, diagonal)
        counts.append([count_of(env.get_blocking_reward(a + 1)) for a in range(len(pos))])
    out = base(grid, states[0], goals, size, diagonal)
    del out["starts"]
    out["states"] = np.array(states, dtype=np.int32)
    out["counts"] = np.array(counts, dtype=np.int32)
    path = os.path.join(OUT_DIR, "pbq_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote %-34s %5.1f KB  %3d states, counts sum %d" % (os.path.basename(path),
          os.path.getsize(path) / 1024.0, len(states), int(out["counts"].sum())))
    return out


def doors_h(w):  # 3 x w, row 1 a wall with doors at its two ends
    g = np.zeros((3, w), dtype=np.int8)
    g[1, 1:w - 1] = -1
    return g


def corridor(w):  # 3 x w, rows 0 and 2 walled at columns 1 .. w - 2: row 1 is a corridor
    g = np.zeros((3, w), dtype=np.int8)
    g[0, 1:w - 1] = g[2, 1:w - 1] = -1
    return g


def serpentine(n):
    """n x n (n odd): the even rows are lanes, the odd rows walls with one gap, at
    alternating ends: one path through every cell."""
    g = np.zeros((n, n), dtype=np.int8)
    for r in range(1, n, 2):
        g[r, :] = -1
        g[r, n - 1 if (r // 2) % 2 == 0 else 0] = 0
    return g


def main():
    os.makedirs(OUT_DIR, exist_ok=True)
    states = {}  # name -> (grid, goals, size, [positions]) for the pbq files

    # ---- the scripted single calls ----
    # detour exactly 10 (path lengths 3 and 13): not blocked
    single("door6_detour10", doors_h(6), [(0, 0), (1, 0)], [(2, 0), (1, 0)], 3, (2, 0), 0.0, 0)
    # detour 12: blocked
    single("door7_detour12", doors_h(7), [(0, 0), (1, 0)], [(2, 0), (1, 0)], 3, (2, 0), -1.0, 1)
    # roles swapped: the walker is the last agent, which is never examined (:523)
    single("door7_last_walker", doors_h(7), [(1, 0), (0, 0)], [(1, 0), (2, 0)], 3, (1, 0), 0.0, 0)
    # two walkers need the corridor the sitter stands in
    g = np.zeros((3, 8), dtype=np.int8)
    g[0, 2:6] = g[2, 2:6] = -1
    single("corridor8_two", g, [(0, 1), (2, 1), (1, 4), (0, 0)], [(0, 7), (2, 7), (1, 4), (2, 0)], 10,
           (3, 0), -2.0, 2)
    # the even window is asymmetric: rows 1 .. 4 around a sitter in row 3 (s = 4)
    g = np.zeros((7, 3), dtype=np.int8)
    g[1:6, 0] = g[1:6, 2] = -1
    single("tall7_in_window", g, [(1, 1), (3, 1)], [(6, 1), (3, 1)], 4, (2, 0), -1.0, 1)
    single("tall7_out_of_window", g, [(5, 1), (3, 1)], [(0, 1), (3, 1)], 4, (2, 0), 0.0, 0)
    # agent 1's goal lies under visible agent 3: neither search finds a path
    single("corridor7_goal_taken", corridor(7), [(1, 0), (1, 3), (1, 6), (0, 0)],
           [(1, 6), (1, 3), (0, 6), (2, 0)], 10, (2, 0), 0.0, 0)
    # only agent 2 is examined (agent 3 is the last)
    single("corridor7_one", corridor(7), [(1, 3), (1, 0), (0, 0)], [(1, 3), (1, 6), (2, 6)], 10,
           (1, 0), -1.0, 1)
    # the last agent stands in the corridor too, but other_locations is filled by the same
    # range(1, num_agents) loop: it is no obstacle, "after" finds a path, agent 2 is blocked
    single("corridor7_last_in_way", corridor(7), [(1, 3), (1, 0), (1, 5)], [(1, 3), (1, 6), (0, 6)], 10,
           (1, 0), -1.0, 1)
    states["scripted7"] = (corridor(7), [(1, 6), (1, 3), (0, 6), (2, 0)], 10,
                           [[(1, 0), (1, 3), (1, 6), (0, 0)], [(1, 1), (1, 3), (0, 6), (2, 0)],
                            [(1, 6), (1, 3), (0, 0), (1, 0)], [(0, 0), (1, 2), (1, 4), (2, 6)]])

    # ---- positions change between candidate calls (the kernel undoes later moves) ----
    # 3 x 7 doors; agent 2 sits in the left door, agent 1 walks (0,1) -> (2,0), agent 3 roams
    starts, goals = [(0, 1), (1, 0), (2, 3)], [(2, 0), (1, 0), (2, 6)]
    script = [(1, 3), (3, 1), (2, 0),                      # walker at the door: blocked (14 vs 2)
              (1, 1), (3, 1), (1, 1), (1, 1), (1, 1), (3, 3), (2, 0),   # walker at (0,4): 10 vs 6, not blocked
              (1, 1), (2, 0),                              # walker at (0,5): outside the window
              (1, 1), (1, 2), (1, 2), (3, 0), (1, 3), (1, 3), (2, 0),   # walker went round to (2,5); its
              (2, 4), (1, 3), (2, 0),                      # next move runs into agent 3 (valid = 0: not
              (2, 2), (2, 0), (1, 3), (1, 3), (1, 3), (2, 0), (1, 0), (3, 1), (2, 0)]  # undone)
    out = run("door7_undo", doors_h(7), starts, goals, 10, script)
    stays = [int(n) for n, a, ac, og in zip(out["n_blocking"], out["agent"], out["action"], out["on_goal"])
             if a == 2 and ac == 0 and og]
    assert stays == [1, 0, 0, 0, 0, 0, 0], stays
    assert out["reward"][21] == -0.5 and not out["on_goal"][21]      # the idle stay off the goal
    assert out["reward"][19] == -0.3 and out["reward"][22] == 0.0    # left the goal, came back
    assert [tuple(p) for p in out["pos"][18]] == [(2, 5), (1, 0), (2, 4)] and not out["valid"][17]
    states["door7"] = (doors_h(7), goals, 10, [[tuple(p) for p in out["pos"][k]] for k in (2, 9, 11, 18)])

    # ---- 33 x 33 serpentine: a path longer than 255 levels, the sitter in the lane ----
    g = serpentine(33)
    starts, goals = [(14, 16), (16, 16), (0, 0)], [(32, 30), (16, 16), (0, 5)]
    out = run("serpentine33", g, starts, goals, 10, [(3, 1), (2, 0), (1, 1), (2, 0)])
    assert list(out["n_blocking"]) == [0, 1, 0, 1]
    env = make_env(g, starts, goals, 10)
    assert len(bfs_find_path(env.getObstacleMap(), [starts[0]], [goals[0]], 1, 5)) - 1 > 255
    # a by-pass through the lane above (two gaps in the wall between), walker and sitter in
    # lane 16, the goal more than 255 levels away: detour exactly 10 is not blocked, 12 is
    starts2 = [(16, 14), (16, 16), (0, 0)]
    for tag, west, n in (("detour10", 11, 0), ("detour12", 10, 1)):
        g2 = g.copy()
        g2[15, west] = g2[15, 21] = 0
        out = run("serpentine33_%s" % tag, g2, starts2, goals, 10, [(2, 0)])
        assert list(out["n_blocking"]) == [n], (tag, out["n_blocking"])
    states["serpentine33"] = (g, goals, 10, [starts, [(14, 20), (16, 16), (16, 12)]])

    # ---- DIAGONAL_MOVEMENT: the searches stay 4-connected ----
    # the sitter reaches its door by a diagonal move; an 8-connected search would find
    # a detour of 10 ((0,5) -> (1,6) -> (2,5) diagonally), the 4-connected one has 12
    out = run("diag_door7", doors_h(7), [(0, 0), (0, 1)], [(2, 0), (1, 0)], 10,
              [(2, 6), (2, 0), (1, 1), (2, 0), (1, 3), (2, 0)], diagonal=True)
    assert bool(out["valid"][0]) and bool(out["on_goal"][0])
    assert list(out["n_blocking"]) == [0, 1, 0, 0, 0, 1] and out["reward"][1] == -1.0

    # ---- random rooms with doors ----
    for name, seed, h, w, n, n_door, size, rounds, diag in (
            ("rooms14_n10_s10", 12, 14, 14, 10, 4, 10, 8, False),
            ("rooms14_n10_s7", 20, 14, 14, 10, 4, 7, 8, False),
            ("rooms19x14_n12_s8", 22, 19, 14, 12, 5, 8, 8, False),
            ("diag_rooms14_n10_s9", 2, 14, 14, 10, 4, 9, 8, True)):
        rng = np.random.default_rng(seed)
        grid, starts, goals, door_agents = rooms_world(rng, h, w, n, n_door)
        script = rooms_script(rng, n, door_agents, rounds, 9 if diag else 5)
        out = run(name, grid, starts, goals, size, script, diagonal=diag)
        n_stay = int(((out["action"] == 0) & out["on_goal"]).sum())
        assert n_stay >= 15 and int(out["blocking"].sum()) >= 3, (name, n_stay, int(out["blocking"].sum()))
        if not diag:
            states[name] = (grid, goals, size, [[tuple(p) for p in out["pos"][k]]
                                                for k in range(n - 1, len(script), 2 * n)])
    for name, (grid, goals, size, sts) in states.items():
        q = query(name, grid, goals, size, sts)
        if name.startswith("rooms"):
            assert int(q["counts"].sum()) >= 3, name


if __name__ == "__main__":
    main()
