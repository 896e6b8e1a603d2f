"""Plain-Python restatement of PRIMAL's stay-on-goal blocking penalty -- TEST
INFRASTRUCTURE ONLY.

MARL-curve-main/src/envs/mapf_primal.py `get_blocking_reward` (:513-546), added to the
reward of a stay on the goal at :582-585, on top of the unchanged
oracle.primal_dyn_oracle.PrimalWorld.  The reference's planner call
`find_path(world, [start], [goal], 1, 5)` (:506) is taken to return an optimal
4-connected single-robot path, so `len(path)` is the BFS distance + 1 and "no solution"
means the start or goal cell is occupied or the goal is unreachable; the planner's time
limit is not modelled.  Pinned by tests/golden/primal_blocking/pb_*.npz and pbq_*.npz
(tests/golden/gen_primal_blocking_fixtures.py).
"""
from __future__ import annotations

from collections import deque

from oracle.primal_dyn_oracle import GOAL_REWARD, PrimalWorld

BLOCKING_COST = -1.  # :25
INFLATION = 10       # :519


def bfs_dist(blocked, h, w, start, goal):
    """4-connected distance start -> goal over cells not in `blocked`; None when the
    start or goal cell is blocked or the goal cannot be reached."""
    if start in blocked or goal in blocked:
        return None
    if start == goal:
        return 0
    seen = {start}
    q = deque([(start, 0)])
    while q:
        (r, c), d = q.popleft()
        for nr, nc in ((r, c + 1), (r + 1, c), (r, c - 1), (r - 1, c)):
            if nr < 0 or nr >= h or nc < 0 or nc >= w:
                continue
            cell = (nr, nc)
            if cell in seen or cell in blocked:
                continue
            if cell == goal:
                return d + 1
            seen.add(cell)
            q.append((cell, d + 1))
    return None


class BlockingWorld:
    """PrimalWorld whose step() carries the blocking term: the same tuple, with the
    reward of a stay on the goal = GOAL_REWARD + n * BLOCKING_COST and blocking = n > 0,
    plus `last_n` (0 for every other call)."""

    def __init__(self, grid, starts, goals, size=10, diagonal=False, past=None):
        self.world = PrimalWorld(grid, starts, goals, size=size, diagonal=diagonal, past=past)
        w = self.world
        self.walls = {(r, c) for r in range(w.h) for c in range(w.w) if w.grid[r, c] < 0}
        self.last_n = 0

    @property
    def pos(self):
        return self.world.pos

    def blocking_count(self, aid):
        """num_blocking of get_blocking_reward(aid + 1) on the world as it stands."""
        w = self.world
        s = w.size
        tl = (w.pos[aid][0] - s // 2, w.pos[aid][1] - s // 2)
        # :523 loops range(1, num_agents): the last agent is neither examined nor, since
        # other_locations is filled in the same loop, an obstacle of the searches
        others = [j for j in range(w.n - 1)
                  if j != aid and tl[0] <= w.pos[j][0] < tl[0] + s and tl[1] <= w.pos[j][1] < tl[1] + s]
        n = 0
        for j in others:
            after = self.walls | {w.pos[b] for b in others if b != j}
            before = after | {w.pos[aid]}
            d_after = bfs_dist(after, w.h, w.w, w.pos[j], w.goals[j])
            if d_after is None:
                continue
            d_before = bfs_dist(before, w.h, w.w, w.pos[j], w.goals[j])
            if d_before is None or d_before > d_after + INFLATION:
                n += 1
        return n

    def step(self, aid, action):
        maps, vec, reward, done, mask, on_goal, blocking, valid = self.world.step(aid, action)
        self.last_n = 0
        if action == 0 and on_goal:  # action_status == 1 of a stay (:580)
            self.last_n = self.blocking_count(aid)
            reward = GOAL_REWARD + self.last_n * BLOCKING_COST
            blocking = self.last_n > 0
        return maps, vec, float(reward), done, mask, on_goal, blocking, valid


def rooms_layout(rng, h, w, period=5):
    """Walls on every `period`-th row and column, one door per wall segment.
    rng: np.random.Generator.  Returns (grid int8 [h, w] -1 / 0, door cells)."""
    import numpy as np
    grid = np.zeros((h, w), dtype=np.int8)
    rows = list(range(period - 1, h, period))
    cols = list(range(period - 1, w, period))
    grid[rows, :] = -1
    grid[:, cols] = -1
    doors = []

    def segments(limit, cuts):
        edges = [-1] + [c for c in cuts if c < limit] + [limit]
        return [(a + 1, b) for a, b in zip(edges[:-1], edges[1:]) if b > a + 1]

    for r in rows:
        for c0, c1 in segments(w, cols):
            doors.append((r, int(rng.integers(c0, c1))))
    for c in cols:
        for r0, r1 in segments(h, rows):
            doors.append((int(rng.integers(r0, r1)), c))
    for r, c in doors:
        grid[r, c] = 0
    return grid, doors


def rooms_world(rng, h, w, n, n_door, period=5, layout=None):
    """A "rooms with doors" world (rooms_layout, or the given `layout`): the first
    `n_door` agents of a random order start on their goals, which are door cells, the
    rest start and end on distinct free non-door cells.
    Returns (grid, starts, goals, door_agents (0-based, sorted))."""
    import numpy as np
    grid, doors = layout if layout is not None else rooms_layout(rng, h, w, period)
    dset = set(doors)
    free = [(int(r), int(c)) for r, c in np.argwhere(grid == 0) if (int(r), int(c)) not in dset]
    order = [int(a) for a in rng.permutation(n)]
    door_agents = sorted(order[:n_door])
    dsel = [doors[int(i)] for i in rng.choice(len(doors), size=n_door, replace=False)]
    fsel = [free[int(i)] for i in rng.choice(len(free), size=2 * (n - n_door), replace=False)]
    starts, goals = [None] * n, [None] * n
    for a, d in zip(order[:n_door], dsel):
        starts[a] = goals[a] = d
    for i, a in enumerate(order[n_door:]):
        starts[a], goals[a] = fsel[2 * i], fsel[2 * i + 1]
    return grid, starts, goals, door_agents


def rooms_script(rng, n, door_agents, rounds, n_actions=5, p_stay=0.8):
    """`rounds` rounds of one call per agent in order: door agents mostly stay, the
    others move at random.  Returns a list of (agent id 1-based, action)."""
    calls = []
    for _ in range(rounds):
        for a in range(n):
            if a in door_agents and rng.random() < p_stay:
                calls.append((a + 1, 0))
            else:
                calls.append((a + 1, int(rng.integers(0, n_actions))))
    return calls
