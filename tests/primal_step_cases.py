"""Worlds, goal-seeking call scripts, the dispatch rule and the comparer of the PRIMAL
step tests (tests/test_primal_step_cases.py on the CPU, tests/test_gpu_primal_step_shapes.py
on the device).  TEST INFRASTRUCTURE ONLY; no test lives here.

Random actions never finish a world, so `done`, reward 0.0 and status 2 stay unpinned.
`drive` therefore builds each world's calls one by one ON the restatement
(oracle.primal_dyn_oracle.PrimalWorld): mostly a step that lowers an agent's BFS distance
to its goal, some stays, some moves out of the grid from a border cell, the rest random --
and with DIAGONAL_MOVEMENT a two-call gadget that makes one agent cross another's last
diagonal move (refused by State.diagonalCollision alone).  The expected outputs of every
call are the restatement's; `compare` names the first element that differs.

`expected_kernel` restates the host's dispatch (the comments of mapfx_primal_create and
its LDS layout) and returns the instance as mapfx_last_kernel prints it.
"""
from __future__ import annotations

import functools
from collections import deque, namedtuple

import numpy as np

from oracle.primal_dyn_oracle import DIRS, PrimalWorld

FIELDS = ("reward", "done", "next_mask", "on_goal", "valid", "obs", "vec")
TOP, BOTTOM, LEFT, RIGHT = 1, 2, 4, 8   # bit flags of a side (out-of-bounds moves, clamped goals)


# --------------------------------------------------------------------------- worlds
def _bfs(grid, src, radius, diag=False):
    """{cell: distance <= radius} from src over the free cells (agents do not block)."""
    h, w = grid.shape
    steps = [DIRS[a] for a in range(1, 9 if diag else 5)]
    dist = {src: 0}
    q = deque([src])
    while q:
        cur = q.popleft()
        d = dist[cur]
        if d == radius:
            continue
        for dr, dc in steps:
            nb = (cur[0] + dr, cur[1] + dc)
            if 0 <= nb[0] < h and 0 <= nb[1] < w and grid[nb] >= 0 and nb not in dist:
                dist[nb] = d + 1
                q.append(nb)
    return dist


def _without_goals(grid, goals, a):
    """The grid with every goal but agent a's turned into an obstacle."""
    g = np.array(grid)
    for b, cell in enumerate(goals):
        if b != a:
            g[tuple(cell)] = -1
    return g


def world(rng, H, W, N, density, n_off, corners, guest=0):
    """One world: a random obstacle grid (int8, -1 = obstacle), distinct goals on free cells
    and starts equal to the goals, except that `n_off` agents start at BFS distance 1..4
    from their goal; these are drawn among the agents that are neither corner agents,
    guests nor the pair (below), so with fewer such agents fewer start off (none at
    N = 2).  corners=True: the 5 x 5 block around every corner is cleared, agents
    1..4 have the corner cells as goals and start within distance 3 of them (they come on
    top of n_off).  guest > 0 (with corners; the cases pass s // 2 + 1): agents 5 and 6 (5
    alone when N = 6) are guests of the corners (0, 0) and (H-1, W-1) -- their goal lies
    `guest` cells diagonally inside the corner, just outside the window of an agent standing
    on it, and they start between the two: the corner agent sees a guest whose goal is
    clamped to the far window edge, a guest at home sees a corner agent whose goal is
    clamped to the near one, so one corner yields all four sides.  The goals of
    the last two agents are orthogonal neighbours where the grid allows it (the
    diagonal-crossing gadget of `drive` starts from such a pair)."""
    grid = np.where(rng.random((H, W)) < density, -1, 0).astype(np.int8)
    ncorner = min(N, 4) if corners else 0
    corner_cells = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    if corners:
        for r, c in corner_cells:
            grid[max(0, r - 4):r + 5, max(0, c - 4):c + 5] = 0
    goals = list(corner_cells[:ncorner])
    taken = set(corner_cells) if corners else set()
    guests = []
    if corners and guest and N >= ncorner + 2:   # (one guest where a second leaves no pair)
        gr = guest if guest <= H - 2 else (H - 1) // 2    # a window taller than the grid: no row clamp
        gc = guest if guest <= W - 2 else (W - 1) // 2
        both = (((gr, gc), (0, 0)), ((H - 1 - gr, W - 1 - gc), (H - 1, W - 1)))
        for cell, corner in both[:min(2, N - ncorner - 1)]:
            grid[max(0, cell[0] - 1):cell[0] + 2, max(0, cell[1] - 1):cell[1] + 2] = 0
            guests.append((len(goals), corner, (gr, gc)))
            goals.append(cell)
            taken.add(cell)
    free = [tuple(int(v) for v in p) for p in np.argwhere(grid == 0)]
    order = iter(rng.permutation(len(free)))
    while len(goals) < N:
        if len(goals) == N - 1 and len(goals) > ncorner:   # the pair
            r, c = goals[-1]
            nbs = [(r + dr, c + dc) for dr, dc in ((0, 1), (1, 0), (0, -1), (-1, 0))]
            nbs = [p for p in nbs if 0 <= p[0] < H and 0 <= p[1] < W and grid[p] == 0 and p not in taken]
            if nbs:
                p = nbs[int(rng.integers(len(nbs)))]
                goals.append(p)
                taken.add(p)
                continue
        p = free[next(order)]
        if p in taken:
            continue
        goals.append(p)
        taken.add(p)
    starts = list(goals)
    occupied = set(starts)
    first = ncorner + len(guests)
    rest = [int(a) for a in rng.permutation(np.arange(first, max(first, N - 2)))]   # (not the pair)
    off = ([(a, 3, None, None) for a in range(ncorner)] + [(a, 3, cn, o) for a, cn, o in guests]
           + [(a, 4, None, None) for a in rest[:n_off]])
    for a, far, cn, o in off:
        # (over the cells that are nobody else's goal: the way back is never walled off by
        # agents that sit on their goals)
        ring = [p for p, d in _bfs(_without_goals(grid, goals, a), goals[a], far).items()
                if d >= 1 and p not in occupied]
        if cn:   # nearer the corner than the goal: on both axes if possible, else on either
            nr = [(abs(p[0] - cn[0]) < o[0], abs(p[1] - cn[1]) < o[1]) for p in ring]
            ring = ([p for p, n in zip(ring, nr) if all(n)] or [p for p, n in zip(ring, nr) if any(n)]
                    or ring)
        if not ring:
            continue
        p = ring[int(rng.integers(len(ring)))]
        occupied.discard(starts[a])
        starts[a] = p
        occupied.add(p)
    return {"grid": grid, "starts": np.array(starts, np.int32), "goals": np.array(goals, np.int32)}


# --------------------------------------------------------------------------- scripts
class RecordedWorld(PrimalWorld):
    """PrimalWorld that keeps the status of its last move, and can answer without the
    midpoint test (State.diagonalCollision) -- both for the coverage counts only."""
    status = 0
    no_midpoint = False

    def move(self, aid, action):
        self.status = super().move(aid, action)
        return self.status

    def diagonal_collision(self, aid, new):
        return False if self.no_midpoint else super().diagonal_collision(aid, new)


def _inside(w, p):
    return 0 <= p[0] < w.h and 0 <= p[1] < w.w


def _open(w, p):
    return _inside(w, p) and w.grid[p] >= 0 and w._occupant(p) < 0


def _crossing(rng, w):
    """The gadget: agents A at p and B at p + d (d orthogonal), p + e and p + d + e open
    (e perpendicular).  B steps diagonally to p + e; then A's diagonal step to p + d + e has
    the midpoint of B's last move and is refused, its target cell free.  Returns the two
    calls [(B, action), (A, action)] or None."""
    act_of = {v: k for k, v in DIRS.items()}
    where = {p: a for a, p in enumerate(w.pos)}
    found = []
    for a, p in enumerate(w.pos):
        for d in ((0, 1), (1, 0), (0, -1), (-1, 0)):
            b = where.get((p[0] + d[0], p[1] + d[1]))
            if b is None:
                continue
            for e in ((d[1], d[0]), (-d[1], -d[0])):
                if _open(w, (p[0] + e[0], p[1] + e[1])) and _open(w, (p[0] + d[0] + e[0], p[1] + d[1] + e[1])):
                    found.append([(b, act_of[(e[0] - d[0], e[1] - d[1])]), (a, act_of[(d[0] + e[0], d[1] + e[1])])])
    return found[int(rng.integers(len(found)))] if found else None


def drive(rng, wd, K, s=10, diag=False, radius=12, calls=None):
    """K calls for the world `wd` (of `world`), chosen call by call on the restatement --
    or, with calls = (ids [K] 1-based, actions [K]), those calls as given (rng unused).
    Returns ids (1-based) and actions [K], the expected outputs of every call -- reward
    and vec as fp64 bit patterns (uint64), done, next_mask, on_goal, valid, obs [K, 4, s, s] --
    pos / past [N, 2] after the last call and after every call (pos_at / past_at), and what
    the coverage conditions count: status, the acting agent's cell (`at`), the sides an
    out-of-bounds move left by (`oob`), the window sides a visible agent's goal was clamped
    to (`clamp`), `mid` (a move refused by the midpoint test alone) and `mid_mask` (the
    call's next_mask lacks a bit that the same 9-action mask has with the midpoint test
    switched off: a bit removed by it alone)."""
    w = RecordedWorld(wd["grid"], wd["starts"], wd["goals"], s, diagonal=diag)
    N, nact, half = w.n, 9 if diag else 5, s // 2
    dist = {}
    pending = []
    out = {"ids": np.zeros(K, np.int32), "actions": np.zeros(K, np.int32),
           "reward": np.zeros(K, np.uint64), "vec": np.zeros((K, 3), np.uint64),
           "done": np.zeros(K, np.uint8), "next_mask": np.zeros(K, np.int64),
           "on_goal": np.zeros(K, np.uint8), "valid": np.zeros(K, np.uint8),
           "obs": np.zeros((K, 4, s, s), np.uint8),
           "pos_at": np.zeros((K, N, 2), np.int32), "past_at": np.zeros((K, N, 2), np.int32),
           "status": np.zeros(K, np.int64), "at": np.zeros((K, 2), np.int64),
           "oob": np.zeros(K, np.int64), "clamp": np.zeros(K, np.int64),
           "mid": np.zeros(K, bool), "mid_mask": np.zeros(K, bool)}
    for k in range(K):
        call = pending.pop(0) if pending else None
        if calls is not None:      # a given script (`episode`): nothing is drawn
            call, u = (int(calls[0][k]) - 1, int(calls[1][k])), 1.0
        else:
            u = rng.random()
        off = [a for a in range(N) if w.pos[a] != w.goals[a]]
        if call is None and u < 0.55 and off:                      # toward the goal
            a = off[int(rng.integers(len(off)))]
            if a not in dist:     # around the other agents' goals where that is possible
                dist[a] = _bfs(_without_goals(w.grid, w.goals, a), w.goals[a], radius, diag)
                if w.pos[a] not in dist[a]:
                    dist[a] = _bfs(w.grid, w.goals[a], radius, diag)
            here = dist[a].get(w.pos[a], 1 << 30)
            better = [m for m in range(1, nact)
                      if dist[a].get((w.pos[a][0] + DIRS[m][0], w.pos[a][1] + DIRS[m][1]), 1 << 30) < here]
            clear = [m for m in better
                     if _open(w, (w.pos[a][0] + DIRS[m][0], w.pos[a][1] + DIRS[m][1]))]
            if clear and rng.random() < 0.9:    # (the rest bump into whoever stands there)
                better = clear
            if better:
                call = (a, better[int(rng.integers(len(better)))])
        elif call is None and 0.55 <= u < 0.70:                    # a stay
            pool = off if off and rng.random() < 0.5 else range(N)
            call = (int(pool[int(rng.integers(len(pool)))]), 0)
        elif call is None and 0.70 <= u < 0.80:                    # out of the grid
            outs = [(a, m) for a in range(N) for m in range(1, nact)
                    if (w.pos[a][0] in (0, w.h - 1) or w.pos[a][1] in (0, w.w - 1))
                    and not _inside(w, (w.pos[a][0] + DIRS[m][0], w.pos[a][1] + DIRS[m][1]))]
            if outs:
                call = outs[int(rng.integers(len(outs)))]
        elif call is None and diag and u >= 0.93:                  # cross a diagonal move
            pair = _crossing(rng, w)
            if pair:
                call, pending = pair[0], [pair[1]]
        if call is None:                                           # anyone, any move
            call = (int(rng.integers(N)), int(rng.integers(1, nact)))
        a, m = call
        tgt = (w.pos[a][0] + DIRS[m][0], w.pos[a][1] + DIRS[m][1])
        tgt_open = m != 0 and _open(w, tgt)
        maps, vec, r, done, mask, on_goal, _, valid = w.step(a, m)
        out["ids"][k], out["actions"][k] = a + 1, m
        out["reward"][k] = np.float64(r).view(np.uint64)
        out["vec"][k] = np.asarray(vec, np.float64).view(np.uint64)
        out["done"][k], out["next_mask"][k], out["on_goal"][k], out["valid"][k] = done, mask, on_goal, valid
        out["obs"][k] = maps
        out["pos_at"][k], out["past_at"][k] = w.pos, w.past
        out["status"][k], out["at"][k] = w.status, w.pos[a]
        if w.status == -1:
            out["oob"][k] = (TOP * (tgt[0] < 0) | BOTTOM * (tgt[0] >= w.h) | LEFT * (tgt[1] < 0)
                             | RIGHT * (tgt[1] >= w.w))
        out["mid"][k] = w.status == -3 and tgt_open
        if diag:   # the same 9-action mask with the midpoint test alone switched off
            w.no_midpoint = True
            plain = w.next_mask(a, m)
            w.no_midpoint = False
            assert plain & mask == mask
            out["mid_mask"][k] = plain != mask
        tr, tc = w.pos[a][0] - half, w.pos[a][1] - half
        for b in range(N):
            br, bc = w.pos[b]
            if b != a and tr <= br < tr + s and tc <= bc < tc + s:
                x, y = w.goals[b]
                out["clamp"][k] |= (TOP * (x < tr) | BOTTOM * (x > tr + s - 1) | LEFT * (y < tc)
                                    | RIGHT * (y > tc + s - 1))
    out["pos"], out["past"] = np.array(w.pos, np.int32), np.array(w.past, np.int32)
    return out


# --------------------------------------------------------------------------- cases
# lanes: MAPFX_PRIMAL_LANES ("" = the host's own rule); path: MAPFX_PRIMAL_PATH; pool: the
# number of distinct worlds the E worlds cycle through (0: every world its own)
Case = namedtuple("Case", "name H W N s diag E K density n_off corners lanes path pool seed kernel")


def _case(name, H, W, N, s, diag, kernel, E=9, K=70, density=0.15, n_off=2, corners=False, lanes="",
          path="", pool=0, seed=0):
    return Case(name, H, W, N, s, diag, E, K, density, n_off, corners, lanes, path, pool, seed, kernel)


def _b(x):
    return "true" if x else "false"


def _cases():
    seq, act = "primal_seq_kernel<%d, %s>", "primal_act_kernel<%d, %d, %s, %d>"
    out = []
    # a) primal_seq_kernel instances, its eligibility edges, and just past each edge
    for d in (False, True):
        out.append(_case("seq6", 11, 9, 5, 6, d, seq % (6, _b(d))))
        out.append(_case("seq8", 13, 16, 9, 8, d, seq % (8, _b(d))))
    out.append(_case("seq4", 9, 13, 5, 4, True, seq % (4, "true")))
    out.append(_case("seq10-limits", 54, 54, 64, 10, True, seq % (10, "true"), K=130, corners=True, density=0.1))
    out.append(_case("seq4-limits", 60, 60, 64, 4, False, seq % (4, "false"), corners=True, density=0.1))
    out.append(_case("seq10-H54", 54, 20, 8, 10, False, seq % (10, "false"), corners=True))
    out.append(_case("seq10-W54", 20, 54, 8, 10, True, seq % (10, "true"), corners=True))
    out.append(_case("past-H", 55, 20, 8, 10, False, act % (10, 6, "false", 1)))
    out.append(_case("past-W", 20, 55, 8, 10, True, act % (10, 6, "true", 1)))
    out.append(_case("past-N", 20, 20, 65, 10, False, act % (10, 6, "false", 4), density=0.1))
    out.append(_case("past-H-s4", 61, 30, 6, 4, False, act % (0, 6, "false", 1)))
    out.append(_case("side70", 70, 70, 16, 10, False, act % (10, 6, "false", 1), corners=True))
    # b) every primal_act_kernel<S, LS, DIAG, MA>
    for s in (10, 7):
        for ls in (4, 5, 6):
            for d in (False, True):
                for ma in (1, 4):
                    n = (1 << ls) + (1 if ma == 4 else 0)
                    out.append(_case("inst", 12, 12, n, s, d, act % (10 if s == 10 else 0, ls, _b(d), ma),
                                     corners=True, lanes=str(1 << ls), density=0.3, n_off=1))
    out.append(_case("path-groups", 12, 12, 6, 10, False, act % (10, 6, "false", 1), corners=True,
                     path="groups", density=0.6))
    # c) the host's own lane rule (K = 3: what is pinned here is the packing of many worlds)
    for E, ls in ((4093, 6), (4096, 5), (8188, 5), (8189, 4)):
        out.append(_case("lane-rule", 5, 5, 2, 3, False, act % (0, ls, "false", 1), E=E, K=3, n_off=0, pool=509))
    out.append(_case("lane-rule-s10", 12, 12, 4, 10, False, act % (10, 4, "false", 1), E=8192, K=3, n_off=0,
                     path="groups", pool=509))
    # d) LDS branches
    out.append(_case("lds-attr", 8, 2048, 6, 32, False, act % (0, 6, "false", 1), E=3, corners=True, density=0.45))
    out.append(_case("long-rows", 2, 8000, 5, 3, True, act % (0, 6, "true", 1), density=0.05))
    out.append(_case("limits", 128, 128, 255, 32, True, act % (0, 6, "true", 4), E=3, K=130, corners=True,
                     density=0.1))
    out.append(_case("pin-widened", 120, 120, 8, 10, False, act % (10, 5, "false", 1), lanes="16"))
    # e) small windows, and the first even s above the seq kernel
    out.append(_case("s1", 7, 7, 3, 1, False, act % (0, 6, "false", 1)))
    out.append(_case("s2", 7, 7, 3, 2, True, act % (0, 6, "true", 1)))
    out.append(_case("s12", 20, 20, 6, 12, False, act % (0, 6, "false", 1)))
    # f) through the C ABI with the test's own buffers (K = 130: the chunked launches)
    out.append(_case("abi-seq10", 32, 32, 16, 10, False, seq % (10, "false"), K=130))
    out.append(_case("abi-seq8", 13, 16, 9, 8, True, seq % (8, "true"), K=130))
    out.append(_case("abi-groups", 12, 12, 17, 7, False, act % (0, 4, "false", 4), K=130, corners=True,
                     lanes="16", density=0.3, n_off=1))
    return out


CASES = _cases()


def case_id(c):
    return "%s-%dx%d-N%d-s%d%s-E%d%s" % (c.name, c.H, c.W, c.N, c.s, "-diag" if c.diag else "", c.E,
                                         "-L" + c.lanes if c.lanes else "")


def _seed(c):
    """A fixed seed per case (no hash(): str hashes change from process to process)."""
    return [c.H, c.W, c.N, c.s, int(c.diag), c.E, c.K, int(c.corners), len(c.lanes), len(c.path), c.seed]


@functools.lru_cache(maxsize=None)
def build(c):
    """The worlds and scripts of a case, stacked: grids [E, H, W], starts / goals [E, N, 2],
    and every array of `drive` with a leading E.  Built once per process; read-only."""
    rng = np.random.default_rng(_seed(c))
    n = min(c.E, c.pool) if c.pool else c.E
    worlds, scripts = [], []
    for _ in range(n):
        wd = world(rng, c.H, c.W, c.N, c.density, c.n_off, c.corners, guest=c.s // 2 + 1)
        worlds.append(wd)
        scripts.append(drive(rng, wd, c.K, c.s, c.diag))
    idx = np.arange(c.E) % n
    out = {"grids": np.stack([w["grid"] for w in worlds])[idx],
           "starts": np.stack([w["starts"] for w in worlds])[idx],
           "goals": np.stack([w["goals"] for w in worlds])[idx],
           "distinct": n}
    return _stacked(out, scripts, idx)


def _stacked(out, scripts, idx):
    for key in scripts[0]:
        out[key] = np.stack([sc[key] for sc in scripts])[idx]
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def episode(c, b, calls):
    """The restatement's outputs of a built case's worlds under calls = (ids [E, K] 1-based,
    actions [E, K]) in place of the scripts `build` chose: every array of `drive` with a
    leading E, through `drive` itself (tests/graph_replay_cases.py: further episodes of a
    built case).  Needs every world its own (pool = 0)."""
    assert c.pool == 0 and b["distinct"] == c.E
    ids, acts = calls
    scripts = [drive(None, {"grid": b["grids"][e], "starts": b["starts"][e], "goals": b["goals"][e]},
                     ids.shape[1], c.s, c.diag, calls=(ids[e], acts[e])) for e in range(c.E)]
    return _stacked({}, scripts, np.arange(c.E))


# --------------------------------------------------------------------------- dispatch
def _r16(x):
    return (x + 15) & ~15


def world_lds(H, W, N, s):
    """Bytes of LDS one world takes in primal_act_kernel (`layout` in primal.hip): the padded
    map (+ 4: the realigning read's overrun), the bitmap, the goals plane, 16 bytes per
    agent, three [64] 8-byte arrays and the [5][64] flags."""
    P = max(1, s // 2)
    PW = (W + 2 * P + 3) & ~3
    o = _r16((H + 2 * P) * PW + 4)
    o += _r16(((H * W + 31) // 32) * 4)
    o += _r16(s * s + 4)
    o += 16 * N + 3 * 64 * 8 + 5 * 64
    return _r16(o)


def expected_lanes(H, W, N, s, E, lanes=""):
    """log2 of the lanes per world of primal_act_kernel, as mapfx_primal_create chooses it."""
    D = s * s // 4 if s % 2 == 0 else 1
    ls = 4
    while ls < 6 and (D > 4 * (1 << ls) or N > 4 * (1 << ls)):
        ls += 1
    if lanes in ("16", "32", "64"):
        ls = max(ls, {"16": 4, "32": 5, "64": 6}[lanes])
    else:
        while ls < 6 and -(-E // (64 >> ls)) < 2048:
            ls += 1
    while ls < 6 and (64 >> ls) * world_lds(H, W, N, s) > 65536:
        ls += 1
    return ls


def expected_kernel(H, W, N, s, E, diag, lanes="", path="", obs_aligned=True):
    """The instance mapfx_primal_act launches, as mapfx_last_kernel prints it."""
    P = max(1, s // 2)
    groups = (bool(lanes) or path == "groups" or s % 2 == 1 or s < 4 or s > 10 or N > 64
              or H + 2 * P > 64 or W + 2 * P > 64 or not obs_aligned)
    if not groups:
        return "primal_seq_kernel<%d, %s>" % (s, _b(diag))
    ls = expected_lanes(H, W, N, s, E, lanes)
    ma = 1 if -(-N // (1 << ls)) <= 1 else 4
    return "primal_act_kernel<%d, %d, %s, %d>" % (10 if s == 10 else 0, ls, _b(diag), ma)


# --------------------------------------------------------------------------- comparer
Diff = namedtuple("Diff", "world call field index got want")


def _norm(a):
    a = np.asarray(a)
    if a.dtype == np.float64:
        return np.ascontiguousarray(a).view(np.uint64)
    if a.dtype == np.uint64:
        return a
    return a.astype(np.int64)


def compare(got, want, upto=None):
    """None when every element of the calls < upto (an int, or one per world; None: all K)
    of every output in `got` equals `want`, and pos / past where `got` has them; else the
    first difference in (world, call, field) order as a Diff (call -1 for pos / past, index
    = the flat position inside that world-call's element)."""
    names = [f for f in FIELDS if f in got]
    E, K = np.asarray(want["done"]).shape
    lim = np.full(E, K if upto is None else 0) + (0 if upto is None else np.asarray(upto))
    live = np.arange(K)[None, :] < lim[:, None]
    bad = np.zeros((E, K, len(names)), bool)
    pairs = {}
    for i, f in enumerate(names):
        g, w = _norm(got[f]).reshape(E, K, -1), _norm(want[f]).reshape(E, K, -1)
        pairs[f] = (g, w)
        bad[:, :, i] = (g != w).any(-1) & live
    first = None
    if bad.any():
        e, k, i = np.unravel_index(int(np.argmax(bad)), bad.shape)
        g, w = pairs[names[i]]
        j = int(np.argmax(g[e, k] != w[e, k]))
        first = Diff(int(e), int(k), names[i], j, int(g[e, k, j]), int(w[e, k, j]))
    for f in ("pos", "past"):
        if f not in got or got[f] is None:
            continue
        g, w = _norm(got[f]).reshape(E, -1), _norm(want[f]).reshape(E, -1)
        rows = np.flatnonzero((g != w).any(-1))
        if len(rows) and (first is None or rows[0] < first.world):
            e = int(rows[0])
            j = int(np.argmax(g[e] != w[e]))
            first = Diff(e, -1, f, j, int(g[e, j]), int(w[e, j]))
    return first
