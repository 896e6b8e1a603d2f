"""Cases, scripted episodes, the dispatch rule and the comparer of the MARL_PARTIAL plain-step
tests (tests/test_partial_step_cases.py on the CPU, tests/test_gpu_partial_step_shapes.py on
the device).  TEST INFRASTRUCTURE ONLY; no test lives here, and nothing here imports mapfx.

Every expected value is the restatement's (oracle/partial_oracle.py: PartialEnvState,
bfs_goal_dist), which the mp_* goldens pin to the reference.  The reference itself raises
on non-square maps (MARL_PARTIAL_ENV.__create_grid), so the non-square cases -- most of
the table: a square map hides every H / W mix-up -- pin the kernels to the restatement's
semantics only.  Instances stay inside the reference's domain: one free component, no
agent starting on an obstacle.

`expected_step_kernel`, `expected_bfs_kernel` and `expected_geometry` restate the host side
of csrc/partial.hip (pick(), launch(), wg_apl, mapfx_partial_goal_dist, layout()'s LDS
sums); the kernels come back as (name, template arguments without spaces), the form
`kernel_args` reduces a mapfx_last_kernel string to.

Random actions are the base of every episode ([T, E, N]; limit = T - 2, so every case runs
two steps past its limit).  On top of them `build` scripts, per case:
  env 0      the stacked-swap gadget (N >= 3): agent 0 on Y, agents 1 and 2 on two other
             neighbours of Y's neighbour X; step 0 both move into X (node = 1, 1), step 1
             agent 0 moves to X and both move to Y: edge = [2, 1, 1].  N = 2: the two movers
             alone (a node collision).
  env 1      completion: every goal one free move from its start, all stay, then all make
             that move at a step t < limit (the bonus below the limit), then random actions
             on a terminated env.
  env 2      run-out: the same with the move at t = limit: the bonus at t = limit,
             limit + 1 and limit + 2 (LUT entries past the limit).
  six roles  an agent on each of the four borders stepping out of the grid, one stepping
             into a free-standing obstacle, one that reaches its goal at step 0 and stays on
             it at step 1.  Agents 3..8 of env 0 when N >= 9, else spread over envs 3...
"""
from __future__ import annotations

import functools
import re
import types
from collections import namedtuple

import numpy as np

from oracle.partial_oracle import PartialEnvState, bfs_goal_dist

KW = dict(move_reward=-0.01, stay_reward=-0.02, stay_goal_reward=0.5, node_collide_reward=-1.5,
          edge_collide_reward=-2, env_collide_reward=-3, complete_reward=1000, complete_fac=1.5,
          gamma=0.99)
STEPS = ((-1, 0), (1, 0), (0, -1), (0, 1))      # action 0 up, 1 down, 2 left, 3 right
SIDES = ("top", "bottom", "left", "right")
FAST_PAIRS = ((5, 16), (5, 8), (5, 32), (3, 16), (7, 16))     # (WIN, LF) of pick()
VARIANTS = 5          # distinct maps a per-env case cycles through


# --------------------------------------------------------------------------- maps
def sprinkle(H, W, variant=0):
    """An open H x W map with a few single-cell obstacles off the border, no two of them
    adjacent (diagonals included): the free cells stay one component."""
    rng = np.random.default_rng([H, W, variant, 7])
    g = np.zeros((H, W), np.int8)
    cells = [(r, c) for r in range(1, H - 1) for c in range(1, W - 1)]
    placed = []
    for k in rng.permutation(len(cells)):
        r, c = cells[k]
        if all(max(abs(r - pr), abs(c - pc)) >= 2 for pr, pc in placed):
            placed.append((r, c))
            g[r, c] = -1
            if len(placed) == max(2, min(12, H * W // 40)):
                break
    return g


def block(H, W, variant=0):
    """All obstacle but a 20 x 20 block (three obstacles inside), one full row and one full
    column through it: the free cells touch all four borders and the restatement's BFS,
    whose cost per level is the whole grid, has ~H + W levels of few cells."""
    g = np.full((H, W), -1, np.int8)
    r0, c0 = (H - 20) // 2 + variant, (W - 20) // 3 + 2 * variant
    g[r0:r0 + 20, c0:c0 + 20] = 0
    g[r0 + 10, :] = 0
    g[:, c0 + 10] = 0
    for dr, dc in ((3, 5), (8, 14), (15, 7)):
        g[r0 + dr, c0 + dc] = -1
    return g


BUILDERS = {"sprinkle": sprinkle, "block": block}


@functools.lru_cache(maxsize=None)
def grid_of(builder, H, W, variant):
    g = BUILDERS[builder](H, W, variant)
    free = np.argwhere(g == 0)
    reach = bfs_goal_dist(g, free[0]) >= 0
    assert reach.sum() == len(free), "the free cells must be one component"
    g.setflags(write=False)
    return g


_TABLES = {}


def goal_table(builder, H, W, variant, goal):
    """bfs_goal_dist of one goal cell, computed once per (map, goal) and shared."""
    key = (builder, H, W, variant, int(goal[0]), int(goal[1]))
    if key not in _TABLES:
        t = bfs_goal_dist(grid_of(builder, H, W, variant), goal)
        t.setflags(write=False)
        _TABLES[key] = t
    return _TABLES[key]


# --------------------------------------------------------------------------- cases
# dtype: the action dtype of the case's matrix run; shared: one map for all envs, else
# env e has variant e % VARIANTS of it
Case = namedtuple("Case", "name H W builder N win K E T shared dtype")


def _c(name, H, W, N, win, K, E, T=6, builder="sprinkle", shared=False, dtype="int64"):
    return Case(name, H, W, builder, N, win, K, E, T, shared, dtype)


def limit_of(c):
    return c.T - 2


def _cases():
    out = []
    # --- fast plain instances partial_kernel<WIN, 5, LF, GDE, false>: per (WIN, LF) pair u8
    # tables with / without the LDS sqrt table (2 (max(H, W) - 1)^2 < 512: sides <= 16),
    # int16 with / without, int32.  Per env (mapfx_partial_create): 2 map images of
    # (H + 2P) * round4(round4(P) + W + P) bytes + the bitmap + L * 64, EPW = 64 / L envs per
    # wave, 4 waves per block.  Windows 3 and 5 stage whole waves (stage_lanes 64: <= 34.8 KB
    # per wave); at window 7 four stage images of 16 * 163 * 4 + 16 bytes pass 40 KB, so two
    # alias the second map image onwards: half waves (32); the int32 maps take ~75 KB per
    # env: EPW 1, no staging (rows stored straight to HBM), 2 waves per block.  E: more than
    # one block, a partial last wave and a partial last block.
    #                 u8+table   u8         int16+table int16      int32 (block map)
    shapes = {(5, 16): ((11, 13), (7, 33), (16, 16), (21, 19), (129, 256)),
              (5, 8): ((13, 11), (3, 80), (16, 16), (19, 21), (256, 129)),
              (5, 32): ((12, 13), (33, 7), (16, 16), (21, 19), (129, 256)),
              (3, 16): ((13, 12), (80, 3), (16, 16), (19, 21), (256, 129)),
              (7, 16): ((11, 13), (7, 33), (16, 16), (21, 19), (129, 256))}
    agents = {16: (9, 16, 12, 13, 11), 8: (5, 8, 6, 7, 5), 32: (17, 32, 24, 29, 17)}
    envs = {16: 21, 8: 37, 32: 11}
    tags = ("u8t", "u8", "i16t", "i16", "i32")
    dts = ("int64", "int8", "int32")
    for p, (win, L) in enumerate(FAST_PAIRS):
        for k, (H, W) in enumerate(shapes[(win, L)]):
            i32 = tags[k] == "i32"
            out.append(_c("fast-w%d-l%d-%s" % (win, L, tags[k]), H, W, agents[L][k], win, 5,
                          (5 if L == 8 else 3) if i32 else envs[L], builder="block" if i32 else "sprinkle",
                          shared=(p + k) % 2 == 0, dtype=dts[(p + k) % 3]))
    # half-wave staging (stage_lanes 32): 4 envs of 64 x 60 take 42.6 KB, past the 40 KB of
    # whole-wave staging; 3 waves per block
    out.append(_c("fast-half-64x60", 64, 60, 16, 5, 5, 14, dtype="int32"))
    # --- generic instances partial_kernel<WIN, 0, 0> on the plain path: every window, lane
    # groups 1, 2, 4, 8, 16 and 64; K above N (rows of -1), K != 5; u8 and int16 tables, the
    # 256-thread BFS with int16 tables (70 x 9)
    out.append(_c("gen-w0-n2", 9, 14, 2, 0, 5, 131, dtype="int8"))          # L 2: 128 envs per block
    out.append(_c("gen-w1-n1", 14, 9, 1, 1, 5, 259, shared=True))           # L 1: 256 envs per block
    out.append(_c("gen-w3-n6", 17, 20, 6, 3, 5, 37, dtype="int32"))         # win 3 is fast only at L 16
    out.append(_c("gen-w5-n3", 10, 13, 3, 5, 5, 67, shared=True))           # L 4: 64 envs per block
    out.append(_c("gen-w7-n12-k3", 70, 9, 12, 7, 3, 21, dtype="int8"))      # K != 5
    out.append(_c("gen-w9-n40-k4", 15, 12, 40, 9, 4, 6, shared=True, dtype="int32"))  # L 64: 1 env per wave
    # --- workgroup kernel partial_wg_kernel<WIN, APL>: N = 70 / 300 / 600 (APL 1 / 2 / 4; 600
    # leaves the fourth register row of every thread empty) on 30 x 34 and 34 x 30, and per
    # second window a map with a side above 256 and N = 4 (the huge BFS: int16 tables on
    # 260 x 6, int32 on 130 x 260).  T = 4, limit 2: the completion env ends at t = 1
    for k, win in enumerate((0, 1, 3, 5, 7, 9)):
        H, W = ((30, 34), (34, 30))[k % 2]
        K = 5 if k % 3 else 3
        if k % 2 == 0:
            out.append(_c("wg-w%d-n70" % win, H, W, 70, win, K, 3, T=4, dtype=dts[k % 3]))
        elif win == 5:
            out.append(_c("wg-w5-wide130x260", 130, 260, 4, win, K, 5, T=4, builder="block", shared=True))
        else:
            out.append(_c("wg-w%d-tall260x6" % win, 260, 6, 4, win, K, 5, T=4, dtype=dts[k % 3]))
        out.append(_c("wg-w%d-n300" % win, W, H, 300, win, K, 3, T=4, shared=True, dtype=dts[(k + 1) % 3]))
        out.append(_c("wg-w%d-n600" % win, H, W, 600, win, K, 3, T=4, shared=True, dtype=dts[(k + 2) % 3]))
    # --- the cases of the action-dtype, masked-reset, observe and error-word tests: T = 8
    # (rows 1..8 of an int8 [9, E, N] tensor with E * N odd start at every residue mod 8)
    out.append(_c("act-fast", 21, 19, 9, 5, 5, 21, T=8))
    out.append(_c("act-gen", 10, 13, 3, 5, 5, 67, T=8))
    out.append(_c("act-wg", 19, 23, 71, 3, 5, 5, T=8))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def case_id(c):
    return "%s-%dx%d-N%d-E%d" % (c.name, c.H, c.W, c.N, c.E)


# --------------------------------------------------------------------------- dispatch
def _r4(x):
    return (x + 3) & ~3


def _r16(x):
    return (x + 15) & ~15


def is_big(H, W, N):
    """The workgroup-per-env path: N > 64 or a side > 256."""
    return N > 64 or H > 256 or W > 256


def lane_group(N):
    L = 1
    while L < N:
        L <<= 1
    return L


def table_bytes(H, W):
    """mapfx_partial_goal_dist_elem_size: u8 up to 255 cells, int16 up to 32767, else int32."""
    return 1 if H * W <= 255 else 4 if H * W > 32767 else 2


def family(c):
    if is_big(c.H, c.W, c.N):
        return "workgroup"
    return "fast" if c.K == 5 and (c.win, lane_group(c.N)) in FAST_PAIRS else "generic"


def expected_step_kernel(c):
    """pick() / launch(): the plain step's instance."""
    fam = family(c)
    if fam == "workgroup":
        apl = -(-c.N // 256)                                    # wg_apl
        return ("partial_wg_kernel", "%d,%d" % (c.win, 1 if apl <= 1 else 2 if apl <= 2 else 4))
    if fam == "fast":
        gde = {1: 1, 2: 2, 4: 0}[table_bytes(c.H, c.W)]
        return ("partial_kernel", "%d,5,%d,%d,false" % (c.win, lane_group(c.N), gde))
    return ("partial_kernel", "%d,0,0,0,true" % c.win)          # <WIN, 0, 0> and its defaults


def expected_bfs_kernel(c):
    """mapfx_partial_goal_dist: the BFS instance (the table's C++ type as the demangler prints it)."""
    typ = {1: "unsignedchar", 2: "short", 4: "int"}[table_bytes(c.H, c.W)]
    if c.H > 256 or c.W > 256:
        return ("partial_bfs_huge_kernel", typ)
    if c.H <= 64 and c.W <= 64:
        return ("partial_bfs_kernel", typ)
    return ("partial_bfs_big_kernel", typ)


ALL_STEP_KERNELS = (
    {("partial_kernel", "%d,5,%d,%d,false" % (w, L, g)) for w, L in FAST_PAIRS for g in (1, 2, 0)}
    | {("partial_kernel", "%d,0,0,0,true" % w) for w in (0, 1, 3, 5, 7, 9)}
    | {("partial_wg_kernel", "%d,%d" % (w, a)) for w in (0, 1, 3, 5, 7, 9) for a in (1, 2, 4)})
ALL_BFS_KERNELS = {("partial_bfs_kernel", "unsignedchar"), ("partial_bfs_kernel", "short"),
                   ("partial_bfs_big_kernel", "unsignedchar"), ("partial_bfs_big_kernel", "short"),
                   ("partial_bfs_big_kernel", "int"), ("partial_bfs_huge_kernel", "short"),
                   ("partial_bfs_huge_kernel", "int")}


def kernel_args(printed):
    """(name, template arguments without spaces) of a mapfx_last_kernel string."""
    m = re.search(r"(partial_(?:wg_|bfs_|bfs_big_|bfs_huge_)?kernel)<([^>]*)>", printed)
    return (m.group(1), m.group(2).replace(" ", "")) if m else None


def expected_geometry(c):
    """layout()'s sums (csrc/partial.hip) for a case (anything with H, W, N, win, K): bytes per env,
    envs per wave, the staging group (64: whole wave, 32: half waves, 0: rows stored
    straight to HBM), waves per block, a wave's LDS and whether the per-wave float32 sqrt
    table exists.  The workgroup path (big) keeps no map in LDS: EPW = wpb = 1."""
    H, W, N, win, K = c.H, c.W, c.N, c.win, c.K
    L = lane_group(N)
    P = max(1, win // 2)
    pitch = _r4(_r4(P) + W + P)
    map_env = _r16((H + 2 * P) * pitch)
    bits_env = _r16(((H * W + 31) // 32) * 4 + 4)
    per_env = 2 * map_env + bits_env + _r16(L * 12 * 4) + 2 * _r16(L * 8)
    big = is_big(H, W, N)
    EPW = 1 if big else 64 // L
    while EPW > 1 and EPW * per_env > 64 * 1024:
        EPW -= 1
    off = EPW * per_env
    sq_max = 2 * (max(H, W) - 1) ** 2
    if sq_max < 512:
        off += _r16((sq_max + 1) * 4)
    stage_env = _r16(L * (2 * win * win + 13 * K) * 4 + 16)
    stage_lanes = 0
    if K == 5 and win in (3, 5, 7) and 8 <= L <= 32:
        for G in (64, 32):
            need = max(off, EPW * map_env + min(EPW, G // L) * stage_env)
            if need <= (40 if G == 64 else 64) * 1024:
                stage_lanes, off = G, need
                break
    lds = _r16(off)
    wpb = 1 if big else 4
    while wpb > 1 and wpb * lds > 160 * 1024:
        wpb -= 1
    return dict(per_env=per_env, EPW=EPW, stage_lanes=stage_lanes, wpb=wpb, lds=lds,
                sqrt_table=sq_max < 512, big=big)


# --------------------------------------------------------------------------- instances
def _nbrs(g, p):
    """(action, cell) of the on-grid neighbours of p."""
    H, W = g.shape
    return [(a, (p[0] + dr, p[1] + dc)) for a, (dr, dc) in enumerate(STEPS)
            if 0 <= p[0] + dr < H and 0 <= p[1] + dc < W]


def _pick(rng, cells, used):
    cells = [p for p in cells if p not in used]
    assert cells, "no cell left"
    return cells[int(rng.integers(len(cells)))]


def _free_list(g):
    return [(int(r), int(c)) for r, c in np.argwhere(g == 0)]


def _gadget(rng, g, N, agents, used):
    """The stacked-swap gadget (module docstring): agents[a] = (start, goal, {step: action})."""
    free = _free_list(g)
    spots = [x for x in free if sum(g[q] == 0 for _, q in _nbrs(g, x)) >= 3]
    X = spots[int(rng.integers(len(spots)))]
    around = [(a, q) for a, q in _nbrs(g, X) if g[q] == 0]
    order = rng.permutation(len(around))
    (aY, Y), (aA, A), (aB, B) = (around[k] for k in order[:3])
    far = [p for p in free if abs(p[0] - X[0]) + abs(p[1] - X[1]) > 2]
    movers = ((A, aA), (B, aB))
    first = 0
    if N >= 3:      # agent 0 waits on Y, then swaps with both
        agents[0] = (Y, X, {0: 4, 1: aY ^ 1})
        used |= {Y}
        first = 1
    for k, (cell, a) in enumerate(movers):      # a ^ 1: towards X; aY: from X to Y
        goal = _pick(rng, far, {agents[i][1] for i in agents})
        agents[first + k] = (cell, goal, {0: a ^ 1, 1: aY})
        used |= {cell}


def _one_move_env(rng, g, N, step):
    """Every agent's goal one free move from its start (starts distinct, goals distinct);
    all stay before `step` and make the move at `step`."""
    free = _free_list(g)
    agents, starts, goals = {}, set(), set()
    for k in rng.permutation(len(free)):
        s = free[k]
        opts = [(a, q) for a, q in _nbrs(g, s) if g[q] == 0 and q not in goals]
        if not opts:
            continue
        a, q = opts[int(rng.integers(len(opts)))]
        script = {t: 4 for t in range(step)}
        script[step] = a
        agents[len(agents)] = (s, q, script)
        starts.add(s)
        goals.add(q)
        if len(agents) == N:
            return agents
    raise AssertionError("not enough agents with a free move")


def _role(rng, g, role, used, goals):
    """(start, goal, script) of one of the six roles."""
    H, W = g.shape
    free = _free_list(g)
    if role in SIDES:
        a = SIDES.index(role)
        line = [p for p in free if (p[0] == 0, p[0] == H - 1, p[1] == 0, p[1] == W - 1)[a]]
        s = _pick(rng, line, used)
        return s, _pick(rng, free, goals | {s}), {0: a}
    if role == "obstacle":
        opts = [(p, a) for p in free if p not in used for a, q in _nbrs(g, p) if g[q] != 0]
        s, a = opts[int(rng.integers(len(opts)))]
        return s, _pick(rng, free, goals | {s}), {0: a}
    opts = [(p, a, q) for p in free if p not in used for a, q in _nbrs(g, p)
            if g[q] == 0 and q not in goals]
    s, a, q = opts[int(rng.integers(len(opts)))]
    return s, q, {0: a, 1: 4}       # "stayer": on its goal after step 0, stays at step 1


ROLES = SIDES + ("obstacle", "stayer")


def role_slots(N):
    """(env, agent) of the six roles."""
    if N >= 9:
        return [(0, 3 + k) for k in range(6)]
    return [(3 + k // N, k % N) for k in range(6)]


def min_envs(N):
    return max(3, max(e for e, _ in role_slots(N)) + 1)


class Ref(PartialEnvState):
    """PartialEnvState that keeps the reward of its last step (None after a reset)."""
    last_reward = None

    def reset(self):
        super().reset()
        self.last_reward = None

    def step(self, actions):
        r, term = super().step(actions)
        self.last_reward = float(r)
        return r, term

    def refuse(self):
        """What the kernels do with an action outside 0..4 (the reference asserts): the env
        is left as it is, its reward is 0.0."""
        self.last_reward = 0.0


def params(c):
    return dict(KW, obs_window=c.win, obs_knn_agents=c.K, episode_limit=limit_of(c))


def make_refs(c, b, limit=None):
    """Fresh restatement envs of a built case (the goal tables are shared, never modified);
    `limit`: an episode_limit in place of the case's own."""
    kw = params(c) if limit is None else dict(params(c), episode_limit=limit)
    return [Ref(b["grids"][0 if c.shared else e], b["starts"][e], b["goals"][e],
                goal_dist=[b["goal_dist"][e, a] for a in range(c.N)], **kw)
            for e in range(c.E)]


def episode(c, b, actions, count=None, limit=None, resets=None):
    """The restatement's episode of the instance `b` (grids, starts, goals, goal_dist of
    `build`) under `actions` [steps, E, N]: the loop `build` itself runs, and what
    tests/graph_replay_cases.py runs for further episodes of a built case.  Returns the
    snapshots in call order: after reset(), then after every step.  limit: an episode_limit
    in place of the case's own.  resets = {k: mask [E]}: reset(env_mask) of the masked envs
    between step k - 1 and step k, its snapshot (no env's reward is a step's) inserted
    there.  count = (bumps [steps, 5], stays [steps]): filled for the coverage test."""
    assert actions.shape[1:] == (c.E, c.N), actions.shape
    refs = make_refs(c, b, limit)
    snaps = [snapshot(refs)]
    for t in range(len(actions)):
        if resets is not None and t in resets:
            for e in np.flatnonzero(resets[t]):
                refs[e].reset()
            for r in refs:
                r.last_reward = None
            snaps.append(snapshot(refs))
        for e, r in enumerate(refs):
            occ = r.occ() if count is not None else None
            for i, a in enumerate(actions[t, e] if count is not None else ()):
                if r.done[i]:
                    continue
                if a == 4:
                    count[1][t] += bool(r.at_goal[i])
                    continue
                cand = (r.pos[i][0] + STEPS[a][0], r.pos[i][1] + STEPS[a][1])
                if not r._valid(cand):
                    count[0][t, a] += 1
                elif r._is_obstacle(occ, cand):
                    count[0][t, 4] += 1
            r.step(actions[t, e])
        snaps.append(snapshot(refs))
    for s in snaps:
        for v in s.values():
            v.setflags(write=False)
    return snaps


def _seed(c):
    return [c.H, c.W, c.N, c.win, c.K, c.E, c.T, int(c.shared), len(c.name)]


@functools.lru_cache(maxsize=None)
def build(c):
    """A case's maps, instances, actions and the restatement's episode, built once per
    process and read-only: grids [1 | E, H, W], starts / goals [E, N, 2], goal_dist
    [E, N, H * W], actions [T, E, N], snaps[0] after reset() and snaps[t + 1] after step t
    (`snapshot`), and what the coverage test counts -- per step the env collisions by kind
    (bumps [T, 5]: four sides, obstacle) and the stay-on-goal rewards (stays [T])."""
    assert c.T >= 4 and c.E >= min_envs(c.N), c
    rng = np.random.default_rng(_seed(c))
    limit, N, E, T = limit_of(c), c.N, c.E, c.T
    variant = (lambda e: 0) if c.shared else (lambda e: e % VARIANTS)
    grids = [grid_of(c.builder, c.H, c.W, v) for v in range(1 if c.shared else min(E, VARIANTS))]
    actions = rng.integers(0, 5, size=(T, E, N))
    starts = np.zeros((E, N, 2), np.int32)
    goals = np.zeros((E, N, 2), np.int32)
    slots = role_slots(N)
    for e in range(E):
        g = grids[variant(e)]
        agents, used = {}, set()
        if e == 1:
            agents = _one_move_env(rng, g, N, min(1, limit - 2))
        elif e == 2:
            agents = _one_move_env(rng, g, N, limit - 1)
        else:
            if e == 0 and N >= 2:
                _gadget(rng, g, N, agents, used)
            for (re_, ag), role in zip(slots, ROLES):
                if re_ == e:
                    agents[ag] = _role(rng, g, role, used, {agents[i][1] for i in agents})
                    used.add(agents[ag][0])
            free = _free_list(g)
            for ag in range(N):
                if ag not in agents:
                    s = _pick(rng, free, used)
                    used.add(s)
                    agents[ag] = (s, _pick(rng, free, {agents[i][1] for i in agents} | {s}), {})
        for ag in range(N):
            s, q, script = agents[ag]
            starts[e, ag], goals[e, ag] = s, q
            for t, a in script.items():
                if t < T:
                    actions[t, e, ag] = a
    goal_dist = np.stack([np.stack([goal_table(c.builder, c.H, c.W, variant(e), goals[e, a])
                                    for a in range(N)]) for e in range(E)])
    b = {"grids": np.stack([grids[variant(e)] for e in range(1 if c.shared else E)]), "starts": starts, "goals": goals, "goal_dist": goal_dist,
         "actions": actions}
    bumps, stays = np.zeros((T, 5), np.int64), np.zeros(T, np.int64)
    snaps = episode(c, b, actions, count=(bumps, stays))
    b.update(snaps=snaps, bumps=bumps, stays=stays)
    for v in list(b.values()) + [x for s in snaps for x in s.values()]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return b


# --------------------------------------------------------------------------- comparer
FIELDS = ("reward", "terminated", "pos", "steps", "at_goal", "done", "goal_cost", "node", "edge",
          "t", "total_coll", "obs", "state", "avail", "pdist", "pnbr")
STATE_ARRAYS = ("pos", "steps", "at_goal", "done", "goal_cost", "node", "edge", "t", "terminated",
                "total_coll", "pdist", "pnbr")
Diff = namedtuple("Diff", "call field env index got want")


def snapshot(refs):
    """Everything `compare` looks at, from the restatement envs: the state arrays, obs /
    state as float32, avail as the 5-bit mask, reward as fp64 bits (reward_ok: the env's
    last call was a step), pdist = the goal table at each agent's cell, pnbr = the table at
    its four neighbours (pnbr_ok: the neighbour is on the grid)."""
    E, N = len(refs), refs[0].n
    h, w = refs[0].h, refs[0].w
    ints = lambda f: np.array([f(r) for r in refs], np.int64)  # noqa: E731
    pos = ints(lambda r: r.pos).reshape(E, N, 2)
    s = {"pos": pos, "steps": ints(lambda r: r.steps), "at_goal": ints(lambda r: r.at_goal),
         "done": ints(lambda r: r.done), "goal_cost": ints(lambda r: r.goal_cost),
         "node": ints(lambda r: r.node), "edge": ints(lambda r: r.edge), "t": ints(lambda r: r.t),
         "terminated": ints(lambda r: r.terminated), "total_coll": ints(lambda r: r.total_collisions),
         "obs": np.stack([r.obs() for r in refs]).astype(np.float32),
         "state": np.stack([r.state() for r in refs]).astype(np.float32),
         "avail": (np.stack([r.avail() for r in refs]).astype(np.int64) << np.arange(5)).sum(-1),
         "reward": np.array([0.0 if r.last_reward is None else r.last_reward for r in refs],
                            np.float64).view(np.uint64),
         "reward_ok": np.array([r.last_reward is not None for r in refs])}
    pdist = np.zeros((E, N), np.int64)
    pnbr = np.zeros((E, N, 4), np.int64)
    ok = np.zeros((E, N, 4), bool)
    for e, r in enumerate(refs):
        for i, (y, x) in enumerate(r.pos):
            tab = r.goal_dist[i]
            pdist[e, i] = tab[y * w + x]
            for a, (dy, dx) in enumerate(STEPS):
                if 0 <= y + dy < h and 0 <= x + dx < w:
                    ok[e, i, a] = True
                    pnbr[e, i, a] = tab[(y + dy) * w + x + dx]
    s.update(pdist=pdist, pnbr=pnbr, pnbr_ok=ok)
    return s


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _bits(a):
    a = np.ascontiguousarray(_host(a))
    if a.dtype == np.float64:
        return a.view(np.uint64)
    if a.dtype == np.float32:
        return a.view(np.uint32).astype(np.int64)
    return a if a.dtype == np.uint64 else a.astype(np.int64)


def carries_pnbr(batch):
    """pnbr is kept by the wave kernel alone, for u8 / int16 tables (the workgroup kernel
    neither reads nor writes it)."""
    return getattr(batch, "pnbr", None) is not None and not is_big(batch.H, batch.W, batch.N)


def state_arrays(batch):
    """Host copies of every state array of a batch (pnbr where it is carried)."""
    return {f: _host(getattr(batch, f)).copy() for f in STATE_ARRAYS
            if f != "pnbr" or carries_pnbr(batch)}


def compare(batch, out, refs, t):
    """None when the batch's state arrays and the outputs `out` (reward, obs, state, avail)
    equal the restatement's -- `refs`: the Ref envs, or a `snapshot` of them -- else the
    first difference in FIELDS order as a Diff (call = t, index = the flat position inside
    the env's element).  Rewards as fp64 bits where the env's last call was a step; the
    off-grid entries of pnbr are unspecified (include/mapfx_partial.h) and skipped."""
    want = refs if isinstance(refs, dict) else snapshot(refs)
    E = len(want["t"])
    for f in FIELDS:
        if f == "pnbr" and not carries_pnbr(batch):
            continue
        src = out[f] if f in ("reward", "obs", "state", "avail") else getattr(batch, f)
        g, w = _bits(src).reshape(E, -1), _bits(want[f]).reshape(E, -1)
        assert g.shape == w.shape, (f, g.shape, w.shape)
        bad = g != w
        if f == "reward":
            bad &= want["reward_ok"][:, None]
        if f == "pnbr":
            bad &= want["pnbr_ok"].reshape(E, -1)
        if bad.any():
            e, j = (int(v) for v in np.argwhere(bad)[0])
            return Diff(t, f, e, j, int(g[e, j]), int(w[e, j]))
    return None


def as_device(c, snap, junk=0x5A5A):
    """(batch, out) holding a snapshot in the device's dtypes, as numpy arrays: what
    `compare` is given on the CPU.  The off-grid pnbr entries hold `junk`."""
    dt = {"pos": np.int32, "steps": np.int32, "at_goal": np.uint8, "done": np.uint8,
          "goal_cost": np.int32, "node": np.uint8, "edge": np.int32, "t": np.int32,
          "terminated": np.uint8, "total_coll": np.int32, "pdist": np.int32}
    batch = types.SimpleNamespace(H=c.H, W=c.W, N=c.N,
                                  **{f: snap[f].astype(d) for f, d in dt.items()})
    batch.pnbr = None if table_bytes(c.H, c.W) == 4 else \
        np.where(snap["pnbr_ok"], snap["pnbr"], junk).astype(np.int16)
    out = {"reward": snap["reward"].view(np.float64).copy(), "obs": snap["obs"].copy(),
           "state": snap["state"].copy(), "avail": snap["avail"].astype(np.uint8)}
    return batch, out
