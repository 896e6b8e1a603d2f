"""Counter-based splitmix64 streams shared by the host (numpy) and the device.

The device versions live in csrc/internal.h (`splitmix64`) and csrc/mapfx.hip (`gen_action`); the
functions here are bit-identical numpy restatements used to build synthetic
instances on the host and to check the device action generator.  Every stream
is keyed by the GLOBAL env id, so an env's inputs do not depend on how envs are
sharded over ranks.
"""
from __future__ import annotations

import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
K_ENV = np.uint64(0xD1B54A32D192ED03)
K_T = np.uint64(0xABC98388FB8FAC03)
K_AGENT = np.uint64(0x8CB92BA72F3D8DD7)
K_CELL = np.uint64(0x9E6C63D0676A9A99)
K_STREAM = np.uint64(0xF1357AEA2E62A9C5)

# Streams of the device PRIMAL world generator (mapfx_primal_generate, csrc/primal.hip);
# mapfx.maps uses 1..3.  The obstacle stream of redraw attempt t is STREAM_GEN_OBST + t,
# t = 0..32.
STREAM_GEN_WORLD, STREAM_GEN_OBST, STREAM_GEN_START, STREAM_GEN_GOAL = 0x100, 0x200, 0x300, 0x400
# Streams of the device MARL_PARTIAL scenario draw (mapfx_partial_draw, csrc/partial.hip)
STREAM_SCEN_FILE, STREAM_SCEN_LINE = 0x500, 0x600
# Stream of the device action selection (mapfx_select_actions, csrc/runner.hip)
STREAM_SELECT = 0x700
SELECT_MODES = {"epsilon_greedy": 0, "multinomial": 1}   # include/mapfx_runner.h MAPFX_SELECT_*


def splitmix64(x):
    """Vectorised splitmix64 finaliser on uint64 arrays (wrapping arithmetic)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _mul(a, k):
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.uint64) * k


def gen_actions(seed, env_ids, t_ids, n_agents):
    """Actions in {0..4}: splitmix64(seed ^ env*K_ENV ^ t*K_T ^ agent*K_AGENT) % 5.

    Same formula as `gen_action` in csrc/mapfx.hip / `mapfx_action` in
    include/mapfx.h.  Returns int8 [len(t_ids), len(env_ids), n_agents].
    """
    env = np.asarray(env_ids, dtype=np.int64).astype(np.uint64)[None, :, None]
    t = (np.asarray(t_ids, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint64)[:, None, None]
    ag = np.arange(n_agents, dtype=np.uint64)[None, None, :]
    k = np.uint64(seed) ^ _mul(env, K_ENV) ^ _mul(t, K_T) ^ _mul(ag, K_AGENT)
    return (splitmix64(k) % np.uint64(5)).astype(np.int8)


def partial_policy_actions(seed, env_ids, t, eps_q, avail, pd, d):
    """The on-device policy of mapfx_partial_rollout (include/mapfx_partial.h), restated for
    one step.

    u = splitmix64(seed ^ gid*K_ENV ^ t*K_T ^ a*K_AGENT) is `gen_actions`' own word: where
    (u >> 32) < eps_q the action is u % 5 (eps_q = 2**32: gen_actions exactly); elsewhere the
    agent descends its goal distances: with ok_m = bit m of the PRE-step avail mask and
    d[m] >= 0, it stays (4) when pd < 0 or no ok_m has d[m] < pd, else takes the lowest m
    among the ok_m of minimal d[m].

    env_ids [E] global env ids, t the step's counter (t0 + k), avail [E, N] 5-bit masks,
    pd [E, N] the goal distance of each agent's cell, d [E, N, 4] those of its neighbours
    (up, down, left, right; any value where the avail bit is clear).  Returns int8 [E, N].
    """
    avail = np.asarray(avail, dtype=np.int64)
    pd = np.asarray(pd, dtype=np.int64)
    d = np.asarray(d, dtype=np.int64)
    E, N = pd.shape
    env = np.asarray(env_ids, dtype=np.int64).astype(np.uint64)[:, None]
    ag = np.arange(N, dtype=np.uint64)[None, :]
    tt = np.uint64(int(t) & 0xFFFFFFFF)
    u = splitmix64(np.uint64(seed) ^ _mul(env, K_ENV) ^ _mul(tt, K_T) ^ _mul(ag, K_AGENT))
    explore = (u >> np.uint64(32)) < np.uint64(eps_q)               # eps_q may be 2**32
    ok = (((avail[..., None] >> np.arange(4)) & 1) == 1) & (d >= 0)
    big = np.iinfo(np.int64).max
    dm = np.where(ok, d, big)
    best = dm.min(-1)
    greedy = np.where((pd >= 0) & (best < pd), dm.argmin(-1), 4)    # argmin: the lowest m of a tie
    return np.where(explore, (u % np.uint64(5)).astype(np.int64), greedy).astype(np.int8)


PIBT_STEPS = ((-1, 0), (1, 0), (0, -1), (0, 1))      # move 0 up, 1 down, 2 left, 3 right
# what partial_policy_pibt_actions(stats=True) counts, in this order
PIBT_STATS = ("push", "push_failed", "depth3", "skip_claimed", "skip_parent", "skip_multi",
              "explore_top", "explore_pushed", "forced_stay")


def partial_policy_pibt_actions(seed, env_ids, t, eps_q, avail, pd, d, pos, stats=False):
    """The collision-free on-device policy (MAPFX_POLICY_PIBT of include/mapfx_partial.h:
    one-step priority inheritance with backtracking), restated for one step.  This function
    is the rule's definition.

    u, explore = (u >> 32) < eps_q and ok_m = bit m of the PRE-step avail mask and d[m] >= 0
    are `partial_policy_actions`' own.  Candidates of agent a, as (move, cell):
      pd < 0                         stay alone
      called at top level, explore   [u % 5 if it is a move m < 4 with ok_m], then stay
      otherwise (a pushed agent too) the ok_m moves and stay as (pd, 4), ascending by (d, m)
    Agents are planned in ascending (pd == 0, (a - t) mod N), t as an unsigned 32-bit value;
    one still undecided at its turn runs PLAN(a, none).  PLAN(a, parent), per candidate
    (m, v) in order: skip v when it is claimed; when it is the parent's cell (no swap); when
    m != 4 and two or more undecided agents other than a stand on v.  Else claim v and decide
    a with m; a single undecided occupant b of v runs PLAN(b, a), and when that returns
    False (b stays on v, which stays claimed) a goes on with its next candidate; otherwise
    return True.  A list exhausted: a stays (4), claims its own cell, returns False.

    pos [E, N, 2] the agents' (row, col); the other arguments as `partial_policy_actions`.
    Returns int8 [E, N]; with stats=True also an int64 [len(PIBT_STATS)] of branch counts.
    """
    avail = np.asarray(avail, dtype=np.int64)
    pd = np.asarray(pd, dtype=np.int64)
    d = np.asarray(d, dtype=np.int64)
    pos = np.asarray(pos, dtype=np.int64)
    E, N = pd.shape
    env = np.asarray(env_ids, dtype=np.int64).astype(np.uint64)[:, None]
    ag = np.arange(N, dtype=np.uint64)[None, :]
    tt = int(t) & 0xFFFFFFFF
    u = splitmix64(np.uint64(seed) ^ _mul(env, K_ENV) ^ _mul(np.uint64(tt), K_T) ^ _mul(ag, K_AGENT))
    explore = (u >> np.uint64(32)) < np.uint64(eps_q)
    draw = (u % np.uint64(5)).astype(np.int64)
    ok = (((avail[..., None] >> np.arange(4)) & 1) == 1) & (d >= 0)
    acts = np.full((E, N), 4, dtype=np.int8)
    cnt = dict.fromkeys(PIBT_STATS, 0)
    for e in range(E):
        cell = [(int(pos[e, a, 0]), int(pos[e, a, 1])) for a in range(N)]
        decided = [False] * N
        claimed = set()

        def candidates(a, top):
            stay = (4, cell[a])
            if pd[e, a] < 0:
                return [stay]
            if explore[e, a]:
                cnt["explore_top" if top else "explore_pushed"] += 1
            if top and explore[e, a]:
                m = int(draw[e, a])
                return ([(m, (cell[a][0] + PIBT_STEPS[m][0], cell[a][1] + PIBT_STEPS[m][1]))]
                        if m < 4 and ok[e, a, m] else []) + [stay]
            keys = sorted([(int(d[e, a, m]), m) for m in range(4) if ok[e, a, m]] + [(int(pd[e, a]), 4)])
            return [(m, cell[a] if m == 4 else (cell[a][0] + PIBT_STEPS[m][0], cell[a][1] + PIBT_STEPS[m][1]))
                    for _, m in keys]

        def plan(a, parent, depth):
            if depth >= 3:
                cnt["depth3"] += 1
            for m, v in candidates(a, parent is None):
                if v in claimed:
                    cnt["skip_claimed"] += 1
                    continue
                if parent is not None and v == cell[parent]:
                    cnt["skip_parent"] += 1
                    continue
                occ = [b for b in range(N) if b != a and not decided[b] and cell[b] == v] if m != 4 else []
                if len(occ) >= 2:
                    cnt["skip_multi"] += 1
                    continue
                claimed.add(v)
                decided[a] = True
                acts[e, a] = m
                if occ:
                    cnt["push"] += 1
                    if not plan(occ[0], a, depth + 1):
                        cnt["push_failed"] += 1
                        continue
                return True
            cnt["forced_stay"] += 1
            decided[a] = True
            acts[e, a] = 4
            claimed.add(cell[a])
            return False

        for a in sorted(range(N), key=lambda a: (bool(pd[e, a] == 0), (a - tt) % N)):
            if not decided[a]:
                plan(a, None, 1)
    if stats:
        return acts, np.array([cnt[k] for k in PIBT_STATS], dtype=np.int64)
    return acts


def runner_policy_seed(seed, run):
    """The policy seed of run number `run` of ParallelRunner.collect:
    splitmix64(seed ^ run * K_T) -- a pure function of (seed, run), so every run draws its
    own random words (the policy's counter restarts at 0 with every episode) and a run can
    be replayed from its number."""
    return int(splitmix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
                          ^ _mul(np.uint64(int(run) & 0xFFFFFFFFFFFFFFFF), K_T)))


def runner_repair_seed(seed, run):
    """The repair seed of run number `run` of ParallelRunner.run with runner_device_repair:
    splitmix64(seed ^ run * K_T ^ STREAM_REPAIR * K_STREAM) -- `runner_policy_seed`'s
    derivation on the repair's stream, so a run can be replayed from its number."""
    return int(splitmix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
                          ^ _mul(np.uint64(int(run) & 0xFFFFFFFFFFFFFFFF), K_T)
                          ^ _mul(np.uint64(0x800), K_STREAM)))


def select_words(seed, env_ids, t, n_agents):
    """The selection stream's words, uint64 [len(env_ids), n_agents]:
    splitmix64(seed ^ gid*K_ENV ^ (uint32)t*K_T ^ a*K_AGENT ^ STREAM_SELECT*K_STREAM)
    (mapfx_select_word of include/mapfx_runner.h); env_ids are GLOBAL env ids."""
    env = np.asarray(env_ids, dtype=np.int64).astype(np.uint64)[:, None]
    ag = np.arange(n_agents, dtype=np.uint64)[None, :]
    tt = np.uint64(int(t) & 0xFFFFFFFF)
    return splitmix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ _mul(env, K_ENV) ^ _mul(tt, K_T)
                      ^ _mul(ag, K_AGENT) ^ _mul(np.uint64(STREAM_SELECT), K_STREAM))


def greedy_index(v):
    """The greedy index over the last axis, what torch.max(dim)[1] returns on the CPU: the
    first index of the maximum, a NaN greater than every number (the first NaN wins), 0 when
    every entry is -inf."""
    v = np.asarray(v, dtype=np.float32)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        first_max = (np.where(nan, -np.inf, v) == np.where(nan, -np.inf, v).max(-1, keepdims=True)).argmax(-1)
    return np.where(nan.any(-1), nan.argmax(-1), first_max).astype(np.int64)


def select_actions(seed, env_ids, t, q, avail=None, eps_q=0, mode="epsilon_greedy", greedy_only=False):
    """The device action selection (mapfx_select_actions, include/mapfx_runner.h), restated.
    This function is the rule's definition.

    q [rows, N, A] float32, avail [rows, N, A] (nonzero = available; None: all), env_ids
    [rows] GLOBAL env ids, t the step counter, u = select_words(seed, env_ids, t, N).

    "epsilon_greedy" (PyMARL's EpsilonGreedyActionSelector): v_i = m_i ? q_i : -inf,
    g = greedy_index(v).  explore = not greedy_only and (u >> 32) < eps_q (eps_q = round(eps *
    2**32), 2**32 = always).  With n = the number of available actions: explore and n > 0 takes
    the k-th available index in ascending order, k = ((u & 0xFFFFFFFF) * n) >> 32; else g (0
    when nothing is available).

    "multinomial" (MultinomialActionSelector): p_i = m_i ? q_i : 0.  greedy_only: greedy_index(p)
    (the masked zeros take part).  Else the float32 prefix sums c_0 = p_0, c_i = c_{i-1} + p_i
    and s = c_{A-1}; s not a finite number above 0: greedy_index(p); else r = float((u &
    0xFFFFFFFF) >> 8) * 2**-24 (exact), x = r * s (one float32 rounding), and the action is the
    first i with c_i > x, or, if there is none, the last i with p_i > 0.

    Returns int64 [rows, N]."""
    q = np.asarray(q, dtype=np.float32)
    rows, N, A = q.shape
    m = np.ones(q.shape, dtype=bool) if avail is None else np.asarray(avail) != 0
    u = select_words(seed, env_ids, t, N)
    lo = u & np.uint64(0xFFFFFFFF)
    if SELECT_MODES[mode] == 0:
        g = greedy_index(np.where(m, q, np.float32(-np.inf)))
        explore = ((u >> np.uint64(32)) < np.uint64(eps_q)) & (not greedy_only)
        n = m.sum(-1)
        k = ((lo * n.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        kth = (m & (np.cumsum(m, -1) - 1 == k[..., None])).argmax(-1)
        return np.where(explore & (n > 0), kth, g).astype(np.int64)
    p = np.where(m, q, np.float32(0.0)).astype(np.float32)
    g = greedy_index(p)
    if greedy_only:
        return g
    c = np.empty_like(p)
    with np.errstate(invalid="ignore", over="ignore"):
        c[..., 0] = p[..., 0]
        for i in range(1, A):
            c[..., i] = c[..., i - 1] + p[..., i]                    # float32, in this order
        s = c[..., -1]
        ok = np.isfinite(s) & (s > 0)
        r = (lo >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
        x = (r * s).astype(np.float32)
        above = c > x[..., None]
        last_pos = A - 1 - (p > 0)[..., ::-1].argmax(-1)
    drawn = np.where(above.any(-1), above.argmax(-1), last_pos)
    return np.where(ok, drawn, g).astype(np.int64)


def cell_keys(seed, env_ids, n_cells, stream):
    """Per-(env, cell) uint64 keys of stream `stream` (obstacles, starts, goals)."""
    env = np.asarray(env_ids, dtype=np.int64).astype(np.uint64)[:, None]
    cell = np.arange(n_cells, dtype=np.uint64)[None, :]
    k = (np.uint64(seed) ^ _mul(env, K_ENV) ^ _mul(cell, K_CELL)
         ^ _mul(np.uint64(stream), K_STREAM))
    return splitmix64(k)


def scen_draw(seed, env_ids, episodes, n_lines, n_agents):
    """The device scenario draw of mapfx_partial_draw (include/mapfx_partial.h), restated.

    key(stream, idx) = splitmix64(seed ^ gid*K_ENV ^ ep*K_T ^ idx*K_CELL ^ stream*K_STREAM)
    per env (global id gid, episode counter ep):
      f = ((key(STREAM_SCEN_FILE, 0) >> 32) * F) >> 32            a uniform file
      s_j = (key(STREAM_SCEN_LINE, j) & ~0xFFFF) | j,  j < L = n_lines[f]
      agent a gets line sorted(s)[a] & 0xFFFF                     a uniform ordered sample
    (the distribution of random.randint + random.sample, marl_partial.py:902-929).
    `episodes` is one counter or one per env.  Returns (file int32 [E], line int32
    [E, n_agents]); an env whose file has no more than n_agents lines (the reference
    asserts) has a row of -1 (its `file` entry still names the file drawn).
    """
    n_lines = np.asarray(n_lines, dtype=np.int64)
    F, N = int(n_lines.shape[0]), int(n_agents)
    gid = np.asarray(env_ids, dtype=np.int64).astype(np.uint64)
    ep = np.broadcast_to(np.asarray(episodes, dtype=np.int64) & 0xFFFFFFFF, gid.shape).astype(np.uint64)
    base = np.uint64(seed) ^ _mul(gid, K_ENV) ^ _mul(ep, K_T)
    kf = splitmix64(base ^ _mul(np.uint64(STREAM_SCEN_FILE), K_STREAM))
    file = (((kf >> np.uint64(32)) * np.uint64(F)) >> np.uint64(32)).astype(np.int32)
    line = np.full((gid.shape[0], N), -1, dtype=np.int32)
    sl = _mul(np.uint64(STREAM_SCEN_LINE), K_STREAM)
    for e in range(gid.shape[0]):
        L = int(n_lines[file[e]])
        if L <= N:
            continue
        j = np.arange(L, dtype=np.uint64)
        s = (splitmix64(base[e] ^ _mul(j, K_CELL) ^ sl) & ~np.uint64(0xFFFF)) | j
        line[e] = (np.sort(s)[:N] & np.uint64(0xFFFF)).astype(np.int32)
    return file, line


# Stream of output mode's collision repair (mapfx_partial_repair, csrc/repair.hip): site s of
# the table below draws from stream STREAM_REPAIR + s
STREAM_REPAIR = 0x800
REPAIR_MAX_ROUNDS = 16
# mapfx_partial_repair's flags byte (include/mapfx_partial.h MAPFX_REPAIR_*)
REPAIR_NODE_RAN, REPAIR_EDGE_RAN, REPAIR_NODE_CAP, REPAIR_EDGE_CAP = 1, 2, 4, 8
REPAIR_SWAP_LEFT = 16   # the edge check of the final positions reads above 0
# what partial_repair(counters=True) counts, in this order: a colliding agent sent back to its
# old cell, moved by one of `these_acts`, moved by one of `acts_try`; a swapping agent that
# side-stepped, that backed up, a pair put back on its old cells
REPAIR_COUNTERS = ("node_back", "node_these", "node_try", "edge_side", "edge_back", "edge_put")
_REPAIR_DELTA = ((-1, 0), (1, 0), (0, -1), (0, 1))           # marl_partial.py:617-643, acts 0..3
_REPAIR_SIDE = ((2, 3), (3, 2), (0, 1), (1, 0))              # :775 try_map
_REPAIR_BACK = (1, 0, 3, 2)                                  # :776


def repair_word(seed, gid, t, site, r, owner, j):
    """splitmix64(seed ^ gid*K_ENV ^ (uint32)t*K_T ^ owner*K_AGENT ^ (r*4096 + j)*K_CELL ^
    (STREAM_REPAIR + site)*K_STREAM): the word of item j of `site` in round r (per phase, from
    0) of the repair of global env `gid` at step count t."""
    m = 0xFFFFFFFFFFFFFFFF                       # (plain Python integers: one word at a time)
    x = (int(seed) ^ int(gid) * int(K_ENV) ^ (int(t) & 0xFFFFFFFF) * int(K_T) ^ int(owner) * int(K_AGENT)
         ^ (int(r) * 4096 + int(j)) * int(K_CELL) ^ (STREAM_REPAIR + int(site)) * int(K_STREAM)) & m
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def repair_order(seed, gid, t):
    """The counter-based `order(site, r, owner, items)` of partial_repair for one env-step: the
    items in canonical ascending order, item j keyed (repair_word(.., site, r, owner, j) &
    ~0xFFFF) | j, returned in ascending key order.  Site 4 (the two members (i, j) of a pair):
    (j, i) iff bit 63 of repair_word(.., 4, r, i, j) is set."""
    def order(site, r, owner, items):
        items = sorted(items)
        if site == 4:
            i, j = items
            return [j, i] if repair_word(seed, gid, t, 4, r, i, j) >> 63 else [i, j]
        keys = [(repair_word(seed, gid, t, site, r, owner, j) & ~0xFFFF) | j for j in range(len(items))]
        return [items[k & 0xFFFF] for k in sorted(keys)]
    return order


def _repair_check_node(pos):
    """marl_partial.py:713-737 -> (count, 0/1 vector)."""
    n = {}
    for p in pos:
        n[p] = n.get(p, 0) + 1
    vec = [1 if n[p] > 1 else 0 for p in pos]
    return sum(vec), vec


def _repair_check_edge(old, new):
    """marl_partial.py:822-857 -> (count, vector, set of sorted pairs)."""
    vec, pairs = [0] * len(new), set()
    for i, (io, inew) in enumerate(zip(old, new)):
        if io == inew:
            continue
        for j, jo in enumerate(old):
            if j != i and jo == inew and new[j] == io:
                vec[i] += 1
                pairs.add(tuple(sorted([i, j])))
    return sum(vec), vec, pairs


def partial_repair_env(old, new, acts, grid, t, gid, seed=0, max_rounds=REPAIR_MAX_ROUNDS, order=None,
                       counters=None):
    """Output mode's collision repair of ONE env-step (MARL-curve-main/src/envs/marl_partial.py
    :262-275 with the solvers :645-711 and :739-820), the definition of mapfx_partial_repair
    (include/mapfx_partial.h).  The reference's control flow, quirks included; its two `while`
    loops are cut at `max_rounds` rounds each and every random.shuffle is `order(site, r,
    owner, items)` -- by default `repair_order(seed, gid, t)`.

    old / new: the N cells (row, col) before the step and the raw ones after it; acts: the
    step's actions (0..4); grid [H, W], nonzero = obstacle; t: the env's step count after the
    step.  A cell is free iff it is on the grid and is no obstacle or held an agent before the
    step (grid + counts(old) != -1, :504-522).

    Returns (pos, node_vec, edge_vec, flags, (node rounds, edge rounds)): the vectors are those
    of the last check of each kind (the raw one where the phase did not run); flags bit 4
    (REPAIR_SWAP_LEFT) says that the edge check of the final positions reads above 0.  `counters`, a
    dict, gets REPAIR_COUNTERS added up."""
    if not 1 <= int(max_rounds) <= REPAIR_MAX_ROUNDS:
        raise ValueError("max_rounds must be in 1..%d" % REPAIR_MAX_ROUNDS)
    grid = np.asarray(grid)
    H, W = grid.shape
    old = [(int(p[0]), int(p[1])) for p in old]
    new = [(int(p[0]), int(p[1])) for p in new]
    acts = [int(a) for a in acts]
    n = len(new)
    if order is None:
        order = repair_order(seed, gid, t)
    cnt_br = counters if counters is not None else {}
    held = set(old)

    def bump(k):
        cnt_br[k] = cnt_br.get(k, 0) + 1

    def free(p):
        return 0 <= p[0] < H and 0 <= p[1] < W and (grid[p] == 0 or p in held)

    def move(p, a):
        return (p[0] + _REPAIR_DELTA[a][0], p[1] + _REPAIR_DELTA[a][1])

    def counts():
        c = {}
        for p in new:
            c[p] = c.get(p, 0) + 1
        return c

    def solve_node(r, node_vec):                                                   # :645-711
        col = order(0, r, 0, [i for i in range(n) if node_vec[i] > 0])
        cnt = counts()
        for a in col:
            a_pos = new[a]
            if cnt.get(a_pos, 0) <= 1:
                continue
            o = old[a]
            if cnt.get(o, 0) <= 0:
                cnt[a_pos] = cnt.get(a_pos, 0) - 1
                new[a] = o
                cnt[o] = cnt.get(o, 0) + 1
                bump("node_back")
                continue
            these = order(1, r, a, [i for i in range(n) if new[i] == o])
            solved = False
            for act in [acts[i] for i in these]:
                if act == acts[a]:
                    continue
                if act == 4:                       # __agent_step: a stay is the old cell itself
                    p = o
                else:
                    p = move(o, act)
                    if not free(p):
                        continue
                if cnt.get(p, 0) <= 0:
                    cnt[a_pos] = cnt.get(a_pos, 0) - 1
                    new[a] = p
                    cnt[p] = cnt.get(p, 0) + 1
                    bump("node_these")
                    solved = True
                    break
            if solved:
                continue
            for act in order(2, r, a, [0, 1, 2, 3]):
                p = move(o, act)
                if act == acts[a] or not free(p):
                    continue
                if cnt.get(p, 0) <= 0:
                    cnt[o] = cnt.get(o, 0) - 1     # the OLD cell, not a_pos (:706)
                    new[a] = p
                    cnt[p] = cnt.get(p, 0) + 1
                    bump("node_try")
                    break

    def solve_edge(r, pairs):                                                      # :739-820
        cnt = counts()
        for pair in order(3, r, 0, pairs):
            pair = order(4, r, min(pair), [pair[0], pair[1]])
            solved = False
            a_pos = None
            for a in pair:
                a_pos = new[a]
                for act in _REPAIR_SIDE[acts[a]]:
                    p = move(old[a], act)
                    if free(p) and cnt.get(p, 0) <= 0:
                        cnt[a_pos] = cnt.get(a_pos, 0) - 1
                        new[a] = p
                        cnt[p] = cnt.get(p, 0) + 1
                        bump("edge_side")
                        solved = True
                        break
                if solved:
                    break
            if solved:
                continue
            for a in pair:
                p = move(old[a], _REPAIR_BACK[acts[a]])
                if free(p) and cnt.get(p, 0) <= 0:
                    cnt[a_pos] = cnt.get(a_pos, 0) - 1   # a_pos as the loop above left it (:807)
                    new[a] = p
                    cnt[p] = cnt.get(p, 0) + 1
                    bump("edge_back")
                    solved = True
            if solved:
                continue
            bump("edge_put")
            for a in pair:
                new[a] = old[a]

    n_node, node_vec = _repair_check_node(new)                                     # :236
    n_edge, edge_vec, pairs = _repair_check_edge(old, new)                         # :238
    flags, rounds = 0, [0, 0]
    if n_node > 0:                                                                 # :263-268
        flags |= REPAIR_NODE_RAN
        while n_node > 0 and rounds[0] < max_rounds:
            solve_node(rounds[0], node_vec)
            n_node, node_vec = _repair_check_node(new)
            rounds[0] += 1
        if n_node > 0:
            flags |= REPAIR_NODE_CAP
    if n_edge > 0 and not flags & REPAIR_NODE_CAP:                                 # :269-275
        flags |= REPAIR_EDGE_RAN
        while n_edge > 0 and rounds[1] < max_rounds:
            solve_edge(rounds[1], pairs)                 # always the RAW pair set (:246, :272)
            n_edge, edge_vec, _ = _repair_check_edge(old, new)
            rounds[1] += 1
        if n_edge > 0:
            flags |= REPAIR_EDGE_CAP
    # a swap on the final positions (the edge vector returned stays that of the last check the
    # reference makes): with no cap hit, one the node phase created on a step whose raw edge
    # count was 0, for which the reference starts no edge phase
    if flags and _repair_check_edge(old, new)[0] > 0:
        flags |= REPAIR_SWAP_LEFT
    return new, node_vec, edge_vec, flags, tuple(rounds)


def partial_repair(old, new, acts, grid, t, seed=0, env_offset=0, max_rounds=REPAIR_MAX_ROUNDS, order=None,
                   counters=False):
    """`partial_repair_env` over a batch: what mapfx_partial_repair computes, bit for bit.

    old / new [E, N, 2], acts [E, N], grid [H, W] or [E | 1, H, W] (nonzero = obstacle), t one
    step count or one per env; env e is global env env_offset + e.  An env with an action
    outside 0..4 (its step was skipped) is not repaired: pos = new, flags 0, zero vectors and
    skipped[e] set (the device writes nothing of it but the flags byte).  `order`, when given,
    replaces the counter-based order of every env (see partial_repair_env).

    Returns a dict: pos int32 [E, N, 2], node uint8 [E, N], edge int32 [E, N], flags uint8 [E],
    rounds int32 [E, 2], skipped bool [E]; with counters=True also counters, int64
    [len(REPAIR_COUNTERS)]."""
    old = np.asarray(old, dtype=np.int64)
    new = np.asarray(new, dtype=np.int64)
    acts = np.asarray(acts, dtype=np.int64)
    E, N = acts.shape
    grid = np.asarray(grid)
    if grid.ndim == 2:
        grid = grid[None]
    tt = np.broadcast_to(np.asarray(t, dtype=np.int64), (E,))
    res = dict(pos=new.astype(np.int32), node=np.zeros((E, N), np.uint8), edge=np.zeros((E, N), np.int32),
               flags=np.zeros((E,), np.uint8), rounds=np.zeros((E, 2), np.int32), skipped=np.zeros((E,), bool))
    cnt = {}
    for e in range(E):
        if ((acts[e] < 0) | (acts[e] > 4)).any():
            res["skipped"][e] = True
            continue
        pos, nv, ev, fl, rd = partial_repair_env(old[e], new[e], acts[e], grid[e if grid.shape[0] > 1 else 0],
                                                 int(tt[e]), env_offset + e, seed, max_rounds, order, cnt)
        res["pos"][e], res["node"][e], res["edge"][e], res["flags"][e], res["rounds"][e] = pos, nv, ev, fl, rd
    if counters:
        res["counters"] = np.array([cnt.get(k, 0) for k in REPAIR_COUNTERS], dtype=np.int64)
    return res
