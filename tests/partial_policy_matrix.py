"""The policy-mode matrix of MARL_PARTIAL: one case per kernel instance that runs an on-device
policy -- partial_rollout_kernel and partial_pibt_rollout_kernel (MarlPartialBatch.rollout),
partial_runner_rollout_kernel and partial_pibt_runner_rollout_kernel (ParallelRunner.collect)
-- each on a crowded pocket map, where the priority-inheritance rule backtracks.  TEST
INFRASTRUCTURE ONLY; no test lives here.  tests/test_partial_policy_matrix.py proves on the CPU
what tests/test_gpu_partial_policy_matrix.py and tests/test_gpu_runner_policy_matrix.py rely on.

A pocket map is obstacle everywhere but a small rectangle (minus a few cells) that the agents
fill: H x W decides the table width (u8 up to 255 cells, int16 up to 32767) and the LDS
geometry, the pocket decides the crowding.  Every pocket touches the bottom or the right
border of its map (an off-grid neighbour: the descent's "unavailable neighbour that would have
been best") and none touches the origin; a per-env case moves it one or two cells along the
border it touches in envs 1 and 2 (mod 3).

The rollout cases have the dict form of partial_step_cases.build (grids, starts, goals,
goal_dist, actions), so its make_refs, snapshot and compare, partial_rollout_cases'
compare_slot and policy_episode and partial_pibt_cases' episode serve unchanged.  The collect
cases keep runner_collect_cases' termination scheme (pens, a closed corridor with one walker)
and put the envs that played in its open field into a pocket below the corridor.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import partial_pibt_cases as pc
import runner_collect_cases as rcc
import runner_ref
from oracle.partial_oracle import bfs_goal_dist
from partial_rollout_cases import expected_rollout_kernel, policy_counts, policy_episode, policy_inputs
from partial_step_cases import FAST_PAIRS, KW, Case, expected_geometry, lane_group, make_refs, table_bytes
from test_gpu_runner_shapes import FILL, REWARDS, RUNS

RULES = ("descent", "pibt")
WINDOWS = (0, 1, 3, 5, 7, 9)
ROLLOUT_KERNEL = {"descent": "partial_rollout_kernel", "pibt": "partial_pibt_rollout_kernel"}
COLLECT_KERNEL = {"descent": "partial_runner_rollout_kernel", "pibt": "partial_pibt_runner_rollout_kernel"}
DESCENT_COUNTS = ("ties", "passed", "explore", "stays")       # partial_rollout_cases.policy_counts
EPS = 2 ** 30           # of every case's own episode; EXTRA_* below add eps 0 and 2^32
SEED = 0x7E57AB1E5
LIMIT = 40              # episode_limit of the rollout cases: past every T


# ------------------------------------------------------------------ the domain
def rollout_domain(rule):
    """What pick_roll<RULE> (csrc/partial.hip) returns in policy mode, where int32 tables are
    refused before it is called: with the rows the five fast pairs at u8 (GDE 1) and int16
    (GDE 2) tables and the six generic windows; without them one per fast lane group and
    table width, and the one generic."""
    k = ROLLOUT_KERNEL[rule]
    return ({(k, "%d,5,%d,%d,true" % (w, L, g)) for w, L in FAST_PAIRS for g in (1, 2)}
            | {(k, "%d,0,0,0,true" % w) for w in WINDOWS}
            | {(k, "0,5,%d,%d,false" % (L, g)) for L in (8, 16, 32) for g in (1, 2)}
            | {(k, "0,0,0,0,false")})


def collect_domain(rule):
    """What pick_run_roll<RULE> returns in policy mode.  mapfx_partial_runner_rollout_offered
    refuses the policy on int32 tables (for either rule) before the pick, so the generic
    window instances are reached through the generic shapes alone; without the rows the table
    width is a run-time value: one instance per fast lane group, and the one generic."""
    k = COLLECT_KERNEL[rule]
    return ({(k, "%d,5,%d,%d,true" % (w, L, g)) for w, L in FAST_PAIRS for g in (1, 2)}
            | {(k, "%d,0,0,0,true" % w) for w in WINDOWS}
            | {(k, "0,5,%d,0,false" % L) for L in (8, 16, 32)}
            | {(k, "0,0,0,0,false")})


def _gde(H, W):
    return {1: 1, 2: 2}[table_bytes(H, W)]      # (KeyError on int32 tables: not offered)


def expected_collect_kernel(c, obs, rule):
    """pick_run_roll<RULE>(win, K, L, table width, obs) for anything with H, W, N, win, K."""
    k, L = COLLECT_KERNEL[rule], lane_group(c.N)
    if not obs:
        return (k, "0,5,%d,0,false" % L if L in (8, 16, 32) else "0,0,0,0,false")
    if c.K == 5 and (c.win, L) in FAST_PAIRS:
        return (k, "%d,5,%d,%d,true" % (c.win, L, _gde(c.H, c.W)))
    return (k, "%d,0,0,0,true" % c.win)


def expected_kernel(name, obs, rule):
    """The instance rollout(policy=rule) launches for a rollout case."""
    _gde(case_of(name).H, case_of(name).W)
    return (ROLLOUT_KERNEL[rule], expected_rollout_kernel(case_of(name), obs)[1])


# ------------------------------------------------------------------ pocket maps
def pocket_origin(H, W, ph, pw, anchor, variant=0):
    """Top-left cell of a ph x pw pocket: "br" against the bottom-right corner, "b" against the
    bottom border, "r" against the right border; variant v moves it v cells along the border
    (for "br": up the right border)."""
    r0 = H - ph if anchor in ("br", "b") else (H - ph) // 2 + 1
    c0 = W - pw if anchor in ("br", "r") else (W - pw) // 2 + 1
    if anchor == "b":
        c0 -= variant
    else:
        r0 -= variant
    assert r0 >= 0 and c0 >= 0 and (r0, c0) != (0, 0), "the pocket stays off the origin"
    return r0, c0


def pocket_grid(H, W, ph, pw, anchor, holes=(), variant=0):
    g = np.full((H, W), -1, np.int8)
    r0, c0 = pocket_origin(H, W, ph, pw, anchor, variant)
    g[r0:r0 + ph, c0:c0 + pw] = 0
    for dr, dc in holes:
        g[r0 + dr, c0 + dc] = -1
    free = np.argwhere(g == 0)
    assert (bfs_goal_dist(g, free[0]) >= 0).sum() == len(free), "the free cells must be one component"
    g.setflags(write=False)
    return g


# ------------------------------------------------------------------ the rollout cases
# pocket: (rows, columns, anchor, holes); stacked: the env in which the last agent and every
# second one before it, three at the most, start on their predecessor's cell (at t = 0 the
# rule plans them last: the agents before them find two undecided occupants there); phase:
# "fresh" (pdist still INT32_MIN: the distances are looked up) or "mid" (after two given steps,
# t0 = 2).  E per lane group L: 64 / L envs fill a wave and 4 waves a block, fewer
# where one wave's LDS (64 KB) holds fewer envs.
Spec = namedtuple("Spec", "H W pocket N win K E T shared stacked phase note")
VARIANTS = 3
ROLLOUT = {
    # --- the five fast pairs x {u8, int16}; without the rows: L {8, 16, 32} x {u8, int16}
    "f-w5-l16-u8": Spec(12, 20, (4, 5, "br", ()), 16, 5, 5, 5, 10, False, 1, "fresh",
                        "N = L: no idle lane; 4 envs per wave + 1; per-env maps"),
    "f-w5-l16-i16": Spec(64, 60, (3, 4, "r", ()), 9, 5, 5, 5, 10, True, None, "mid",
                         "N = L / 2 + 1; 64 x 60: 4 envs pass 40 KB, the rows are staged by half waves"),
    "f-w5-l8-u8": Spec(9, 25, (3, 4, "br", ()), 8, 5, 5, 9, 10, True, 3, "fresh",
                       "N = L; 8 envs per wave + 1"),
    "f-w5-l8-i16": Spec(20, 21, (2, 4, "b", ()), 5, 5, 5, 9, 10, False, None, "mid", "N = L / 2 + 1"),
    "f-w5-l32-u8": Spec(15, 17, (5, 6, "br", ((2, 2),)), 20, 5, 5, 3, 10, False, 2, "fresh",
                        "255 cells: the widest u8 map; 2 envs per wave + 1"),
    "f-w5-l32-i16": Spec(256, 127, (5, 5, "br", ()), 17, 5, 5, 3, 10, True, None, "mid",
                         "N = L / 2 + 1; 256 x 127: one env takes ~77 KB of LDS, so 1 env per wave "
                         "(not 2), 2 waves per block: 2 blocks"),
    "f-w3-l16-u8": Spec(16, 15, (4, 4, "br", ()), 12, 3, 5, 5, 10, False, None, "mid", ""),
    "f-w3-l16-i16": Spec(16, 16, (4, 5, "b", ((1, 2),)), 13, 3, 5, 6, 10, True, None, "fresh",
                         "256 cells: the smallest int16 map"),
    "f-w7-l16-u8": Spec(17, 15, (4, 5, "br", ()), 14, 7, 5, 5, 10, True, None, "mid", ""),
    "f-w7-l16-i16": Spec(127, 256, (3, 4, "br", ()), 10, 7, 5, 3, 10, True, None, "fresh",
                         "127 x 256: the largest map the policy is offered on; 1 env per wave (not 4), "
                         "no staging (the rows stored straight), 2 blocks"),
    # --- the six generic windows; run-time lane groups 1, 2, 4, 8, 16, 32 (K != 5), 64
    "g-w0-n1": Spec(6, 9, (2, 3, "br", ()), 1, 0, 5, 65, 8, False, None, "mid",
                    "L 1: t % N is always 0; K > N; 64 envs per wave + 1"),
    "g-w3-n2": Spec(17, 16, (2, 2, "b", ()), 2, 3, 5, 33, 8, True, None, "fresh",
                    "L 2, int16 tables; K > N"),
    "g-w3-n4": Spec(8, 11, (2, 3, "r", ()), 4, 3, 5, 17, 10, True, None, "mid",
                    "L 4 = N (window 3 is fast at L 16 only); K > N; 16 envs per wave + 1"),
    "g-w7-n7": Spec(11, 19, (3, 4, "br", ()), 7, 7, 5, 9, 10, False, 5, "fresh",
                    "L 8 (window 7 is fast at L 16 only); the stacked env of the generic instance"),
    "g-w1-n10": Spec(10, 14, (3, 5, "b", ()), 10, 1, 5, 5, 10, False, None, "mid", "L 16"),
    "g-w9-n20-k3": Spec(14, 18, (5, 5, "br", ()), 20, 9, 3, 3, 10, True, None, "fresh", "L 32, K != 5"),
    "g-w5-n50": Spec(18, 17, (8, 8, "br", ((3, 3), (5, 1))), 50, 5, 5, 3, 8, True, 1, "fresh",
                     "L 64, int16 tables: the deepest chains"),
}
# the offered limit (H * W <= 32767): not part of the matrix, no instance is theirs alone
EDGE = {
    "edge-181x181": Spec(181, 181, (3, 4, "br", ()), 9, 5, 5, 2, 4, True, None, "fresh", "32761 cells: offered"),
    "edge-128x256": Spec(128, 256, (3, 4, "br", ()), 9, 5, 5, 2, 4, True, None, "fresh", "32768 cells: int32 tables"),
}
SPECS = dict(ROLLOUT, **EDGE)
STACKED = tuple(n for n, s in ROLLOUT.items() if s.stacked is not None)
# the N = 1 and N = 2 cases cannot push three deep (or at all): exempt by name
NO_CHAIN = {"g-w0-n1": 1, "g-w3-n2": 2}
# one further run per kernel family at eps 0 and one at eps 2^32
EXTRA_ROLLOUT = (("f-w7-l16-u8", 0, "fresh"), ("g-w7-n7", 2 ** 32, "mid"),
                 ("f-w3-l16-i16", 2 ** 32, "fresh"), ("g-w9-n20-k3", 0, "mid"))
ROLLOUT_RUNS = tuple((n, EPS, s.phase) for n, s in ROLLOUT.items()) + EXTRA_ROLLOUT


def case_of(name):
    s = SPECS[name]
    return Case(name, s.H, s.W, "pocket", s.N, s.win, s.K, s.E, s.T, s.shared, "int8")


def params(name, limit=LIMIT):
    s = SPECS[name]
    return dict(KW, obs_window=s.win, obs_knn_agents=s.K, episode_limit=limit)


@functools.lru_cache(maxsize=None)
def build_case(name):
    """The dict form of partial_step_cases.build: random distinct starts and distinct goals
    inside the pocket, random given actions for the "mid" phase, and in the stacked env up to
    three pairs of agents on one cell each."""
    s = SPECS[name]
    ph, pw, anchor, holes = s.pocket
    rng = np.random.default_rng([s.H, s.W, s.N, s.E, s.win, 23])
    nv = 1 if s.shared else min(s.E, VARIANTS)
    grids = [pocket_grid(s.H, s.W, ph, pw, anchor, holes, v) for v in range(nv)]
    var = (lambda e: 0) if s.shared else (lambda e: e % VARIANTS)
    starts = np.zeros((s.E, s.N, 2), np.int32)
    goals = np.zeros((s.E, s.N, 2), np.int32)
    for e in range(s.E):
        free = np.argwhere(grids[var(e)] == 0)
        assert len(free) >= s.N
        starts[e] = free[rng.permutation(len(free))[:s.N]]
        goals[e] = free[rng.permutation(len(free))[:s.N]]
    if s.stacked is not None:
        for a in range(s.N - 1, max(s.N - 6, 0), -2):     # up to three stacked pairs
            starts[s.stacked, a] = starts[s.stacked, a - 1]
    tables = {}
    for e in range(s.E):
        for q in goals[e]:
            key = (var(e), int(q[0]), int(q[1]))
            if key not in tables:
                tables[key] = bfs_goal_dist(grids[var(e)], q)
    goal_dist = np.stack([np.stack([tables[(var(e), int(q[0]), int(q[1]))] for q in goals[e]])
                          for e in range(s.E)])
    b = {"grids": np.stack([grids[var(e)] for e in range(1 if s.shared else s.E)]), "starts": starts,
         "goals": goals, "goal_dist": goal_dist, "actions": rng.integers(0, 5, size=(s.T, s.E, s.N))}
    for v in b.values():
        v.setflags(write=False)
    return b


def refs_of(name, limit=LIMIT):
    return make_refs(case_of(name), build_case(name), limit)


def stacked_envs(name):
    b = build_case(name)
    return [e for e in range(len(b["starts"])) if len({tuple(p) for p in b["starts"][e].tolist()}) < b["starts"].shape[1]]


def rule_episode(rule, refs, T, eps_q, t0=0, env_ids=None, autoreset=False):
    """(actions, snapshots, branch counts by name) of `refs` stepped T times under the rule."""
    from mapfx import rng
    if rule == "pibt":
        acts, snaps, stats, _ = pc.episode(refs, T, eps_q, SEED, t0=t0, env_ids=env_ids, autoreset=autoreset)
        return acts, snaps, dict(zip(rng.PIBT_STATS, stats.tolist()))
    acts, snaps, cnt = policy_episode(refs, T, eps_q, SEED, t0=t0, env_ids=env_ids, autoreset=autoreset)
    return acts, snaps, dict(zip(DESCENT_COUNTS, cnt.tolist()))


@functools.lru_cache(maxsize=None)
def run(name, rule, eps_q, phase):
    """The expected episode of a GPU test: phase "mid" steps the case's own given actions
    twice first, then T = s.T - pre policy steps at t0 = pre."""
    s, b = SPECS[name], build_case(name)
    refs = refs_of(name)
    pre = 2 if phase == "mid" else 0
    for t in range(pre):
        for e, r in enumerate(refs):
            r.step(b["actions"][t, e])
    acts, snaps, counts = rule_episode(rule, refs, s.T - pre, eps_q, t0=pre)
    return dict(pre=pre, T=s.T - pre, actions=acts, snaps=snaps, counts=counts)


def geometry(name):
    """expected_geometry of the case, and how its E envs fall into waves and blocks."""
    s = ROLLOUT[name]
    g = expected_geometry(case_of(name))
    waves = -(-s.E // g["EPW"])
    return dict(g, full=64 // lane_group(s.N), waves=waves, partial_last=s.E % g["EPW"] != 0)


# ------------------------------------------------------------------ the collect cases
# name: N, window, K, B, H x W, the pocket (rows, columns: against the bottom-right corner),
# stacked (up to three pairs of agents of the first pocket env start on one cell each).  limit 5: max_t = 6.
CSpec = namedtuple("CSpec", "N win K B H W pocket stacked")
COLLECT = {
    "cf-w5-l16-u8": CSpec(16, 5, 5, 7, 10, 20, (4, 5), True),
    "cf-w5-l16-i16": CSpec(9, 5, 5, 7, 64, 60, (3, 4), False),
    "cf-w5-l8-u8": CSpec(8, 5, 5, 11, 8, 25, (3, 4), True),
    "cf-w5-l8-i16": CSpec(5, 5, 5, 11, 20, 21, (2, 4), False),
    "cf-w5-l32-u8": CSpec(20, 5, 5, 7, 13, 16, (5, 6), True),
    "cf-w5-l32-i16": CSpec(17, 5, 5, 7, 40, 17, (5, 5), False),
    "cf-w3-l16-u8": CSpec(12, 3, 5, 7, 10, 15, (4, 4), False),
    "cf-w3-l16-i16": CSpec(13, 3, 5, 7, 16, 16, (4, 5), False),
    "cf-w7-l16-u8": CSpec(14, 7, 5, 7, 10, 15, (4, 5), False),
    "cf-w7-l16-i16": CSpec(10, 7, 5, 7, 30, 40, (3, 4), False),
    "cg-w0-n1": CSpec(1, 0, 5, 67, 6, 9, (2, 3), False),
    "cg-w1-n10": CSpec(10, 1, 5, 7, 10, 14, (3, 5), False),
    "cg-w3-n4": CSpec(4, 3, 5, 19, 8, 11, (2, 3), False),
    "cg-w5-n50": CSpec(50, 5, 5, 7, 20, 20, (8, 8), True),
    "cg-w7-n7": CSpec(7, 7, 5, 11, 11, 19, (3, 4), False),
    "cg-w9-n20-k3": CSpec(20, 9, 3, 7, 14, 18, (5, 5), False),
}
COLLECT_LIMIT = 5
COLLECT_NO_CHAIN = {"cg-w0-n1": 1}
COLLECT_STACKED = tuple(n for n, s in COLLECT.items() if s.stacked)
# the cases that also run without the rows: lane groups 8, 16, 32 and the generic
COLLECT_NO_ROWS = ("cf-w5-l8-i16", "cf-w3-l16-u8", "cf-w5-l32-u8", "cg-w5-n50")
EXTRA_COLLECT = (("cf-w5-l8-u8", 0), ("cg-w3-n4", 2 ** 32), ("cg-w7-n7", 0), ("cf-w5-l8-i16", 2 ** 32))
COLLECT_RUNS = tuple((n, EPS) for n in COLLECT) + EXTRA_COLLECT
# args.seed of the runs, searched on the CPU so that both runs of (case, rule, eps_q) meet
# test_partial_policy_matrix.py's termination conditions; others: 1
COLLECT_SEEDS = {(n, "descent", EPS): 6 for n in (
    "cf-w5-l16-u8", "cf-w5-l16-i16", "cf-w5-l32-u8", "cf-w5-l32-i16", "cf-w3-l16-u8", "cf-w3-l16-i16",
    "cf-w7-l16-u8", "cf-w7-l16-i16", "cg-w1-n10", "cg-w5-n50", "cg-w9-n20-k3")}
COLLECT_SEEDS.update({("cf-w5-l8-i16", "descent", EPS): 2, ("cf-w5-l8-i16", "descent", 2 ** 32): 330,
                      ("cf-w5-l8-i16", "pibt", 2 ** 32): 17})


def collect_case(name):
    """The dict form of test_gpu_runner_shapes.CASES (what the runner helpers take)."""
    s = COLLECT[name]
    return dict(grid=collect_grid(name), N=s.N, win=s.win, K=s.K, B=s.B, limit=COLLECT_LIMIT,
                H=s.H, W=s.W)


def collect_shape(name):
    s = COLLECT[name]
    return Case(name, s.H, s.W, "pocket", s.N, s.win, s.K, s.B, COLLECT_LIMIT + 1, True, "int8")


def _pen_rows(s):
    per_row = (s.W + 1) // 2
    return -(-(s.N - 1) // per_row) if s.N > 1 else 0


@functools.lru_cache(maxsize=None)
def collect_grid(name):
    """runner_collect_cases.policy_grid with the pocket in the open field's place: pens, the
    closed corridor of five cells, a row of obstacles, then obstacles but for the pocket."""
    s = COLLECT[name]
    nr = _pen_rows(s)
    ph, pw = s.pocket
    assert 2 * nr + 2 + ph <= s.H and s.W >= 5, name
    rows = [["@"] * s.W for _ in range(s.H)]
    for r in range(0, 2 * nr, 2):
        for c in range(0, s.W, 2):
            rows[r][c] = "."
    for c in range(5):
        rows[2 * nr][c] = "."
    for r in range(s.H - ph, s.H):
        for c in range(s.W - pw, s.W):
            rows[r][c] = "."
    return tuple("".join(r) for r in rows)


def collect_kind(name, b):
    """'never' (env 2), 'pocket', or ('early', d): envs 0, 1, 3, 4 and every third from 7 on
    have one walker d cells from its goal in the corridor, the others resting in pens."""
    if b == 2:
        return "never"
    early = [x for x in range(b + 1) if x in (0, 1, 3, 4) or (x >= 7 and x % 3 == 1)]
    if b not in early:
        return "pocket"
    return ("early", rcc.WALK_D[(len(early) - 1) % len(rcc.WALK_D)])


def collect_instances(name, run):
    """(starts, goals) [B, N, 2] of one run."""
    s = COLLECT[name]
    grid = runner_ref.parse_map(collect_grid(name))
    nr, (ph, pw) = _pen_rows(s), s.pocket
    pens = [(r, c) for r in range(0, 2 * nr, 2) for c in range(0, s.W, 2)]
    pocket = np.argwhere(grid == 0)
    pocket = pocket[pocket[:, 0] >= s.H - ph]
    assert len(pocket) == ph * pw >= s.N
    rng = np.random.RandomState(977 + 1000 * run + s.N)
    starts = np.zeros((s.B, s.N, 2), np.int32)
    goals = np.zeros((s.B, s.N, 2), np.int32)
    first = True
    for b in range(s.B):
        kd = collect_kind(name, b)
        if kd == "pocket":
            starts[b] = pocket[rng.choice(len(pocket), s.N, replace=False)]
            goals[b] = pocket[rng.choice(len(pocket), s.N, replace=False)]
            if s.stacked and first:
                for a in range(s.N - 1, max(s.N - 6, 0), -2):
                    starts[b, a] = starts[b, a - 1]
            first = False
        elif kd == "never":
            for n in range(s.N - 1):
                starts[b, n], goals[b, n] = pens[n % len(pens)], pens[(n + 1) % len(pens)]
            starts[b, s.N - 1], goals[b, s.N - 1] = (2 * nr, 0), pocket[0]
        else:
            walker = b % s.N
            for i, n in enumerate(n for n in range(s.N) if n != walker):
                starts[b, n] = goals[b, n] = pens[i]
            starts[b, walker], goals[b, walker] = (2 * nr, 4 - kd[1]), (2 * nr, 4)
    return starts, goals


def collect_pocket_envs(name):
    return [b for b in range(COLLECT[name].B) if collect_kind(name, b) == "pocket"]


_CREF = {}


def collect_reference(name, rule, eps_q, seed=None):
    """The restated reference loop with the rule as its MAC (partial_pibt_cases.rule_actions of
    the envs as they stand, stale ones included): RUNS runs; per run the instances, the policy
    seed, the final batch, the MAC calls (`macs`: t, bs, actions, which had terminated),
    returns, lengths, t_env; the log; and the rule's branch counts over both runs."""
    from mapfx import rng
    seed = COLLECT_SEEDS.get((name, rule, eps_q), 1) if seed is None else seed
    key = (name, rule, eps_q, seed)
    if key in _CREF:
        return _CREF[key]
    s, case = COLLECT[name], collect_case(name)
    grid = runner_ref.parse_map(case["grid"])
    ref = runner_ref.RefRunner(runner_log_interval=1)
    stats = np.zeros(len(rng.PIBT_STATS), np.int64)
    dcounts = np.zeros(len(DESCENT_COUNTS), np.int64)
    runs = []
    for r in range(RUNS):
        starts, goals = collect_instances(name, r)
        envs = runner_ref.make_envs(grid, starts, goals, obs_window=s.win, obs_knn_agents=s.K,
                                    episode_limit=COLLECT_LIMIT, **REWARDS)
        pseed = rng.runner_policy_seed(seed, r)
        macs = []

        def mac(batch, t, bs, envs=envs, pseed=pseed, macs=macs):
            now = [envs[b] for b in bs]
            if rule == "descent":
                dcounts[:] += policy_counts(pseed, np.asarray(bs), t, eps_q, *policy_inputs(now))
            a = pc.rule_actions(rule, pseed, np.asarray(bs), t, eps_q, now, stats)
            macs.append((t, list(bs), a, [bool(e.terminated) for e in now]))
            return a

        batch = runner_ref.new_batch(s.B, COLLECT_LIMIT + 1, s.N, 2 * s.win * s.win + 13 * s.K, fill=FILL)
        batch, calls, returns, lengths = ref.run(envs, batch, mac)
        runs.append(dict(starts=starts, goals=goals, pseed=pseed, batch=batch, calls=calls, macs=macs,
                         returns=np.array(returns, np.float64), lengths=np.array(lengths, np.int64),
                         t_env=ref.t_env))
    _CREF[key] = dict(runs=runs, log=list(ref.log), seed=seed, grid=list(case["grid"]),
                      counts=dict(zip(rng.PIBT_STATS, stats.tolist())) if rule == "pibt"
                      else dict(zip(DESCENT_COUNTS, dcounts.tolist())))
    return _CREF[key]


def collect_unmet(name, rule, ref):
    """Descent: runner_collect_cases.unmet (>= 3 distinct early ends, an env at the limit, a wave
    group with two termination steps, a stale actions row, in every run).  pibt:
    test_runner_reference_episodes_end_at_several_steps' condition (>= 2 distinct ends below
    the limit, an env at the limit) and the stale row."""
    if rule == "descent":
        return rcc.unmet(collect_case(name), ref)
    out = []
    for r, run in enumerate(ref["runs"]):
        lengths = run["lengths"]
        if len(set(lengths[lengths < COLLECT_LIMIT].tolist())) < 2:
            out.append((r, "fewer than 2 distinct early terminations", lengths.tolist()))
        if not (lengths == COLLECT_LIMIT).any():
            out.append((r, "no env runs to the limit"))
        if not any(any(done) for _, _, _, done in run["macs"]):
            out.append((r, "no stale actions row"))
    return out
