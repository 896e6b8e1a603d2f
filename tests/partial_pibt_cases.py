"""Cases and expected episodes of the collision-free on-device policy (MAPFX_POLICY_PIBT of
include/mapfx_partial.h; mapfx.rng.partial_policy_pibt_actions is its definition) -- TEST
INFRASTRUCTURE ONLY; no test lives here.  tests/test_partial_pibt_ref.py proves on the CPU
what tests/test_gpu_partial_pibt.py and tests/test_gpu_runner_pibt.py rely on.

The sparse cases are tests/partial_step_cases.py's own (four of them); the dense ones, where
the push chains and the backtracking live, are built here in the same dict form (`build` of
partial_step_cases: grids, starts, goals, goal_dist, actions), so that its make_refs,
snapshot and compare serve both.
"""
from __future__ import annotations

import functools

import numpy as np

import runner_collect_cases as rcc
import runner_ref
from oracle.partial_oracle import bfs_goal_dist
from partial_rollout_cases import policy_inputs
from partial_step_cases import BY_NAME, KW, Case, build, make_refs, snapshot
from test_gpu_runner_shapes import CASES as RUNNER_CASES, FILL, RUNS

SPARSE = ("fast-w5-l16-u8t", "fast-w5-l8-i16", "fast-w5-l32-u8", "gen-w5-n3")
# name: (H, W, obstacles, N, E, T, limit, stacked env or None).  E: a last wave with fewer envs
# than the wave holds (64 / lane group: 4, 2, 1, 8); limit past T except where the autoreset
# test wants restarts
DENSE = {
    "dense-6x6-n15": (6, 6, ((1, 1), (3, 4), (4, 2)), 15, 6, 16, 40, 5),     # L 16; env 5 stacked
    "dense-5x5-n20": (5, 5, (), 20, 3, 12, 40, None),                        # L 32
    "dense-9x9-n64": (9, 9, ((4, 4), (2, 6)), 64, 3, 10, 40, None),          # L 64: the deepest chains
    "dense-3x7-n5": (3, 7, ((1, 3),), 5, 11, 24, 40, None),                  # L 8
}
CASES = SPARSE + tuple(DENSE)
EPS = (0, 2 ** 30, 2 ** 32)
PHASES = ("fresh", "mid")
SEED = 0x91B7C0FFEE


def case_of(name):
    if name in BY_NAME:
        return BY_NAME[name]
    H, W, _, N, E, T, _, _ = DENSE[name]
    return Case(name, H, W, "dense", N, 5, 5, E, T, False, "int8")


def limit_of(name):
    return DENSE[name][6] if name in DENSE else case_of(name).T - 2


def params(name, limit=None):
    c = case_of(name)
    return dict(KW, obs_window=c.win, obs_knn_agents=c.K, episode_limit=limit_of(name) if limit is None else limit)


@functools.lru_cache(maxsize=None)
def build_case(name):
    """`build` of partial_step_cases for a sparse case; for a dense one random distinct starts
    and distinct goals on its map (one map for all envs, passed per env), random given
    actions for the "mid" phase, and in the stacked env agent 1 starting on agent 0's cell."""
    if name in BY_NAME:
        return build(BY_NAME[name])
    H, W, obst, N, E, T, _, stacked = DENSE[name]
    rng = np.random.default_rng([H, W, N, E, 11])
    g = np.zeros((H, W), np.int8)
    for r, c in obst:
        g[r, c] = -1
    free = np.argwhere(g == 0)
    assert (bfs_goal_dist(g, free[0]) >= 0).sum() == len(free), "the free cells must be one component"
    starts = np.stack([free[rng.permutation(len(free))[:N]] for _ in range(E)]).astype(np.int32)
    goals = np.stack([free[rng.permutation(len(free))[:N]] for _ in range(E)]).astype(np.int32)
    if stacked is not None:
        starts[stacked, 1] = starts[stacked, 0]
    tables = {}
    for q in {tuple(int(v) for v in q) for q in goals.reshape(-1, 2)}:
        tables[q] = bfs_goal_dist(g, q)
    goal_dist = np.stack([np.stack([tables[tuple(int(v) for v in goals[e, a])] for a in range(N)])
                          for e in range(E)])
    b = {"grids": np.stack([g] * E), "starts": starts, "goals": goals, "goal_dist": goal_dist,
         "actions": rng.integers(0, 5, size=(T, E, N))}
    for v in b.values():
        v.setflags(write=False)
    return b


def refs_of(name, limit=None):
    return make_refs(case_of(name), build_case(name), limit_of(name) if limit is None else limit)


def stacked_envs(name):
    """The envs in which two agents start on one cell."""
    b = build_case(name)
    return [e for e in range(len(b["starts"])) if len({tuple(p) for p in b["starts"][e].tolist()}) < b["starts"].shape[1]]


def rule_actions(rule, seed, ids, t, eps_q, refs, stats=None):
    """The actions of one step of `refs` as they stand, by rule "pibt" or "descent"."""
    from mapfx import rng
    avail, pd, d = policy_inputs(refs)
    if rule == "descent":
        return rng.partial_policy_actions(seed, ids, t, eps_q, avail, pd, d)
    pos = np.array([r.pos for r in refs], np.int64).reshape(len(refs), -1, 2)
    a, st = rng.partial_policy_pibt_actions(seed, ids, t, eps_q, avail, pd, d, pos, stats=True)
    if stats is not None:
        stats += st
    return a


def episode(refs, T, eps_q, seed, t0=0, env_ids=None, autoreset=False, rules="pibt"):
    """The restatement stepped T times under the rule (`rules`: one name, or one per step).
    Returns (actions int8 [T, E, N], snapshots after each step, the rule's branch counts,
    completed [E]: every agent of the env stood on its goal after some step)."""
    from mapfx import rng
    ids = np.arange(len(refs)) if env_ids is None else np.asarray(env_ids)
    acts, snaps = [], []
    stats = np.zeros(len(rng.PIBT_STATS), np.int64)
    completed = np.zeros(len(refs), bool)
    for k in range(T):
        if autoreset:
            for r in refs:
                if r.terminated:
                    r.reset()
        a = rule_actions(rules if isinstance(rules, str) else rules[k], seed, ids, t0 + k, eps_q, refs, stats)
        for e, r in enumerate(refs):
            r.step(a[e])
            completed[e] |= all(r.at_goal)
        acts.append(a)
        snaps.append(snapshot(refs))
    return np.stack(acts), snaps, stats, completed


@functools.lru_cache(maxsize=None)
def run(name, eps_q, phase, rule="pibt"):
    """The expected episode of a GPU test: phase "mid" steps the case's own given actions
    twice first, then T = c.T - pre policy steps at t0 = pre."""
    c, b = case_of(name), build_case(name)
    refs = refs_of(name)
    pre = 2 if phase == "mid" else 0
    for t in range(pre):
        for e, r in enumerate(refs):
            r.step(b["actions"][t, e])
    acts, snaps, stats, completed = episode(refs, c.T - pre, eps_q, SEED, t0=pre, rules=rule)
    return dict(pre=pre, T=c.T - pre, actions=acts, snaps=snaps, stats=stats, completed=completed)


def expected_kernel(name, obs):
    """The instance a pibt rollout launches: partial_rollout_cases.expected_rollout_kernel's
    arguments on partial_pibt_rollout_kernel."""
    from partial_rollout_cases import expected_rollout_kernel
    k = expected_rollout_kernel(case_of(name), obs)
    return ("partial_pibt_rollout_kernel", k[1])


def kernel_args(printed, kernel="partial_pibt_rollout_kernel"):
    import re
    m = re.search(r"(%s)<([^>]*)>" % kernel, printed)
    return (m.group(1), m.group(2).replace(" ", "")) if m else None


# ------------------------------------------------------------------ the runner (collect)
RUNNER_CASES_PIBT = ("fast8_n5", "fast16_n16", "fast16_w7", "gen_n3")
RUNNER_EPS = (0, 2 ** 31)
_RREF = {}


def runner_mac(envs, seed, eps_q, rule="pibt"):
    """The checker's MAC: the rule's actions of envs[b] for b in bs, as they stand before the
    step (terminated envs on the stale list included), with counter t and global env id b."""
    def mac(batch, t, bs):
        return rule_actions(rule, seed, np.asarray(bs), t, eps_q, [envs[b] for b in bs])
    return mac


def runner_reference(name, eps_q, seed=1):
    """runner_collect_cases.policy_reference with the pibt rule as the MAC: RUNS runs on the
    policy maps of the case (pens, a corridor, a field)."""
    from mapfx import rng
    key = (name, eps_q, seed)
    if key in _RREF:
        return _RREF[key]
    case = RUNNER_CASES[name]
    N, W, K, limit, B = case["N"], case["win"], case["K"], case["limit"], case["B"]
    grid_rows = rcc.policy_grid(case)
    ref = runner_ref.RefRunner(runner_log_interval=1)
    runs = []
    for r in range(RUNS):
        starts, goals = rcc.policy_instances(case, r)
        envs = rcc.make_envs(case, grid_rows, starts, goals)
        pseed = rng.runner_policy_seed(seed, r)
        table = np.full((limit + 1, B, N), 4, np.int64)

        def mac(batch, t, bs, inner=runner_mac(envs, pseed, eps_q), table=table):
            a = inner(batch, t, bs)
            table[t, bs] = a
            return a

        batch = runner_ref.new_batch(B, limit + 1, N, 2 * W * W + 13 * K, fill=FILL)
        batch, calls, returns, lengths = ref.run(envs, batch, mac)
        runs.append(dict(starts=starts, goals=goals, pseed=pseed, batch=batch, calls=calls, table=table,
                         returns=np.array(returns, np.float64), lengths=np.array(lengths, np.int64),
                         t_env=ref.t_env))
    _RREF[key] = dict(runs=runs, log=list(ref.log), seed=seed, grid=grid_rows)
    return _RREF[key]
