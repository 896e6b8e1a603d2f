"""Cases of ParallelRunner.collect / mapfx_runner_rollout (the runner's episode loop as one
launch), expected from tests/runner_ref.py alone -- TEST INFRASTRUCTURE ONLY; no test lives
here.  tests/test_runner_collect_ref.py proves on the CPU what tests/test_gpu_runner_collect.py
relies on.

Shapes (N, window, K, B, H x W, limit 5) are those of tests/test_gpu_runner_shapes.py's matrix.
Policy mode needs terminations that happen whatever the random words are, so its maps are
built here (same H x W):

  rows 0 .. 2 nr - 1   "pens": the cells (even row, even column) free, everything else an
                        obstacle -- an agent in a pen cannot move, whatever its action
  row  2 nr             a closed corridor of five free cells (columns 0..4), the rest obstacle
  row  2 nr + 1         obstacles
  rows below            an open field with a few obstacles

An "early" env has N - 1 agents resting on their goals in pens and one walker in the corridor
whose goal is the corridor's last cell, d cells away: pure descent ends the env after exactly d
steps, a uniform walker whenever it happens to stand there.  Env 2 can never end (every goal in
another pen: unreachable); every third env from env 8 on plays random starts / goals in the
field.
"""
from __future__ import annotations

import numpy as np

import runner_ref
from partial_rollout_cases import policy_inputs
from test_gpu_runner_shapes import CASES, FILL, REWARDS, RUNS, _instances

POLICY_CASES = ("fast8_n5", "fast8_n6", "fast8_n7", "fast8_n8", "fast16_n16", "fast16_w3", "fast16_w7",
                "fast32_n17", "half64_n16", "gen_n3", "gen_w9_k3", "gen_w0")
EPS_QS = (0, 2 ** 31, 2 ** 32)
GIVEN_CASES = ("fast8_n5", "block200_n9")
# args.seed of the policy runs: searched so that, per case and eps_q, both runs meet
# test_runner_collect_ref.py's termination asserts
SEEDS = {("fast8_n5", 2 ** 32): 6, ("fast8_n6", 2 ** 32): 2, ("fast16_w3", 2 ** 32): 19,
         ("fast16_w7", 2 ** 32): 19, ("fast32_n17", 2 ** 31): 8, ("fast32_n17", 2 ** 32): 357,
         ("half64_n16", 2 ** 32): 19, ("gen_n3", 2 ** 32): 3, ("gen_w9_k3", 2 ** 31): 8,
         ("gen_w9_k3", 2 ** 32): 357, ("gen_w0", 2 ** 31): 8, ("gen_w0", 2 ** 32): 22}   # others: 1
WALK_D = (1, 2, 1, 3, 1, 4, 1, 1)


def pen_rows(case):
    W = len(case["grid"][0])
    per_row = (W + 1) // 2
    return -(-(case["N"] - 1) // per_row) if case["N"] > 1 else 0


def policy_grid(case):
    """The map rows ('.' free, '@' obstacle) of a policy case."""
    H, W = len(case["grid"]), len(case["grid"][0])
    nr = pen_rows(case)
    rows = [["@"] * W for _ in range(H)]
    for r in range(0, 2 * nr, 2):
        for c in range(0, W, 2):
            rows[r][c] = "."
    for c in range(5):
        rows[2 * nr][c] = "."
    for r in range(2 * nr + 2, H):
        for c in range(W):
            rows[r][c] = "."
    f0 = 2 * nr + 2
    for r, c in ((f0 + 1, 3), (H - 1, W - 2)):    # two obstacles in the field
        if r < H:
            rows[r][c] = "@"
    return ["".join(r) for r in rows]


def kind(case, b):
    """'never', 'field' or ('early', d) of env b."""
    if b == 2:
        return "never"
    if b % 3 == 2 and b > 5:
        return "field"
    k = len([x for x in range(b) if x != 2 and not (x % 3 == 2 and x > 5)])
    return ("early", WALK_D[k % len(WALK_D)])


def policy_instances(case, run):
    """(starts, goals) [B, N, 2] of one run of a policy case."""
    N, B = case["N"], case["B"]
    grid = runner_ref.parse_map(policy_grid(case))
    nr = pen_rows(case)
    W = grid.shape[1]
    pens = [(r, c) for r in range(0, 2 * nr, 2) for c in range(0, W, 2)]
    field = np.argwhere(grid == 0)
    field = field[field[:, 0] >= 2 * nr + 2]
    rng = np.random.RandomState(4242 + 1000 * run + N)
    starts = np.zeros((B, N, 2), np.int32)
    goals = np.zeros((B, N, 2), np.int32)
    for b in range(B):
        kd = kind(case, b)
        if kd == "field":
            starts[b] = field[rng.choice(len(field), N, replace=False)]
            goals[b] = field[rng.choice(len(field), N, replace=False)]
        elif kd == "never":
            if N == 1:
                starts[b, 0], goals[b, 0] = (2 * nr, 0), field[0]
            else:
                for n in range(N):
                    starts[b, n] = pens[n % len(pens)] if n < N - 1 else (2 * nr, 0)
                    goals[b, n] = pens[(n + 1) % len(pens)] if n < N - 1 else field[0]
        else:
            walker = b % N
            rest = [n for n in range(N) if n != walker]
            for i, n in enumerate(rest):
                starts[b, n] = goals[b, n] = pens[i]
            starts[b, walker] = (2 * nr, 4 - kd[1])
            goals[b, walker] = (2 * nr, 4)
    return starts, goals


def make_envs(case, grid_rows, starts, goals):
    return runner_ref.make_envs(runner_ref.parse_map(grid_rows), starts, goals, obs_window=case["win"],
                                obs_knn_agents=case["K"], episode_limit=case["limit"], **REWARDS)


def policy_mac(envs, seed, eps_q, record=None):
    """The checker's MAC: mapfx.rng.partial_policy_actions of envs[b] for b in bs, as they
    stand before the step, with counter t (global env id = b)."""
    from mapfx import rng

    def mac(batch, t, bs):
        avail, pd, d = policy_inputs([envs[b] for b in bs])
        a = rng.partial_policy_actions(seed, np.asarray(bs), t, eps_q, avail, pd, d)
        if record is not None:
            record.append((t, list(bs), a, [bool(envs[b].terminated) for b in bs]))
        return a

    return mac


_REF = {}


def policy_reference(name, eps_q, seed=None):
    """The restatement's result of RUNS runs of collect(eps) on a policy case, computed once
    per session: per run the instances, the policy seed, the final batch, the MAC calls,
    returns, lengths, t_env; and the log."""
    from mapfx import rng
    seed = SEEDS.get((name, eps_q), 1) if seed is None else seed
    key = (name, eps_q, seed)
    if key in _REF:
        return _REF[key]
    case = CASES[name]
    N, W, K, limit, B = case["N"], case["win"], case["K"], case["limit"], case["B"]
    grid_rows = policy_grid(case)
    ref = runner_ref.RefRunner(runner_log_interval=1)
    runs = []
    for r in range(RUNS):
        starts, goals = policy_instances(case, r)
        envs = make_envs(case, grid_rows, starts, goals)
        pseed = rng.runner_policy_seed(seed, r)
        macs = []
        batch = runner_ref.new_batch(B, limit + 1, N, 2 * W * W + 13 * K, fill=FILL)
        batch, calls, returns, lengths = ref.run(envs, batch, policy_mac(envs, pseed, eps_q, macs))
        runs.append(dict(starts=starts, goals=goals, pseed=pseed, batch=batch, calls=calls, macs=macs,
                         returns=np.array(returns, np.float64), lengths=np.array(lengths, np.int64),
                         t_env=ref.t_env))
    _REF[key] = dict(runs=runs, log=list(ref.log), seed=seed, grid=grid_rows)
    return _REF[key]


def unmet(case, res):
    """What a reference result lacks of: >= 3 distinct termination steps before the limit, an
    env that runs to the limit, two envs of one wave's env group (envs 2j, 2j + 1: every
    case here has an even number >= 2 of envs per wave) that end at different steps, and a
    stale actions row (an env in the MAC's bs that has terminated) -- in every run."""
    out = []
    for r, run in enumerate(res["runs"]):
        lengths, limit = run["lengths"], case["limit"]
        if len(set(lengths[lengths < limit].tolist())) < 3:
            out.append((r, "fewer than 3 distinct early terminations", lengths.tolist()))
        if not (lengths == limit).any():
            out.append((r, "no env runs to the limit"))
        if not any(lengths[j] != lengths[j + 1] for j in range(0, len(lengths) - 1, 2)):
            out.append((r, "no wave group with two termination steps"))
        if "macs" in run and not any(any(done) for _, _, _, done in run["macs"]):
            out.append((r, "no stale actions row"))
        if "macs" not in run and not any(
                lengths[b] <= t for t, bs in run["calls"] for b in bs):
            out.append((r, "no stale actions row"))
    return out


def given_reference(name):
    """The restatement's result of RUNS runs of collect(actions=table) on a matrix case: the
    matrix's own instances and seeded table (early terminations built in, one at step 0),
    the table read as it is (no avail rule: collect has no MAC to apply one)."""
    key = (name, "given")
    if key in _REF:
        return _REF[key]
    case = CASES[name]
    N, W, K, limit, B = case["N"], case["win"], case["K"], case["limit"], case["B"]
    ref = runner_ref.RefRunner(runner_log_interval=1)
    runs = []
    for r in range(RUNS):
        starts, goals, table = _instances(case, 1000 * r + 17 + N + W)
        envs = make_envs(case, case["grid"], starts, goals)
        batch = runner_ref.new_batch(B, limit + 1, N, 2 * W * W + 13 * K, fill=FILL)
        batch, calls, returns, lengths = ref.run(envs, batch, lambda batch, t, bs, table=table: table[t][bs])
        runs.append(dict(starts=starts, goals=goals, table=table, batch=batch, calls=calls,
                         returns=np.array(returns, np.float64), lengths=np.array(lengths, np.int64),
                         t_env=ref.t_env))
    _REF[key] = dict(runs=runs, log=list(ref.log), grid=case["grid"])
    return _REF[key]
