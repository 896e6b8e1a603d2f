"""Expected episodes of the MARL_PARTIAL fused rollout (MarlPartialBatch.rollout) from the
restatement alone: tests/test_partial_policy_ref.py on the CPU, tests/test_gpu_partial_rollout.py
on the device.  TEST INFRASTRUCTURE ONLY; no test lives here.  The cases, instances and the
comparer are tests/partial_step_cases.py's; mapfx.rng.partial_policy_actions is the policy.
"""
from __future__ import annotations

import functools

import numpy as np

from partial_step_cases import BY_NAME, STEPS, as_device, build, compare, lane_group, make_refs, snapshot, table_bytes, is_big

# the given-action cases of the issue: every way the rollout instance can differ
GIVEN_CASES = ("fast-w5-l16-u8t", "fast-w5-l8-i16", "fast-w5-l32-u8", "fast-w3-l16-i16t",
               "fast-w7-l16-i16", "fast-half-64x60", "fast-w5-l16-i32",
               "gen-w0-n2", "gen-w1-n1", "gen-w9-n40-k4", "gen-w7-n12-k3", "wg-w3-n70")
POLICY_CASES = ("fast-w5-l16-u8t", "fast-w5-l16-i16", "gen-w5-n3")
POLICY_EPS = (0, 2 ** 30, 2 ** 32)
POLICY_PHASES = ("fresh", "mid")       # straight after compute_goal_dist / after two given steps
POLICY_SEED = 0x5EED0F1A9
OFF_GRID_D = 0      # what the expected episode feeds as d_m of an off-grid neighbour: the best
#                     possible distance, which the clear avail bit must keep from being taken


def expected_rollout_kernel(c, obs):
    """pick_roll() of csrc/partial.hip: (name, template arguments without spaces), None on
    the workgroup path (no fused kernel)."""
    if is_big(c.H, c.W, c.N):
        return None
    L = lane_group(c.N)
    gde = {1: 1, 2: 2, 4: 0}[table_bytes(c.H, c.W)]
    if not obs:
        return ("partial_rollout_kernel", "0,5,%d,%d,false" % (L, gde) if L in (8, 16, 32) else "0,0,0,0,false")
    if c.K == 5 and (c.win, L) in ((5, 16), (5, 8), (5, 32), (3, 16), (7, 16)):
        return ("partial_rollout_kernel", "%d,5,%d,%d,true" % (c.win, L, gde))
    return ("partial_rollout_kernel", "%d,0,0,0,true" % c.win)


def rollout_kernel_args(printed):
    import re
    m = re.search(r"(partial_rollout_kernel)<([^>]*)>", printed)
    return (m.group(1), m.group(2).replace(" ", "")) if m else None


def policy_inputs(refs):
    """(avail masks [E, N], pd [E, N], d [E, N, 4]) of the envs' current (pre-step) state."""
    E, N = len(refs), refs[0].n
    avail = np.zeros((E, N), np.int64)
    pd = np.zeros((E, N), np.int64)
    d = np.full((E, N, 4), OFF_GRID_D, np.int64)
    for e, r in enumerate(refs):
        avail[e] = (r.avail().astype(np.int64) << np.arange(5)).sum(-1)
        for i, (y, x) in enumerate(r.pos):
            tab = r.goal_dist[i]
            pd[e, i] = tab[y * r.w + x]
            for m, (dy, dx) in enumerate(STEPS):
                if 0 <= y + dy < r.h and 0 <= x + dx < r.w:
                    d[e, i, m] = tab[(y + dy) * r.w + x + dx]
    return avail, pd, d


def policy_counts(seed, env_ids, t, eps_q, avail, pd, d):
    """How often each branch of the rule occurs in one step: (ties among the best
    neighbours, unavailable neighbours that would have been best, explore draws, greedy
    stays)."""
    from mapfx import rng
    N = pd.shape[1]
    env = np.asarray(env_ids, np.int64).astype(np.uint64)[:, None]
    with np.errstate(over="ignore"):
        u = rng.splitmix64(np.uint64(seed) ^ env * rng.K_ENV ^ np.uint64(t & 0xFFFFFFFF) * rng.K_T
                           ^ np.arange(N, dtype=np.uint64)[None, :] * rng.K_AGENT)
    explore = (u >> np.uint64(32)) < np.uint64(eps_q)
    bit = ((avail[..., None] >> np.arange(4)) & 1) == 1
    ok = bit & (d >= 0)
    big = np.iinfo(np.int64).max
    dm = np.where(ok, d, big)
    best = dm.min(-1)
    improving = (pd >= 0) & (best < pd)
    ties = ~explore & improving & ((dm == best[..., None]).sum(-1) >= 2)
    passed = ~explore & (~bit & (d >= 0) & (d < np.minimum(best, pd)[..., None])).any(-1)
    return np.array([ties.sum(), passed.sum(), explore.sum(), (~explore & ~improving).sum()])


def policy_episode(refs, T, eps_q, seed, t0=0, env_ids=None, autoreset=False):
    """The restatement stepped T times under the policy.  Returns (actions int8 [T, E, N],
    snapshots after each step, branch counts [4])."""
    from mapfx import rng
    ids = np.arange(len(refs)) if env_ids is None else np.asarray(env_ids)
    acts, snaps, counts = [], [], np.zeros(4, np.int64)
    for k in range(T):
        if autoreset:
            for r in refs:
                if r.terminated:
                    r.reset()
        avail, pd, d = policy_inputs(refs)
        a = rng.partial_policy_actions(seed, ids, t0 + k, eps_q, avail, pd, d)
        counts += policy_counts(seed, ids, t0 + k, eps_q, avail, pd, d)
        for e, r in enumerate(refs):
            r.step(a[e])
        acts.append(a)
        snaps.append(snapshot(refs))
    return np.stack(acts), snaps, counts


@functools.lru_cache(maxsize=None)
def policy_run(name, eps_q, phase):
    """The expected policy episode of a GPU policy test: `pre` given steps of the case's
    own actions first (phase "mid": 2), then T = c.T - pre policy steps at t0 = pre."""
    c = BY_NAME[name]
    b = build(c)
    refs = make_refs(c, b)
    pre = 2 if phase == "mid" else 0
    for t in range(pre):
        for e, r in enumerate(refs):
            r.step(b["actions"][t, e])
    acts, snaps, counts = policy_episode(refs, c.T - pre, eps_q, POLICY_SEED, t0=pre)
    return dict(pre=pre, T=c.T - pre, actions=acts, snaps=snaps, counts=counts)


def compare_slot(c, traj, k, snap, obs=True):
    """compare() of slot k of a trajectory dict (device tensors or arrays) with a snapshot:
    reward, obs, state, avail, and pos / terminated as the state after that step."""
    batch, out = as_device(c, snap)
    host = lambda x: x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)  # noqa: E731
    batch.pos = host(traj["pos"][k])
    batch.terminated = host(traj["terminated"][k])
    for f in ("reward", "state", "avail") + (("obs",) if obs else ()):
        out[f] = host(traj[f][k])
    return compare(batch, out, snap, k)


def autoreset_episode(c, b, actions, limit):
    """The host loop of the autoreset contract: before every step the refs whose terminated
    flag is set are reset, then all step.  Returns (snapshots after each step, the set of
    steps at which envs 1 and 2 restarted)."""
    refs = make_refs(c, b, limit)
    snaps, restarts = [], {1: [], 2: []}
    for k in range(len(actions)):
        for e, r in enumerate(refs):
            if r.terminated:
                r.reset()
                if e in restarts:
                    restarts[e].append(k)
        for e, r in enumerate(refs):
            r.step(actions[k, e])
        snaps.append(snapshot(refs))
    return snaps, restarts
