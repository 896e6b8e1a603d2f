#!/usr/bin/env python3
"""Cost of the PRIMAL stay-on-goal blocking pass (mapfx_primal_blocking) at the bench's
primal shape -- 4096 worlds of 32 x 32, 16 agents, observation_size 10, 64 calls per
world per launch -- on "rooms with doors" worlds (walls every fifth row and column, one
door per wall segment, some agents parked on door goals), where the term is not 0.

Reports, as one JSON line (also written to --out):
  * the share of calls that are stays on a goal, and of those that are penalised;
  * the step kernel alone (start / stop events at the kernel's begin and end,
    mapfx_primal_act_timed), the blocking pass alone and step + pass (stream events
    around the launches), each the median of --reps launches replayed from the same
    positions after --warmup launches;
  * the CPU time of the plain-Python restatement (tests/primal_blocking_ref.py) for the
    blocking term of the same calls, measured on --cpu-worlds worlds, whose counts are
    compared with the device's.

  python tools/primal_blocking_time.py [--envs 4096] [--reps 20] [--out profiles/primal_blocking_time.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mapf-marl_amd"), os.path.join(REPO, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=64)
    ap.add_argument("--door-agents", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-worlds", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "primal_blocking_time.json"))
    a = ap.parse_args()
    import mapfx
    from mapfx import _abi, lib
    from mapfx._abi import check, ptr
    from primal_blocking_ref import BlockingWorld, rooms_world

    S, N, s_obs, E, K = 32, 16, 10, a.envs, a.calls
    rng = np.random.default_rng(11)
    grids = np.zeros((E, S, S), np.int8)
    starts = np.zeros((E, N, 2), np.int32)
    goals = np.zeros((E, N, 2), np.int32)
    ids = np.tile((np.arange(K) % N + 1).astype(np.int32), (E, 1))   # round robin, as bench.py
    acts = rng.integers(0, 5, size=(E, K)).astype(np.int32)
    for e in range(E):
        grids[e], st, gl, doors = rooms_world(rng, S, S, N, a.door_agents)
        starts[e], goals[e] = st, gl
        for d in doors:  # parked agents mostly stay
            sel = (ids[e] == d + 1) & (rng.random(K) < 0.8)
            acts[e, sel] = 0
    ids_d, acts_d = torch.from_numpy(ids).cuda(), torch.from_numpy(acts).cuda()
    stream = torch.cuda.current_stream()

    def timed(fn, pos0, batch):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(a.reps)]
        for e0, e1 in ev:  # creates the HIP events
            e0.record(stream)
            e1.record(stream)
        for i in range(a.warmup + a.reps):
            batch.pos.copy_(pos0)
            fn(ev[i - a.warmup] if i >= a.warmup else None)
        torch.cuda.synchronize()
        return median([e0.elapsed_time(e1) for e0, e1 in ev])

    # the step kernel alone, by its own begin / end events
    plain = mapfx.PrimalBatch(starts, goals, grids=grids, observation_size=s_obs)
    pos0 = plain.pos.clone()
    plain.act(ids_d, acts_d)
    step_kernel = _abi.last_kernel()
    step_ms = timed(lambda pr: plain.act(ids_d, acts_d, events=pr), pos0, plain)
    plain.check_err()

    # step + blocking pass: stream events around both launches
    b = mapfx.PrimalBatch(starts, goals, grids=grids, observation_size=s_obs, blocking=True)

    def both(pr):
        if pr:
            pr[0].record(stream)
        b.act(ids_d, acts_d)
        if pr:
            pr[1].record(stream)

    both_ms = timed(both, pos0, b)
    o = b.out
    pos_after = b.pos.clone()

    def pass_only(pr):  # the pass again on the launch's outputs (it rewrites the same values)
        if pr:
            pr[0].record(stream)
        check(lib.mapfx_primal_blocking(b._h, ctypes.byref(b._state), ptr(ids_d), ptr(acts_d), K,
                                        ptr(o["valid"]), ptr(o["on_goal"]), ptr(o["reward"]),
                                        ptr(o["blocking"]), ptr(o["n_blocking"]), stream.cuda_stream),
              "mapfx_primal_blocking")
        if pr:
            pr[1].record(stream)

    pass_ms = timed(pass_only, pos_after, b)
    pass_kernel = _abi.last_kernel()
    b.check_err()
    on_goal = o["on_goal"].cpu().numpy() != 0
    cnt = o["n_blocking"].cpu().numpy()
    stays = (acts == 0) & on_goal

    # the restatement's blocking term for the same calls, on the first worlds
    nw = min(a.cpu_worlds, E)
    cpu_s, agree = 0.0, True
    for e in range(nw):
        w = BlockingWorld(grids[e], starts[e], goals[e], size=s_obs)
        for k in range(K):
            aid, act = int(ids[e, k]) - 1, int(acts[e, k])
            w.world.move(aid, act)
            n = 0
            if act == 0 and w.world.pos[aid] == w.world.goals[aid]:
                t0 = time.perf_counter()
                n = w.blocking_count(aid)
                cpu_s += time.perf_counter() - t0
            agree &= n == int(cnt[e, k])
    line = {
        "metric": "PRIMAL stay-on-goal blocking pass, kernel time per launch",
        "config": {"workload": "%d rooms worlds of %dx%d, %d agents (%d parked on door goals), "
                               "observation_size %d, %d _step calls per world per launch"
                               % (E, S, S, N, a.door_agents, s_obs, K)},
        "calls": int(E * K), "stay_on_goal_share": round(float(stays.mean()), 4),
        "penalised_share_of_stays": round(float((cnt[stays] > 0).mean()), 4) if stays.any() else None,
        "step_kernel_ms": round(step_ms, 5), "step_plus_blocking_ms": round(both_ms, 5),
        "blocking_pass_ms": round(pass_ms, 5),
        "timing": "step: start/stop events at the kernel's begin/end; pass and step + pass: stream "
                  "events around the launches; median of %d launches after %d warm-up" % (a.reps, a.warmup),
        "cpu_restatement": {"worlds": nw, "blocking_term_s": round(cpu_s, 4),
                            "blocking_term_s_per_launch_scaled": round(cpu_s * E / nw, 3),
                            "counts_equal_device": bool(agree)},
        "kernels": [step_kernel, pass_kernel], "build_id": _abi.build_id()}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not agree:
        raise SystemExit("device counts differ from the restatement")


if __name__ == "__main__":
    main()
