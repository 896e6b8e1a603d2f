#!/usr/bin/env python3
"""Time per env step of the MARL_PARTIAL fused rollout (mapfx_partial_rollout) against the
step path, at `bench.py --env marl_partial`'s shape: the yaml config, 8 x 8, 15 agents,
window 5, K 5, 4096 envs.

Legs, for T in {1, 8, 32, 64}; every leg is ONE captured HIP graph of [reset with no
outputs, then T steps], so all legs pay the same reset launch and no Python between
launches:
  loop_obs      T mapfx_partial_step launches (the existing step path, with obs)
  loop_noobs    T mapfx_partial_step launches with out.obs = NULL
  fused_obs     (a) one partial_rollout_kernel launch, given actions, with obs
  fused_noobs   (b) ... obs=False
  policy_eps0   (c) ... the on-device policy, eps_q = 0, obs=False
  policy_eps1   (c) ... eps_q = 2**32, obs=False
  pibt_eps0     (d) (c) under policy="pibt" (priority inheritance with backtracking), eps_q = 0
  pibt_eps005   (d) ... eps 0.05
  pibt_eps1     (d) ... eps_q = 2**32
The policy legs also report what their episodes came to after [reset, T steps]: the share of
envs with every agent on its goal and the device's total_coll per env.

Timing: stream events around enough replays of a leg's graph to fill --window seconds
(calibrated per leg after its warm-up), --reps alternations over all legs in one session;
ms per step = window time / (replays * T), reported as the list, its min and max.  Bytes per
step are algorithmic, from shapes (rollout_bytes_per_env_step below; the loop legs use
bench.py's partial_bytes_per_env_step), and their share of the 8 TB/s roofline follows.
`separated`: every repeat of fused_noobs below every repeat of loop_noobs at that T.

  python tools/partial_rollout_time.py [--window 1.0] [--reps 5] [--T 64] [--legs policy_eps0 pibt_eps0]
                                        [--out profiles/partial_rollout_time.json]
"""
import argparse
import ctypes
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mapf-marl_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_BYTES_PER_S = 8e12
ALL_LEGS = ("loop_obs", "loop_noobs", "fused_obs", "fused_noobs", "policy_eps0", "policy_eps1", "pibt_eps0",
            "pibt_eps005", "pibt_eps1")


def rollout_bytes_per_env_step(N, D, HW, gd_bytes, T, obs, policy):
    """Algorithmic HBM bytes of one env step inside a fused rollout of T steps: per step the
    given actions (N), the four neighbour goal distances per agent (4 gd_bytes N) and the
    trajectory slots (reward 8, state 12, avail N, pos 8N, terminated 1, obs 4DN when built,
    the policy's actions N); once per launch, so divided by T, the state in and out (27N + 13
    + goal / init 16N + bitmap HW/8 in, 27N + 9 + carried neighbours 8N out)."""
    per_step = (0 if policy else N) + 4 * gd_bytes * N + 8 + 12 + N + 8 * N + 1 + \
        (4 * D * N if obs else 0) + (N if policy else 0)
    per_launch = (27 * N + 13 + 16 * N + HW // 8) + (27 * N + 9 + 8 * N)
    return per_step + per_launch / T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
    ap.add_argument("--reps", type=int, default=5, help="alternations over all legs")
    ap.add_argument("--T", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--legs", nargs="+", default=list(ALL_LEGS), choices=ALL_LEGS)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "partial_rollout_time.json"))
    a = ap.parse_args()
    LEGS = tuple(leg for leg in ALL_LEGS if leg in a.legs)
    if not torch.cuda.is_available():
        raise SystemExit("partial_rollout_time needs a HIP device")
    import bench
    import mapfx
    from mapfx import _abi, lib, rng
    from mapfx._abi import check, ptr
    from mapfx.maps import synthetic_instances

    S, N, E = 8, 15, a.envs
    inst = synthetic_instances(E, S, S, N, p_obstacle=0.0, seed=1)
    grids = np.zeros((1, S, S), dtype=np.int8)
    Tmax = max(a.T)
    acts = torch.as_tensor(rng.gen_actions(2, np.arange(E), np.arange(Tmax), N)).cuda()
    stream = torch.cuda.current_stream()

    def make():
        b = mapfx.MarlPartialBatch(inst["init_pos"], inst["goals"], grids=grids, **bench.PARTIAL_YAML)
        b.reset()
        return b

    def quiet_reset(b):     # reset of every env, no outputs
        none = _abi.POut(reward=None, obs=None, state=None, avail=None, err=ptr(b.err))
        check(b._call(lib.mapfx_partial_reset, b._h, ctypes.byref(b._state), None, ctypes.byref(none)),
              "mapfx_partial_reset")

    def leg_fn(leg, b, T):
        if leg == "loop_obs":
            return lambda: [b.step(acts[k]) for k in range(T)]
        if leg == "loop_noobs":
            out = _abi.POut(reward=ptr(b.out["reward"]), obs=None, state=ptr(b.out["state"]),
                            avail=ptr(b.out["avail"]), err=ptr(b.err))
            return lambda: [check(b._call(lib.mapfx_partial_step, b._h, ctypes.byref(b._state),
                                          ptr(acts[k]), _abi.MAPFX_I8, ctypes.byref(out)),
                                  "mapfx_partial_step") for k in range(T)]
        if leg == "fused_obs":
            return lambda: b.rollout(acts[:T])
        if leg == "fused_noobs":
            return lambda: b.rollout(acts[:T], obs=False)
        eps_q = 0 if leg.endswith("eps0") else int(round(0.05 * 2 ** 32)) if leg.endswith("eps005") else 2 ** 32
        rule = "pibt" if leg.startswith("pibt") else "descent"
        return lambda: b.rollout(T=T, eps=eps_q, seed=3, obs=False, policy=rule)

    D = None
    results = {}
    for T in a.T:
        graphs, kernels, batches = {}, {}, {}
        for leg in LEGS:
            b = make()
            D = b.obs_dim
            fn = leg_fn(leg, b, T)
            side = torch.cuda.Stream()
            side.wait_stream(stream)
            with torch.cuda.stream(side):       # eager warm-up of every launch before capture
                quiet_reset(b)
                fn()
            stream.wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                quiet_reset(b)
                fn()
            kernels[leg] = bench.kernel_instance(_abi.last_kernel())
            for _ in range(20):
                g.replay()
            torch.cuda.synchronize()
            graphs[leg], batches[leg] = g, b
        if T == min(8, Tmax) and set(ALL_LEGS[:4]) <= set(LEGS):   # faster and different is not faster: the legs agree
            ref = batches["loop_obs"]
            for leg in ("loop_noobs", "fused_obs", "fused_noobs"):
                for f in ("pos", "t", "total_coll", "pdist"):
                    assert torch.equal(getattr(batches[leg], f), getattr(ref, f)), (leg, f)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed(g, n):
            e0.record(stream)
            for _ in range(n):
                g.replay()
            e1.record(stream)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        replays = {leg: max(10, int(math.ceil(a.window / (timed(graphs[leg], 50) / 50)))) for leg in LEGS}
        ms = {leg: [] for leg in LEGS}
        for _ in range(a.reps):                 # alternate over the legs
            for leg in LEGS:
                ms[leg].append(timed(graphs[leg], replays[leg]) / (replays[leg] * T) * 1e3)
        gd = batches[LEGS[0]].goal_dist.element_size()
        full = bench.partial_bytes_per_env_step(N, D, S * S, gd)
        by = {"loop_obs": full, "loop_noobs": full - 4 * D * N,
              "fused_obs": rollout_bytes_per_env_step(N, D, S * S, gd, T, True, False),
              "fused_noobs": rollout_bytes_per_env_step(N, D, S * S, gd, T, False, False),
              "policy_eps0": rollout_bytes_per_env_step(N, D, S * S, gd, T, False, True),
              "policy_eps1": rollout_bytes_per_env_step(N, D, S * S, gd, T, False, True),
              "pibt_eps0": rollout_bytes_per_env_step(N, D, S * S, gd, T, False, True),
              "pibt_eps005": rollout_bytes_per_env_step(N, D, S * S, gd, T, False, True),
              "pibt_eps1": rollout_bytes_per_env_step(N, D, S * S, gd, T, False, True)}
        res = {}
        for leg in LEGS:
            lo, hi = min(ms[leg]), max(ms[leg])
            res[leg] = {"ms_per_step": [round(v, 6) for v in ms[leg]], "min": round(lo, 6), "max": round(hi, 6),
                        "replays_per_window": replays[leg], "kernel": kernels[leg],
                        "bytes_per_step": round(E * by[leg], 1),
                        "roofline_share_at_min": round(E * by[leg] / (lo * 1e-3) / HBM_BYTES_PER_S, 5)}
            if leg in ALL_LEGS[4:]:     # the state the last replay left: [reset, T policy steps]
                bt = batches[leg]
                res[leg]["completed_share"] = round(float(bt.at_goal.bool().all(1).float().mean().item()), 4)
                res[leg]["collisions_per_env"] = round(float(bt.total_coll.float().mean().item()), 3)
        res["separated"] = ("fused_noobs" in ms and "loop_noobs" in ms and
                            max(ms["fused_noobs"]) < min(ms["loop_noobs"]))
        results[str(T)] = res
        del graphs, batches
    line = {"metric": "MARL_PARTIAL ms per env step of E envs: fused rollout vs the step loop",
            "config": {"workload": "marl_partial yaml: 8x8 empty, 15 agents, window 5, K 5, %d envs; each "
                                   "leg one graph of [reset without outputs, T steps]" % E, "obs_dim": D},
            "timing": "stream events around replays filling %.2f s per window, %d alternations over the "
                      "legs in one session; ms per step = window / (replays * T), reset launch included"
                      % (a.window, a.reps),
            "roofline": "algorithmic bytes per step over %.0f TB/s" % (HBM_BYTES_PER_S / 1e12),
            "T": results, "build_id": _abi.build_id()}
    text = json.dumps(line)
    print(text)
    print("| T | " + " | ".join(LEGS) + " | (b) separated |")
    print("|---|" + "---|" * (len(LEGS) + 1))
    for T in a.T:
        r = results[str(T)]
        print("| %d | " % T + " | ".join("%.2f-%.2f" % (r[leg]["min"] * 1e3, r[leg]["max"] * 1e3) for leg in LEGS)
              + " | %s |" % ("yes" if r["separated"] else "no"))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
