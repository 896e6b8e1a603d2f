#!/usr/bin/env python3
"""Time per env step of MARL_PARTIAL output mode -- `step` against `step + repair`
(mapfx_partial_step, then mapfx_partial_repair with its observe launch) -- at
`bench.py --env marl_partial`'s shape: the yaml config, 8 x 8, 15 agents, window 5, K 5,
4096 envs, uniform random actions (rng.gen_actions).

The method of tools/partial_rollout_time.py: each leg is ONE captured HIP graph of [reset
with no outputs, then T steps], so both legs pay the same reset launch and no Python between
launches; stream events around enough replays to fill --window seconds, --reps alternations
over the legs in one session; ms per step = window time / (replays * T).
  step          T mapfx_partial_step launches (output=False)
  step_repair   T x [copy of pos, mapfx_partial_step, partial_repair_kernel, observe launch]
The step_repair leg also reports, over the T steps of one replay, the share of env-steps that
needed a repair (flags != 0) and the share that ended at the round cap.

  python tools/partial_repair_time.py [--window 1.0] [--reps 5] [--T 32]
                                      [--out profiles/partial_repair_time.json]
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

LEGS = ("step", "step_repair")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
    ap.add_argument("--reps", type=int, default=5, help="alternations over the legs")
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "partial_repair_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("partial_repair_time needs a HIP device")
    import bench
    import mapfx
    from mapfx import _abi, lib, rng
    from mapfx._abi import check, ptr
    from mapfx.maps import synthetic_instances

    S, N, E, T = 8, 15, a.envs, a.T
    inst = synthetic_instances(E, S, S, N, p_obstacle=0.0, seed=1)
    grids = np.zeros((1, S, S), dtype=np.int8)
    acts = torch.as_tensor(rng.gen_actions(2, np.arange(E), np.arange(T), N)).cuda()
    stream = torch.cuda.current_stream()

    def quiet_reset(b):     # reset of every env, no outputs
        none = _abi.POut(reward=None, obs=None, state=None, avail=None, err=ptr(b.err))
        check(b._call(lib.mapfx_partial_reset, b._h, ctypes.byref(b._state), None, ctypes.byref(none)),
              "mapfx_partial_reset")

    graphs, batches = {}, {}
    for leg in LEGS:
        b = mapfx.MarlPartialBatch(inst["init_pos"], inst["goals"], grids=grids, output=leg == "step_repair",
                                   repair_seed=3, **bench.PARTIAL_YAML)
        b.reset()
        side = torch.cuda.Stream()
        side.wait_stream(stream)
        with torch.cuda.stream(side):       # eager warm-up of every launch before capture
            quiet_reset(b)
            for k in range(T):
                b.step(acts[k])
        stream.wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            quiet_reset(b)
            for k in range(T):
                b.step(acts[k])
        for _ in range(20):
            g.replay()
        torch.cuda.synchronize()
        graphs[leg], batches[leg] = g, b
    # the repair's share: one eager pass over the same T steps, reading the flags after each
    b = batches["step_repair"]
    quiet_reset(b)
    needed = capped = 0
    for k in range(T):
        b.step(acts[k])
        fl = b.repair_flags.cpu().numpy()
        needed += int((fl != 0).sum())
        capped += int(((fl & 12) != 0).sum())
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
    for _ in range(a.reps):
        for leg in LEGS:
            ms[leg].append(timed(graphs[leg], replays[leg]) / (replays[leg] * T) * 1e3)
    res = {leg: {"ms_per_step": [round(v, 6) for v in ms[leg]], "min": round(min(ms[leg]), 6),
                 "max": round(max(ms[leg]), 6), "replays_per_window": replays[leg]} for leg in LEGS}
    res["step_repair"]["repaired_share"] = round(needed / (E * T), 4)
    res["step_repair"]["capped_share"] = round(capped / (E * T), 4)
    line = {"metric": "MARL_PARTIAL ms per env step of E envs: step vs step + repair (output mode)",
            "config": {"workload": "marl_partial yaml: 8x8 empty, 15 agents, window 5, K 5, %d envs, uniform "
                                   "random actions; each leg one graph of [reset without outputs, %d steps]"
                                   % (E, T)},
            "timing": "stream events around replays filling %.2f s per window, %d alternations over the legs "
                      "in one session; ms per step = window / (replays * T), reset launch included"
                      % (a.window, a.reps),
            "legs": res, "build_id": _abi.build_id()}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
