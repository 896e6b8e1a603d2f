#!/usr/bin/env python3
"""Cost of drawing PRIMAL worlds on the device (mapfx_primal_generate, PrimalBatch.regenerate)
at 4096 worlds in a 40 x 40 handle, 16 agents, the reference's SIZE = (10, 40) and
PROB = (0, .5).

Reports, as one JSON line (also written to --out), each device figure the median of --reps
launches after --warmup launches, timed by stream events around the launch:
  * a full regenerate (every world);
  * a regenerate with 1 world in 64 masked in (the reset-on-done case);
  * the host route to the same thing, timed by the wall clock on 64 worlds and stated per
    world: mapfx.maps.primal_world per world (the reference's Python generator), the worlds
    embedded in the 40 x 40 grid, a PrimalBatch built from them (checks, handle, upload);
  * for scale, one K = 64 mapfx_primal_act launch at the bench's primal shape (4096 worlds
    of 32 x 32, 16 agents, observation_size 10) by the kernel's own events.

  python tools/primal_generate_time.py [--envs 4096] [--reps 20] [--out profiles/primal_generate_time.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mapf-marl_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-worlds", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "primal_generate_time.json"))
    a = ap.parse_args()
    import mapfx
    from mapfx import _abi
    from mapfx.maps import primal_world, synthetic_instances

    S, N, E, SIZE, PROB = 40, 16, a.envs, (10, 40), (0, .5)
    b = mapfx.PrimalBatch.random(E, N, (S, S), seed=1, SIZE=SIZE, PROB=PROB)
    kernel = _abi.last_kernel()
    b.check_err()
    stream = torch.cuda.current_stream()

    def timed(fn):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(a.reps)]
        for i in range(a.warmup + a.reps):
            if i >= a.warmup:
                ev[i - a.warmup][0].record(stream)
            fn()
            if i >= a.warmup:
                ev[i - a.warmup][1].record(stream)
        torch.cuda.synchronize()
        return median([e0.elapsed_time(e1) for e0, e1 in ev])

    sparse = (torch.arange(E, device=b.device) % 64 == 0).to(torch.uint8)
    full_ms = timed(lambda: b.regenerate())
    sparse_ms = timed(lambda: b.regenerate(mask=sparse))
    keep_ms = timed(lambda: b.regenerate(keep_map=True))
    b.check_err()
    episodes = int(b.episode.min().item()), int(b.episode.max().item())

    # ---- the host route, per world ----
    n = a.host_worlds
    np.random.seed(1)
    import random
    random.seed(1)
    t0 = time.perf_counter()
    grids = -np.ones((n, S, S), dtype=np.int8)
    starts = np.zeros((n, N, 2), dtype=np.int32)
    goals = np.zeros((n, N, 2), dtype=np.int32)
    for e in range(n):
        world, gl = primal_world(N, SIZE=SIZE, PROB=PROB)
        s = world.shape[0]
        grids[e, :s, :s] = np.where(world < 0, -1, 0)
        for i in range(1, N + 1):
            starts[e, i - 1] = np.argwhere(world == i)[0]
            goals[e, i - 1] = np.argwhere(gl == i)[0]
    t1 = time.perf_counter()
    hb = mapfx.PrimalBatch(starts, goals, grids=grids)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    del hb

    # ---- one K = 64 act launch at the bench shape, by the kernel's own events ----
    Sb, K = 32, 64
    inst = synthetic_instances(E, Sb, Sb, N, p_obstacle=0.10, seed=1)
    pb = mapfx.PrimalBatch(inst["init_pos"], inst["goals"], bits=inst["bits"], hw=(Sb, Sb))
    g = torch.Generator().manual_seed(3)
    ids = (torch.arange(K, dtype=torch.int32) % N + 1).repeat(E, 1).cuda()
    acts = torch.randint(0, 5, (E, K), generator=g, dtype=torch.int32).cuda()
    ts = []
    for i in range(a.warmup + a.reps):
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record(stream)    # torch creates the HIP events at their first record()
        ev[1].record(stream)
        pb.act(ids, acts, events=ev)
        torch.cuda.synchronize()
        if i >= a.warmup:
            ts.append(ev[0].elapsed_time(ev[1]))
    act_ms = median(ts)
    act_kernel = _abi.last_kernel()

    line = {
        "metric": "PRIMAL device world generation (regenerate), time per launch",
        "config": {"workload": "%d worlds in a %dx%d handle, %d agents, SIZE %s, PROB %s"
                               % (E, S, S, N, list(SIZE), list(PROB))},
        "regenerate_all_ms": round(full_ms, 5),
        "regenerate_all_us_per_world": round(full_ms * 1e3 / E, 4),
        "regenerate_1_in_64_ms": round(sparse_ms, 5),
        "regenerate_keep_map_ms": round(keep_ms, 5),
        "episodes_drawn_per_world": list(episodes),
        "host_worlds": n,
        "host_primal_world_ms_per_world": round((t1 - t0) * 1e3 / n, 4),
        "host_batch_build_upload_ms_per_world": round((t2 - t1) * 1e3 / n, 4),
        "host_route_ms_per_world": round((t2 - t0) * 1e3 / n, 4),
        "host_route_vs_device_per_world": round((t2 - t0) / n / (full_ms * 1e-3 / E), 1),
        "act_k64_bench_shape_ms": round(act_ms, 5),
        "act_k64_bench_shape_ms_design_6f": 0.0325,
        "timing": "device: stream events around each launch, median of %d launches after %d warm-up; "
                  "host: wall clock over %d worlds; act: the kernel's own start / stop events"
                  % (a.reps, a.warmup, n),
        "kernels": [kernel, act_kernel], "build_id": _abi.build_id()}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
