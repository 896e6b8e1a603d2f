#!/usr/bin/env python3
"""Cost of the PRIMAL read-only query (mapfx_primal_observe) at the bench's primal shape
-- 4096 worlds of 32 x 32 (10 % obstacles), 16 agents, observation_size 10 -- after 64
random calls per world.

Reports, as one JSON line (also written to --out), each figure the median of --reps
launches after --warmup launches, timed by stream events around the launch:
  * observe() of all agents (Q = N);
  * the only way to the same data without it: mapfx_primal_act with K = N round-robin
    stays (replayed from the same positions; non-diagonal, so a stay moves nothing);
  * observe() of one agent per world (Q = 1);
  * the output bytes of the all-agent observe divided by its time.
The two all-agent results are compared on the device before anything is reported.

  python tools/primal_observe_time.py [--envs 4096] [--reps 20] [--out profiles/primal_observe_time.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mapf-marl_amd")]

import torch  # noqa: E402


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "primal_observe_time.json"))
    a = ap.parse_args()
    import mapfx
    from mapfx import _abi
    from mapfx.maps import synthetic_instances

    S, N, s_obs, E, K0 = 32, 16, 10, a.envs, 64
    inst = synthetic_instances(E, S, S, N, p_obstacle=0.10, seed=1)
    b = mapfx.PrimalBatch(inst["init_pos"], inst["goals"], bits=inst["bits"], hw=(S, S),
                          observation_size=s_obs)
    g = torch.Generator().manual_seed(3)
    b.act(torch.randint(1, N + 1, (E, K0), generator=g, dtype=torch.int32).cuda(),
          torch.randint(0, 5, (E, K0), generator=g, dtype=torch.int32).cuda())
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

    ids_all = torch.arange(1, N + 1, dtype=torch.int32).repeat(E, 1).cuda()
    stay = torch.zeros((E, N), dtype=torch.int32).cuda()
    one = torch.randint(1, N + 1, (E, 1), generator=g, dtype=torch.int32).cuda()

    o = b.observe()
    observe_kernel = _abi.last_kernel()
    s_out = b.act(ids_all, stay)
    stay_kernel = _abi.last_kernel()
    same = all(torch.equal(o[k].view(torch.uint8), s_out[k].view(torch.uint8))
               for k in ("obs", "vec", "next_mask", "on_goal", "done"))
    out_bytes = sum(v.numel() * v.element_size() for v in o.values())

    all_ms = timed(lambda: b.observe())
    stay_ms = timed(lambda: b.act(ids_all, stay))
    one_ms = timed(lambda: b.observe(one))
    b.check_err()
    line = {
        "metric": "PRIMAL read-only query (observe), time per launch",
        "config": {"workload": "%d worlds of %dx%d, %d agents, observation_size %d, after %d random "
                               "_step calls per world" % (E, S, S, N, s_obs, K0)},
        "observe_all_ms": round(all_ms, 5), "stay_calls_ms": round(stay_ms, 5),
        "observe_one_ms": round(one_ms, 5),
        "observe_all_vs_stay_calls": round(all_ms / stay_ms, 4),
        "observe_all_output_bytes": int(out_bytes),
        "observe_all_output_GBps": round(out_bytes / (all_ms * 1e-3) / 1e9, 2),
        "views": int(E * N), "equal_to_stay_calls": bool(same),
        "timing": "stream events around each launch; median of %d launches after %d warm-up"
                  % (a.reps, a.warmup),
        "kernels": [observe_kernel, stay_kernel], "build_id": _abi.build_id()}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not same:
        raise SystemExit("observe() differs from the stay calls")


if __name__ == "__main__":
    main()
