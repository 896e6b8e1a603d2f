#!/usr/bin/env python3
"""Wall time of ParallelRunner.reset() with the three ways a run gets its instances:

  host      the default: _draw()'s per-env random.sample + parsing, set_agents (two H2D
            copies), the BFS tables
  device    args.runner_device_draw: mapfx_partial_draw, the BFS tables
  instance  instance_fn with one fixed instance (what bench.py --env runner passes): no
            draw, no copy, no BFS -- the floor

Shape: a 32 x 32 synthetic map with 10 % obstacles, N = 16, 25 generated scen files of
400 to 1000 lines, B = 1024 and B = 4096 (--envs).  Each timing is reset() plus
torch.cuda.synchronize(); the three forms are interleaved, --alternations rounds after
one warm-up round, medians reported.  --forms device runs one form alone (for a
`rocprofv3 --kernel-trace --stats` run of its own: the draw and BFS kernels' durations).
usage: python3 tools/reset_probe.py [--envs 1024 4096] [--alternations 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mapf-marl_amd")]

S, N, SEED = 32, 16, 5


def make_runner(form, B, mp, prefix, inst):
    import bench
    from mapfx.episode import DeviceEpisodeBatch, OneHot
    from mapfx.runners import ParallelRunner
    ea = dict(bench.PARTIAL_YAML, grid_file_path=mp, agents_path=prefix, n_agents=N)
    rargs = types.SimpleNamespace(env="marl_partial", batch_size_run=B, device="cuda:0", env_args=ea,
                                  seed=SEED, episode_batch_cls=DeviceEpisodeBatch, test_nepisode=B,
                                  runner_log_interval=1 << 62,
                                  runner_device_draw=(form == "device"))
    fn = (lambda ep: inst) if form == "instance" else None
    runner = ParallelRunner(rargs, None, instance_fn=fn)
    info = runner.get_env_info()
    scheme = {"state": {"vshape": info["state_shape"]},
              "obs": {"vshape": info["obs_shape"], "group": "agents"},
              "actions": {"vshape": (1,), "group": "agents", "dtype": torch.long},
              "avail_actions": {"vshape": (info["n_actions"],), "group": "agents", "dtype": torch.int},
              "reward": {"vshape": (1,)}, "terminated": {"vshape": (1,), "dtype": torch.uint8}}
    runner.setup(scheme, {"agents": N}, {"actions": ("actions_onehot", [OneHot(out_dim=5)])},
                 bench.RandomAvailMAC(seed=0))
    return runner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--forms", nargs="+", default=["host", "device", "instance"],
                    choices=["host", "device", "instance"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from mapfx import rng
    from mapfx.maps import load_scen_table, synthetic_instances, write_synthetic_scen
    assert torch.cuda.is_available(), "reset_probe needs a HIP device"
    grid = synthetic_instances(1, S, S, 2, p_obstacle=0.10, seed=SEED)["grid"][0]
    tmp = tempfile.mkdtemp(prefix="mapfx_reset_probe_")
    mp = os.path.join(tmp, "synthetic.map")
    with open(mp, "w") as f:
        f.write("type octile\nheight %d\nwidth %d\nmap\n" % (S, S))
        f.write("\n".join("".join("." if c == 0 else "@" for c in row) for row in grid) + "\n")
    prefix = os.path.join(tmp, "synthetic-random-")
    lengths = [400 + 25 * k for k in range(25)]   # 400 .. 1000
    write_synthetic_scen(prefix, grid, lengths, seed=SEED)
    lines, n_lines = load_scen_table(prefix, S, S)
    result = {"shape": {"side": S, "n_agents": N, "p_obstacle": 0.10, "scen_lines": lengths},
              "alternations": args.alternations, "unit": "us", "envs": {}}
    for B in args.envs:
        f, ln = rng.scen_draw(SEED, np.arange(B), 0, n_lines, N)   # the fixed instance: episode 0's
        rows = lines[f[:, None], ln].astype(np.int32)
        inst = (np.ascontiguousarray(rows[..., :2]), np.ascontiguousarray(rows[..., 2:]))
        runners = {form: make_runner(form, B, mp, prefix, inst) for form in args.forms}
        times = {form: [] for form in args.forms}
        for it in range(args.alternations + 1):
            for form, runner in runners.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                runner.reset()
                torch.cuda.synchronize()
                if it:   # round 0 warms up (code objects, the allocator's blocks)
                    times[form].append((time.perf_counter() - t0) * 1e6)
                runner.env.check_err()
                runner.batch = None
        result["envs"][str(B)] = {form: {"median": statistics.median(v), "min": min(v), "max": max(v)}
                                  for form, v in times.items()}
        for form, v in times.items():
            print("B %5d  %-8s reset median %10.1f us  (min %10.1f, max %10.1f, n %d)"
                  % (B, form, statistics.median(v), min(v), max(v), len(v)))
        del runners
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
