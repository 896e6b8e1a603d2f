#!/usr/bin/env python3
"""Time per episode step of ParallelRunner.collect (the episode loop as one launch,
mapfx_runner_rollout) against run() with a MAC, at `bench.py --env runner`'s shape: the yaml
config, 8 x 8, 15 agents, window 5, K 5, 4096 envs, 100-step episodes.

Legs, each a whole run (reset, the episode, the end-of-run totals) built from one checkout:
  run_table     (a) run() with a MAC that looks a device action table up (the existing path)
  collect_table (b) collect(actions=table), the same table
  collect_eps0  (c) collect(eps=0): pure shortest-path descent (episodes end early)
  collect_eps1  (d) collect(eps=1): uniform random moves
  collect_noobs (e) (b) with rows->obs = NULL: no observation rows built or written
  collect_pibt0 (f) collect(eps=0, policy="pibt"): priority inheritance with backtracking
  collect_pibt005 (f) collect(eps=0.05, policy="pibt")
  collect_pibt1 (f) collect(eps=1, policy="pibt")
The policy legs also report what their last run came to: the share of envs that ended with
every agent on its goal and the collisions per episode (the device's total_coll, read from
the state row after each env's last step).
  reset_only    reset() alone -- the new zeroed EpisodeBatch, the env reset, row 0 -- which
                every leg above pays once per run; `net` figures are a leg minus this one

Timing: wall clock (the legs differ in host work: that is the point) around enough runs of
a leg to fill --window seconds, device synchronised at both ends, every leg warmed first,
--reps alternations over all legs in one session.  us per episode step = window time /
(runs * episode steps), episode steps = the longest episode of the leg's run (100 where
no env ends early).  `total_us_per_run` is the whole run.  Bytes per step are algorithmic,
from shapes (bench.py's runner count for the legs with observation rows), against the
8 TB/s roofline.  `separated`: every repeat of the leg lies below every repeat of (a).

  python tools/runner_rollout_time.py [--window 1.0] [--reps 5] [--out profiles/runner_rollout_time.json]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mapf-marl_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_BYTES_PER_S = 8e12
LEGS = ("run_table", "collect_table", "collect_eps0", "collect_eps1", "collect_noobs", "collect_pibt0",
        "collect_pibt005", "collect_pibt1", "reset_only")
POLICY_LEGS = ("collect_eps0", "collect_eps1", "collect_pibt0", "collect_pibt005", "collect_pibt1")


class TableMAC:
    """select_actions: row bs of the table's time slice, on the device (one gather)."""

    def __init__(self, table):
        self.table = table

    def init_hidden(self, batch_size):
        pass

    def select_actions(self, batch, t_ep, t_env, bs, test_mode=False):
        return self.table[t_ep][bs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
    ap.add_argument("--reps", type=int, default=5, help="alternations over all legs")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "runner_rollout_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("runner_rollout_time needs a HIP device")
    import bench
    from mapfx import _abi, lib, rng
    from mapfx._abi import check
    from mapfx.episode import DeviceEpisodeBatch, OneHot
    from mapfx.maps import synthetic_instances
    from mapfx.runners import ParallelRunner

    S, N, B = 8, 15, a.envs
    inst = synthetic_instances(B, S, S, N, p_obstacle=0.0, seed=1)
    tmp = tempfile.mkdtemp(prefix="mapfx_runner_")
    mp = os.path.join(tmp, "empty-8-8.map")
    with open(mp, "w") as f:
        f.write("type octile\nheight 8\nwidth 8\nmap\n" + "\n".join(["." * 8] * 8) + "\n")
    ea = dict(bench.PARTIAL_YAML, grid_file_path=mp, agents_path=os.path.join(tmp, "x-"), n_agents=N)
    limit = bench.PARTIAL_YAML["episode_limit"]
    table = torch.as_tensor(rng.gen_actions(2, np.arange(B), np.arange(limit + 1), N)).cuda().to(torch.int64)

    def make():
        rargs = types.SimpleNamespace(env="marl_partial", batch_size_run=B, device="cuda:0", env_args=ea,
                                      episode_batch_cls=DeviceEpisodeBatch, test_nepisode=B,
                                      runner_log_interval=1 << 62, seed=0)
        r = ParallelRunner(rargs, None, instance_fn=lambda ep: (inst["init_pos"], inst["goals"]))
        info = r.get_env_info()
        scheme = {"state": {"vshape": info["state_shape"]},
                  "obs": {"vshape": info["obs_shape"], "group": "agents"},
                  "actions": {"vshape": (1,), "group": "agents", "dtype": torch.long},
                  "avail_actions": {"vshape": (info["n_actions"],), "group": "agents", "dtype": torch.int},
                  "reward": {"vshape": (1,)}, "terminated": {"vshape": (1,), "dtype": torch.uint8}}
        r.setup(scheme, {"agents": N}, {"actions": ("actions_onehot", [OneHot(out_dim=5)])}, TableMAC(table))
        return r

    def noobs(r):
        """collect(actions=table) with rows->obs = NULL (the ABI's own switch)."""
        r.reset()
        rows = type(r._erows).from_buffer_copy(r._erows)
        rows.obs = None
        check(lib.mapfx_runner_rollout(r.env._h, ctypes.byref(r.env._state), ctypes.byref(r._rs), 0,
                                       int(rows.max_t), table.data_ptr(), _abi.MAPFX_I64, None, None,
                                       ctypes.byref(rows), torch.cuda.current_stream().cuda_stream),
              "mapfx_runner_rollout")
        return r._finish(False)

    fns = {"run_table": lambda r: r.run(), "collect_table": lambda r: r.collect(actions=table),
           "collect_eps0": lambda r: r.collect(eps=0.0), "collect_eps1": lambda r: r.collect(eps=1.0),
           "collect_noobs": noobs, "collect_pibt0": lambda r: r.collect(eps=0.0, policy="pibt"),
           "collect_pibt005": lambda r: r.collect(eps=0.05, policy="pibt"),
           "collect_pibt1": lambda r: r.collect(eps=1.0, policy="pibt"), "reset_only": lambda r: r.reset()}
    runners, ep_steps, kernels = {}, {}, {}
    for leg in LEGS:                      # warm every leg: first batch, caches, code objects
        r = runners[leg] = make()
        for _ in range(3):
            fns[leg](r)
        torch.cuda.synchronize()
        ep_steps[leg] = int(r._ep_length.max().item()) if leg != "reset_only" else 1
        kernels[leg] = bench.kernel_instance(_abi.last_kernel())
    # faster and different is not faster: (a), (b) and (e) play the same episodes
    ra, rb = runners["run_table"], runners["collect_table"]
    for k, v in ra.batch.data.transition_data.items():
        assert torch.equal(v, rb.batch.data.transition_data[k]), k
        if k != "obs":
            assert torch.equal(v, runners["collect_noobs"].batch.data.transition_data[k]), k
    assert torch.equal(ra._ep_return, rb._ep_return) and torch.equal(ra._ep_length, rb._ep_length)

    def timed(leg, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fns[leg](runners[leg])
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    runs = {leg: max(3, int(np.ceil(a.window / (timed(leg, 5) / 5)))) for leg in LEGS}
    us = {leg: [] for leg in LEGS}
    for _ in range(a.reps):               # alternate over the legs
        for leg in LEGS:
            us[leg].append(timed(leg, runs[leg]) / runs[leg] * 1e6)
    D = runners["run_table"].env.obs_dim
    gd = runners["run_table"].env.goal_dist.element_size()
    # algorithmic bytes of one env step.  The EpisodeBatch rows (episode_buffer.py:100-134
    # layouts): actions i64 + one-hot f32 at ts, reward f32, terminated u8, and at ts + 1
    # state f32, avail i32, filled i64 and the obs f32 when built.  run(): the env step's own
    # bytes (bench.py's count; its observation rows go straight to the batch), the rows, the
    # MAC's gather (table row in, actions out and in again).  collect: per step the table row
    # (none with the policy), the four neighbour goal distances and the rows; once per
    # launch, so divided by the steps, the state in and out (tools/partial_rollout_time.py)
    def rows_b(obs):
        return 8 * N + 20 * N + 4 + 1 + 12 + 20 * N + 8 + (4 * D * N if obs else 0)

    def collect_b(obs, policy, T):
        per_launch = (27 * N + 13 + 16 * N + S * S // 8) + (27 * N + 9 + 8 * N) + 2 + 16
        return (0 if policy else 8 * N) + 4 * gd * N + rows_b(obs) + per_launch / T

    T = limit + 1
    by = {"run_table": bench.partial_bytes_per_env_step(N, D, S * S, gd) - 4 * D * N + rows_b(True) + 3 * 8 * N,
          "collect_table": collect_b(True, False, T), "collect_eps0": collect_b(True, True, T),
          "collect_eps1": collect_b(True, True, T), "collect_noobs": collect_b(False, False, T),
          "collect_pibt0": collect_b(True, True, T), "collect_pibt005": collect_b(True, True, T),
          "collect_pibt1": collect_b(True, True, T),
          "reset_only": 0}
    res = {}
    for leg in LEGS:
        per = [v / ep_steps[leg] for v in us[leg]]
        res[leg] = {"us_per_episode_step": [round(v, 3) for v in per], "min": round(min(per), 3),
                    "max": round(max(per), 3), "total_us_per_run": [round(v, 1) for v in us[leg]],
                    "episode_steps": ep_steps[leg], "runs_per_window": runs[leg], "kernel": kernels[leg],
                    "bytes_per_step": round(B * by[leg], 1),
                    "roofline_share_at_min": round(B * by[leg] / (min(per) * 1e-6) / HBM_BYTES_PER_S, 5)}
    for leg in POLICY_LEGS:               # the leg's last run, from its batch and env state
        r = runners[leg]
        last = r._ep_length.to(r.batch["state"].device).long().clamp(max=limit)
        coll = r.batch["state"][torch.arange(B, device=last.device), last, 0]
        res[leg]["completed_share"] = round(float(r.env.at_goal.bool().all(1).float().mean().item()), 4)
        res[leg]["collisions_per_episode"] = round(float(coll.float().mean().item()), 3)
    reset_us = float(np.median(us["reset_only"]))
    for leg in LEGS[:-1]:
        net = [(v - reset_us) / ep_steps[leg] for v in us[leg]]
        res[leg]["net_us_per_episode_step"] = [round(min(net), 3), round(max(net), 3)]
    for leg in LEGS[1:-1]:
        res[leg]["separated"] = res[leg]["max"] < res["run_table"]["min"]
    line = {"metric": "ParallelRunner us per episode step: collect (one launch) vs run() with a table MAC",
            "config": {"workload": "marl_partial yaml: 8x8 empty, 15 agents, window 5, K 5, %d envs, "
                                   "%d-step episodes; each leg a whole run" % (B, limit), "obs_dim": D},
            "timing": "wall clock around runs filling %.2f s per window, device synchronised at both ends, "
                      "%d alternations over the legs in one session" % (a.window, a.reps),
            "roofline": "algorithmic bytes per step over %.0f TB/s" % (HBM_BYTES_PER_S / 1e12),
            "legs": res, "build_id": _abi.build_id()}
    text = json.dumps(line)
    print(text)
    print("reset_only: %.1f-%.1f us per run" % (min(us["reset_only"]), max(us["reset_only"])))
    print("| leg | us per episode step | net of the reset | us per run | episode steps | separated from (a) |")
    print("|---|---|---|---|---|---|")
    for leg in LEGS[:-1]:
        print("| %s | %.2f-%.2f | %.2f-%.2f | %.0f-%.0f | %d | %s |" % (
            leg, res[leg]["min"], res[leg]["max"], *res[leg]["net_us_per_episode_step"], min(us[leg]),
            max(us[leg]), ep_steps[leg],
            "-" if leg == "run_table" else "yes" if res[leg]["separated"] else "no"))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
