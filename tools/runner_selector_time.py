#!/usr/bin/env python3
"""Wall time per runner step of ParallelRunner.run() with the action selection in torch
against the device selector (mapfx.selectors, one launch of mapfx_select_actions), at
`bench.py --env runner`'s shape: the yaml config, 8 x 8, 15 agents, window 5, K 5, 4096 envs,
100-step episodes.

Both legs use one MAC: Q = 0.01 * the first five observation features of the env's own row
(elementwise, no matmul; sliced before the `bs` gather so that the part the legs share stays
small), then the selector at a fixed epsilon.
  torch_padded    (a) PyMARL's epsilon-greedy chain restated in torch (mask fill, rand,
                      Categorical(avail).sample(), max, blend), the padded `bs`.  Like the
                      reference it builds Categorical with argument validation on, which
                      reads a device value on the host at every call
  torch_novalid   (a') the same with validate_args=False: no host read in the selector
  device_padded   (b) DeviceEpsilonGreedySelector, the padded `bs`
  torch_exact     (a) with args.runner_exact_bs (one host synchronisation per step)
  device_exact    (b) with args.runner_exact_bs
The device legs' two forms must fill byte-identical batches (asserted); the torch legs draw
other numbers from the same distribution, so their episodes differ from the device legs'.

Timing: wall clock around enough runs of a leg to fill --window seconds, device synchronised
at both ends, every leg warmed first, --reps alternations over all legs in one session; us
per step = window time / the loop iterations of its runs (runner.t); the median over the
repeats is the figure, min and max its spread.

  python tools/runner_selector_time.py [--window 1.0] [--reps 5] [--out profiles/selector_ab.txt]
"""
import argparse
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

LEGS = ("torch_padded", "torch_novalid", "device_padded", "torch_exact", "device_exact")
EPS = 0.5


class TorchEpsilonGreedy:
    """The reference selector's chain of torch kernels at a fixed epsilon."""

    def __init__(self, validate):
        self.epsilon = EPS
        self.validate = validate

    def select_action(self, agent_inputs, avail_actions, t_env, test_mode=False):
        q = agent_inputs.clone()                       # the same launches, one by one
        q[avail_actions == 0] = float("-inf")
        explore = (torch.rand_like(q[..., 0]) < self.epsilon).to(torch.int64)
        uniform = torch.distributions.Categorical(probs=avail_actions.to(q.dtype),
                                                  validate_args=self.validate).sample()
        greedy = q.max(dim=2).indices
        return explore * uniform + (1 - explore) * greedy


class StubMAC:
    def __init__(self, selector):
        self.action_selector = selector

    def init_hidden(self, batch_size):
        pass

    def select_actions(self, batch, t_ep, t_env, bs, test_mode=False):
        q = batch["obs"][:, t_ep, :, :5][bs] * 0.01
        return self.action_selector.select_action(q, batch["avail_actions"][bs, t_ep], t_env, test_mode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
    ap.add_argument("--reps", type=int, default=5, help="alternations over all legs")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "selector_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("runner_selector_time needs a HIP device")
    import bench
    from mapfx import _abi
    from mapfx.episode import DeviceEpisodeBatch, OneHot
    from mapfx.maps import synthetic_instances
    from mapfx.runners import ParallelRunner
    from mapfx.selectors import DeviceEpsilonGreedySelector

    S, N, B = 8, 15, a.envs
    inst = synthetic_instances(B, S, S, N, p_obstacle=0.0, seed=1)
    tmp = tempfile.mkdtemp(prefix="mapfx_selector_")
    mp = os.path.join(tmp, "empty-8-8.map")
    with open(mp, "w") as f:
        f.write("type octile\nheight 8\nwidth 8\nmap\n" + "\n".join(["." * 8] * 8) + "\n")
    ea = dict(bench.PARTIAL_YAML, grid_file_path=mp, agents_path=os.path.join(tmp, "x-"), n_agents=N)
    limit = bench.PARTIAL_YAML["episode_limit"]
    sargs = types.SimpleNamespace(epsilon_start=EPS, epsilon_finish=EPS, epsilon_anneal_time=1, seed=0)

    def make(leg):
        rargs = types.SimpleNamespace(env="marl_partial", batch_size_run=B, device="cuda:0", env_args=ea,
                                      episode_batch_cls=DeviceEpisodeBatch, test_nepisode=B,
                                      runner_log_interval=1 << 62, seed=0,
                                      runner_exact_bs=leg.endswith("_exact"))
        r = ParallelRunner(rargs, None, instance_fn=lambda ep: (inst["init_pos"], inst["goals"]))
        info = r.get_env_info()
        scheme = {"state": {"vshape": info["state_shape"]},
                  "obs": {"vshape": info["obs_shape"], "group": "agents"},
                  "actions": {"vshape": (1,), "group": "agents", "dtype": torch.long},
                  "avail_actions": {"vshape": (info["n_actions"],), "group": "agents", "dtype": torch.int},
                  "reward": {"vshape": (1,)}, "terminated": {"vshape": (1,), "dtype": torch.uint8}}
        sel = DeviceEpsilonGreedySelector(sargs) if leg.startswith("device") else \
            TorchEpsilonGreedy(validate=None if leg != "torch_novalid" else False)
        r.setup(scheme, {"agents": N}, {"actions": ("actions_onehot", [OneHot(out_dim=5)])}, StubMAC(sel))
        return r

    runners = {}
    for leg in LEGS:                      # warm every leg: first batch, caches, code objects
        r = runners[leg] = make(leg)
        for _ in range(3):
            r.run()
        torch.cuda.synchronize()
    # the invariance the feature stands on: run 2 of the padded and of the exact device leg
    rp, re_ = runners["device_padded"], runners["device_exact"]
    for k, v in rp.batch.data.transition_data.items():
        assert torch.equal(v, re_.batch.data.transition_data[k]), k
    assert torch.equal(rp._ep_return, re_._ep_return) and rp.t_env == re_.t_env

    def timed(leg, n):
        r, steps = runners[leg], 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            r.run()
            steps += r.t
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e6

    def runs_for(leg):
        r = runners[leg]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            r.run()
        torch.cuda.synchronize()
        return max(3, int(np.ceil(a.window / ((time.perf_counter() - t0) / 3))))

    runs = {leg: runs_for(leg) for leg in LEGS}
    us = {leg: [] for leg in LEGS}
    for _ in range(a.reps):               # alternate over the legs
        for leg in LEGS:
            us[leg].append(timed(leg, runs[leg]))
    res = {leg: {"us_per_step": [round(v, 3) for v in us[leg]], "median": round(float(np.median(us[leg])), 3),
                 "min": round(min(us[leg]), 3), "max": round(max(us[leg]), 3), "runs_per_window": runs[leg],
                 "loop_iterations_per_run": runners[leg].t} for leg in LEGS}
    line = {"metric": "ParallelRunner.run() wall us per runner step: torch epsilon-greedy vs the device selector",
            "config": {"workload": "marl_partial yaml: 8x8 empty, 15 agents, window 5, K 5, %d envs, %d-step "
                                   "episodes, epsilon %.2f, Q = 0.01 * obs[..., :5]" % (B, limit, EPS)},
            "timing": "wall clock around runs filling %.2f s per window, device synchronised at both ends, "
                      "%d alternations over the legs in one session; median, min and max of the repeats"
                      % (a.window, a.reps),
            "legs": res, "build_id": _abi.build_id()}
    lines = [json.dumps(line), "| leg | median us per step | min | max | vs torch_padded (median) |", "|---|---|---|---|---|"]
    base = res["torch_padded"]["median"]
    for leg in LEGS:
        lines.append("| %s | %.2f | %.2f | %.2f | %.3f |" % (leg, res[leg]["median"], res[leg]["min"],
                                                             res[leg]["max"], res[leg]["median"] / base))
    for ta, dv in (("torch_padded", "device_padded"), ("torch_novalid", "device_padded"),
                   ("torch_exact", "device_exact")):
        lines.append("%s separated from %s (every repeat below every repeat): %s"
                     % (dv, ta, "yes" if res[dv]["max"] < res[ta]["min"] else "no"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
