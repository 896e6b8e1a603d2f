"""GPU test of the batched ParallelRunner's opt-in output mode (args.runner_device_repair with
env_args["output"]): every EpisodeBatch tensor of a run equals the reference ParallelRunner's
bookkeeping (tests/runner_ref.py) over envs that are MarlPartialBatch(output=True) instances
of one env each -- a loop of step() calls -- and with the option off the run equals today's,
which drops `output`."""
import types

import numpy as np
import pytest
import torch

import runner_ref
from test_gpu_runner import Logger, scripted_action

pytestmark = pytest.mark.gpu

B, S, N, LIMIT, SEED = 6, 6, 4, 12, 77
REWARDS = dict(move_reward=-0.01, stay_reward=-0.02, stay_goal_reward=0, node_collide_reward=-1,
               edge_collide_reward=-1, env_collide_reward=-1, complete_reward=1000, complete_fac=1.5,
               gamma=0.99)
MAP = ["......", "..@...", "......", "...@..", "......", "......"]


def _instances(ep):
    rs = np.random.RandomState(100 + ep)
    grid = runner_ref.parse_map(MAP)
    free = np.argwhere(grid == 0)
    near = free[(free[:, 0] < 3) & (free[:, 1] < 3)]     # starts close together: collisions
    st = np.stack([near[rs.permutation(len(near))[:N]] for _ in range(B)]).astype(np.int32)
    gl = np.stack([free[rs.permutation(len(free))[:N]] for _ in range(B)]).astype(np.int32)
    return st, gl


class ScriptedMAC:
    action_selector = types.SimpleNamespace()

    def init_hidden(self, batch_size):
        pass

    def select_actions(self, batch, t_ep, t_env, bs=slice(None), test_mode=False):
        av = batch["avail_actions"][:, t_ep].cpu().numpy()
        idx = bs.tolist()
        out = [[scripted_action(b, t_ep, k, av[b, k]) for k in range(N)] for b in idx]
        return torch.tensor(out, dtype=torch.long, device="cuda").view(len(idx), N)


def _runner(tmp_path, **extra):
    from mapfx.episode import DeviceEpisodeBatch, OneHot
    from mapfx.runners import ParallelRunner
    mp = tmp_path / "m.map"
    mp.write_text("type octile\nheight %d\nwidth %d\nmap\n%s\n" % (S, S, "\n".join(MAP)))
    env_args = dict(REWARDS, grid_file_path=str(mp), agents_path=str(tmp_path / "x-"), n_agents=N,
                    obs_window=5, obs_knn_agents=5, episode_limit=LIMIT)
    env_args.update(extra.pop("env_extra", {}))
    args = types.SimpleNamespace(env="marl_partial", batch_size_run=B, device="cuda", seed=SEED,
                                 env_args=env_args, episode_batch_cls=DeviceEpisodeBatch, test_nepisode=B,
                                 runner_log_interval=1, **extra)
    runner = ParallelRunner(args, Logger(), instance_fn=_instances)
    info = runner.get_env_info()
    scheme = {"state": {"vshape": info["state_shape"]},
              "obs": {"vshape": info["obs_shape"], "group": "agents"},
              "actions": {"vshape": (1,), "group": "agents", "dtype": torch.long},
              "avail_actions": {"vshape": (info["n_actions"],), "group": "agents", "dtype": torch.int},
              "reward": {"vshape": (1,)}, "terminated": {"vshape": (1,), "dtype": torch.uint8}}
    runner.setup(scheme, {"agents": N}, {"actions": ("actions_onehot", [OneHot(out_dim=5)])}, ScriptedMAC())
    return runner


class OutputEnv:
    """One env of the reference loop: a MarlPartialBatch(output=True) of E = 1 with the
    runner's global env id, stepped by step()."""

    def __init__(self, b, start, goal, seed):
        from mapfx.partial import MarlPartialBatch
        grid = (runner_ref.parse_map(MAP) != 0).astype(np.uint8)[None]
        self.b = MarlPartialBatch(start[None], goal[None], grids=grid, env_offset=b, output=True,
                                  repair_seed=seed, obs_window=5, obs_knn_agents=5, episode_limit=LIMIT,
                                  **REWARDS)
        self.repaired = 0

    @property
    def t(self):
        return int(self.b.t.cpu()[0])

    def reset(self):
        self.b.reset()

    def step(self, actions):
        out = self.b.step(torch.as_tensor(np.asarray(actions, dtype=np.int8)[None]).cuda())
        self.repaired += int(self.b.repair_flags.cpu()[0] != 0)
        return float(out["reward"].cpu()[0]), bool(self.b.terminated.cpu()[0])

    def state(self):
        return self.b.out["state"].cpu().numpy()[0]

    def avail(self):
        return self.b.avail_actions().cpu().numpy()[0]

    def obs(self):
        return self.b.out["obs"].cpu().numpy()[0]


def _ref_mac(batch, t, bs):
    return [[scripted_action(b, t, k, batch["avail_actions"][b, t, k]) for k in range(N)] for b in bs]


def test_runner_device_repair_equals_step_loop(tmp_path):
    from mapfx import rng
    runner = _runner(tmp_path, runner_device_repair=True, env_extra=dict(output=True))
    ref = runner_ref.RefRunner()
    repaired = 0
    for run in range(2):
        batch = runner.run(test_mode=False)
        st, gl = _instances(run)
        envs = [OutputEnv(b, st[b], gl[b], rng.runner_repair_seed(SEED, run)) for b in range(B)]
        want = runner_ref.new_batch(B, LIMIT + 1, N, runner.env.obs_dim)
        ref.run(envs, want, _ref_mac)
        repaired += sum(e.repaired for e in envs)
        for k, v in batch.data.transition_data.items():
            got = v.cpu().numpy()
            assert got.shape == want[k].shape and got.dtype == want[k].dtype, (run, k)
            assert np.array_equal(got.view(np.uint8), want[k].view(np.uint8)), (run, k)
        assert runner.t_env == ref.t_env
    assert repaired >= 3      # the runs exercise the repair
    with pytest.raises(ValueError):
        runner.collect(eps=0.0)


def test_option_off_equals_today(tmp_path):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    plain = _runner(tmp_path / "a")
    dropped = _runner(tmp_path / "b", env_extra=dict(output=True))     # `output` silently dropped
    only_flag = _runner(tmp_path, runner_device_repair=True)           # no `output`: nothing changes
    for r in (dropped, only_flag):
        assert not r._device_repair
    for run in range(2):
        base = plain.run(test_mode=False).data.transition_data
        for r in (dropped, only_flag):
            got = r.run(test_mode=False).data.transition_data
            for k, v in base.items():
                assert torch.equal(v, got[k]), (run, k)
            assert r.t_env == plain.t_env
