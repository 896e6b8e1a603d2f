"""Plain-Python restatement of the reference ParallelRunner loop -- TEST
INFRASTRUCTURE ONLY.

MARL-curve-main/src/runners/parallel_runner.py `reset` / `run` / `_log` (:67-216) filling
components/episode_buffer.py `EpisodeBatch.update` (:100-134) with PyMARL's scheme and
the OneHot actions preprocess (components/transforms.py), over
oracle.partial_oracle.PartialEnvState envs in place of the forked workers.  Restated:
the stale `envs_not_terminated` list (the MAC's `bs` and the actions rows of step t
cover the envs running before step t - 1, :106-124), the three `update` calls per step
with their bs / ts / mark_filled (:113, :167, :173), update's casts to the scheme's
dtypes (float32 obs / state / reward, int32 avail_actions, int64 actions, uint8
terminated, int64 filled), returns / lengths / env_steps_this_run / t_env and the
logged stats (:175-216; MARL_PARTIAL's info holds `_step_count` only and no
"episode_limit" key, so env_terminated = terminated, :156).
Pinned by tests/golden/runner_*.npz (written by the reference runner itself,
tests/golden/gen_runner_fixtures.py) in tests/test_runner_ref.py.
"""
from __future__ import annotations

import numpy as np

from oracle.partial_oracle import PartialEnvState, bfs_goal_dist

DTYPES = {"state": np.float32, "obs": np.float32, "actions": np.int64,
          "avail_actions": np.int32, "reward": np.float32, "terminated": np.uint8,
          "actions_onehot": np.float32, "filled": np.int64}


def field_shapes(n_agents, obs_dim):
    """The per-step shape of every transition field, in EpisodeBatch's order."""
    return {"state": (3,), "obs": (n_agents, obs_dim), "actions": (n_agents, 1),
            "avail_actions": (n_agents, 5), "reward": (1,), "terminated": (1,),
            "actions_onehot": (n_agents, 5), "filled": (1,)}


def new_batch(B, T, n_agents, obs_dim, fill=0):
    """{field: [B, T, *shape]} with every BYTE set to `fill` (0: EpisodeBatch's zeros)."""
    out = {}
    for k, shape in field_shapes(n_agents, obs_dim).items():
        a = np.empty((B, T) + shape, dtype=DTYPES[k])
        a.view(np.uint8)[...] = fill
        out[k] = a
    return out


def parse_map(rows):
    """Map rows ('.' free, '@' obstacle) -> the oracle's grid (0 free, -1 obstacle)."""
    return np.array([[0 if ch == "." else -1 for ch in str(r)] for r in rows], dtype=np.int64)


def make_envs(grid, starts, goals, **env_kw):
    """One PartialEnvState per row of starts / goals [B, N, 2]; the goal-distance tables
    (one BFS per distinct goal cell) are shared among the envs."""
    cache = {}
    envs = []
    for st, gl in zip(starts, goals):
        gd = []
        for g in gl:
            key = (int(g[0]), int(g[1]))
            if key not in cache:
                cache[key] = bfs_goal_dist(grid, key)
            gd.append(cache[key])
        envs.append(PartialEnvState(grid, st, gl, goal_dist=gd, **env_kw))
    return envs


def update(batch, data, bs, ts, mark_filled):
    """EpisodeBatch.update (:100-134) on a dict of numpy arrays; bs a list (or None for
    every env), ts one time index."""
    B = batch["filled"].shape[0]
    bs = np.arange(B) if bs is None else np.asarray(bs, dtype=np.int64)
    for k, v in data.items():
        if mark_filled:
            batch["filled"][bs, ts] = 1
            mark_filled = False
        v = np.asarray(v).astype(DTYPES[k])                    # th.tensor(v, dtype=scheme's)
        batch[k][bs, ts] = v.reshape(batch[k][bs, ts].shape)   # view_as
        if k == "actions":                                     # preprocess: OneHot(out_dim=5)
            a = batch[k][bs, ts]
            oh = np.zeros(a.shape[:-1] + (5,), dtype=np.float32)
            np.put_along_axis(oh, a, 1.0, axis=-1)
            batch["actions_onehot"][bs, ts] = oh


class RefRunner:
    """The reference runner's state across runs: t_env, the train stats / returns and
    every (key, value, t_env) handed to the logger."""

    def __init__(self, runner_log_interval=1):
        self.runner_log_interval = runner_log_interval
        self.t_env = 0
        self.train_returns = []
        self.train_stats = {}
        self.log_train_stats_t = -100000
        self.log = []

    def run(self, envs, batch, mac):
        """One training run() (:91-206) over `envs` into `batch` (an initial batch from
        new_batch, modified in place).  mac(batch, t_ep, bs) -> actions [len(bs), N].
        Returns (batch, calls, returns, lengths), calls = [(t_ep, tuple(bs)), ...]."""
        B = len(envs)
        for e in envs:                                                       # reset (:67-89)
            e.reset()
        update(batch, {"state": [e.state() for e in envs],
                       "avail_actions": [e.avail() for e in envs],
                       "obs": [e.obs() for e in envs]}, None, 0, True)
        t = 0
        env_steps_this_run = 0
        episode_returns = [0 for _ in range(B)]
        episode_lengths = [0 for _ in range(B)]
        terminated = [False for _ in range(B)]
        envs_not_terminated = [b for b, termed in enumerate(terminated) if not termed]
        final_env_infos = []
        calls = []
        while True:
            calls.append((t, tuple(envs_not_terminated)))
            actions = np.asarray(mac(batch, t, list(envs_not_terminated)))
            actions = actions.reshape(len(envs_not_terminated), -1)
            update(batch, {"actions": actions[:, None]}, envs_not_terminated, t, False)
            action_idx = 0
            data = {}
            for idx in range(B):
                if idx in envs_not_terminated:       # the stale list (:118)
                    if not terminated[idx]:
                        reward, term = envs[idx].step(actions[action_idx])
                        data[idx] = (reward, term, envs[idx].state(), envs[idx].avail(),
                                     envs[idx].obs(), {"_step_count": envs[idx].t} if term else {})
                    action_idx += 1
            envs_not_terminated = [b for b, termed in enumerate(terminated) if not termed]
            if all(terminated):
                break
            post = {"reward": [], "terminated": []}
            pre = {"state": [], "avail_actions": [], "obs": []}
            for idx in range(B):
                if not terminated[idx]:
                    reward, term, state, avail, obs, info = data[idx]
                    post["reward"].append((reward,))
                    episode_returns[idx] += reward
                    episode_lengths[idx] += 1
                    env_steps_this_run += 1
                    if term:
                        final_env_infos.append(info)
                    terminated[idx] = term
                    post["terminated"].append((term,))
                    pre["state"].append(state)
                    pre["avail_actions"].append(avail)
                    pre["obs"].append(obs)
            update(batch, post, envs_not_terminated, t, False)
            t += 1
            update(batch, pre, envs_not_terminated, t, True)
        self.finish(episode_returns, episode_lengths, env_steps_this_run, final_env_infos)
        return batch, calls, episode_returns, episode_lengths

    def finish(self, episode_returns, episode_lengths, env_steps_this_run, final_env_infos):
        """The end of run() (:175-204): t_env, the stats and the log."""
        B = len(episode_returns)
        self.t_env += env_steps_this_run
        cur_stats, cur_returns = self.train_stats, self.train_returns
        infos = [cur_stats] + final_env_infos
        keys = []
        for d in infos:
            keys += [k for k in d if k not in keys]
        cur_stats.update({k: sum(d.get(k, 0) for d in infos) for k in keys})
        cur_stats["n_episodes"] = B + cur_stats.get("n_episodes", 0)
        cur_stats["ep_length"] = sum(episode_lengths) + cur_stats.get("ep_length", 0)
        cur_returns.extend(episode_returns)
        if self.t_env - self.log_train_stats_t >= self.runner_log_interval:
            self._log(cur_returns, cur_stats)
            self.log_train_stats_t = self.t_env

    def _log(self, returns, stats):   # :208-216
        self.log.append(("return_mean", float(np.mean(returns)), self.t_env))
        self.log.append(("return_std", float(np.std(returns)), self.t_env))
        returns.clear()
        for k, v in stats.items():
            if k != "n_episodes":
                self.log.append((k + "_mean", float(v / stats["n_episodes"]), self.t_env))
        stats.clear()
