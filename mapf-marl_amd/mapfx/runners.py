"""Batched, device-resident ParallelRunner.

Same public surface as MARL-curve-main/src/runners/parallel_runner.py
(`ParallelRunner.__init__(args, logger)`, `setup(scheme, groups, preprocess, mac)`,
`get_env_info`, `reset`, `run(test_mode)`, `close_env`, `save_replay`, the
`t_env` counter and the return / stat logging), but the `batch_size_run` envs are
one MarlPartialBatch on the GPU instead of one subprocess + Pipe each, and a
runner step is: the MAC's select_actions, then three device launches
(include/mapfx_runner.h) -- actions rows, the env step, the step's rows straight
into the EpisodeBatch tensors with the runner's bookkeeping (running envs, the
MAC's `bs`, returns, lengths, env steps) kept on the device.  No per-step host
synchronisation: the loop-exit test reads the count of running envs from a pinned
ring, written by the step two launches back (the reference stops one MAC call after
the last env terminated; the one call the lag adds with the fused step finds no
running env and records nothing, and `args.runner_exact_bs` makes exactly the
reference's calls; see `run`).

The EpisodeBatch is whatever `setup` is given (PyMARL passes
components.episode_buffer.EpisodeBatch); the runner writes its
`data.transition_data` tensors (PyMARL's scheme: obs / state float32,
avail_actions int32, actions int64 (+ actions_onehot float32 from the OneHot
preprocess), reward float32, terminated uint8, filled int64) on the batch's device.

Row semantics are the reference's (tests/golden/runner_*.npz were produced by the
reference ParallelRunner itself), including its stale list: the MAC's `bs` and the
actions row at step t cover the envs that were running before step t - 1.  The
MAC gets `bs` as a device LongTensor of length B (ascending running env ids,
padded with the first one), a form the reference EpisodeBatch / BasicMAC index
with (episode_buffer.py:186-190); `args.runner_exact_bs` passes the exact-length
list instead (one host sync per step, for stochastic torch action selectors whose RNG
consumption must follow the reference's; mapfx.selectors' device selectors key their random
words by env and step -- `run` binds them -- and pick the same actions from either form).

`args.runner_device_repair = True` with `env_args["output"]` (default: `output` is dropped)
turns on output mode: every step of `run()` is followed by the device collision repair
(mapfx_partial_repair, seed rng.runner_repair_seed(args.seed, run)) and the rows at ts + 1
are rewritten from the repaired state (mapfx_runner_reobserve); `collect()` then raises.

`collect()` is a run with no MAC at all: the whole episode loop as one launch
(mapfx_runner_rollout), the actions from the on-device policy or a given table, the
batch, t_env and the stats as `run()` leaves them.

Per-env instances: every reset draws each env's scenario like
MARL_PARTIAL_ENV.__setup_agent (:896-920: random.randint(1, 25) then
random.sample of the scen lines), from a per-env `random.Random(seed + e)` stream
(the reference's forked workers all share one stream and draw identical instances).
`instance_fn(episode) -> (starts [B, N, 2], goals [B, N, 2])` overrides the draw.
`args.runner_device_draw = True` draws on the device instead (MarlPartialBatch.redraw:
the same distribution from the library's counter-based streams, keyed by args.seed, the
env id and the run number; run r plays the instances rng.scen_draw(seed, ids, r, ...)
names), with no host loop and no copy of instances per reset.
"""
from __future__ import annotations

import ctypes
import random
from functools import partial

import numpy as np
import torch

from . import _abi
from ._abi import check, lib, ptr
from ._base import DTYPES as _ADT    # noqa: F401  (tools/runner_host_probe.py replays `run` with it)
from ._base import as_actions
from .maps import draw_scen, load_map, load_scen_table, read_scen
from .partial import MarlPartialBatch
from .rng import runner_policy_seed, runner_repair_seed

_ROW_DTYPES = {"obs": torch.float32, "state": torch.float32, "avail_actions": torch.int32,
               "actions": torch.int64, "actions_onehot": torch.float32, "reward": torch.float32,
               "terminated": torch.uint8, "filled": torch.int64}
_ROW_FIELDS = {"obs": "obs", "state": "state", "avail_actions": "avail", "actions": "actions",
               "actions_onehot": "onehot", "reward": "reward", "terminated": "terminated",
               "filled": "filled"}
_RING = 4


_SCEN_CACHE = {}


def _scen_lines(path):
    lines = _SCEN_CACHE.get(path)
    if lines is None:
        lines = _SCEN_CACHE[path] = read_scen(path)
    return lines


def _scen_draw(rng, agents_path, n):
    """:896-920 with an explicit Random: (starts, goals) as (row, col)."""
    rows = draw_scen(rng, agents_path, n, read=_scen_lines)
    return [(sy, sx) for sx, sy, _, _ in rows], [(gy, gx) for _, _, gx, gy in rows]


class ParallelRunner:
    """runners/parallel_runner.py:9-226 over one batched GPU env."""

    def __init__(self, args, logger, instance_fn=None):
        self.args = args
        self.logger = logger
        self.batch_size = int(args.batch_size_run)
        if args.env != "marl_partial":
            raise ValueError("the batched runner drives the marl_partial env (got %r)" % args.env)
        ea = dict(args.env_args)
        self.n_agents = int(ea.pop("n_agents", 4))
        grid_path, self.agents_path = ea.pop("grid_file_path"), ea.pop("agents_path")
        # args.runner_device_repair (default False: `output` is dropped, as ever): with
        # env_args["output"] every step of run() is followed by the device collision repair
        # (mapfx_partial_repair) and the rows at ts + 1 are written again from the repaired
        # state (mapfx_runner_reobserve)
        self._device_repair = bool(getattr(args, "runner_device_repair", False)) and bool(ea.get("output"))
        for k in ("seed", "render", "debug", "visual", "output"):
            ea.pop(k, None)
        dev = torch.device(getattr(args, "device", "cuda"))
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.grid = load_map(grid_path)
        seed = int(getattr(args, "seed", 0) or 0)
        self._rngs = [random.Random(seed + e) for e in range(self.batch_size)]
        self._instance_fn = instance_fn
        self._episode = 0
        # args.runner_device_draw (default False: the host draw above): every reset draws
        # the envs' scenarios on the device (see the module docstring)
        self._device_draw = bool(getattr(args, "runner_device_draw", False))
        if self._device_draw:
            if instance_fn is not None:
                raise ValueError("runner_device_draw draws the instances itself: it cannot be "
                                 "combined with instance_fn")
            H, W = self.grid.shape
            lines, n_lines = load_scen_table(self.agents_path, H, W)
            # placeholder instance from the table's first lines: it consumes no episode
            # (every env is re-drawn, tables included, by the first reset's redraw)
            k = int(np.argmax(n_lines > 0))
            rows = lines[k, np.arange(self.n_agents) % max(int(n_lines[k]), 1)].astype(np.int32)
            starts = np.repeat(rows[None, :, :2], self.batch_size, axis=0)
            goals = np.repeat(rows[None, :, 2:], self.batch_size, axis=0)
        else:
            starts, goals = self._draw()
        self.env = MarlPartialBatch(starts, goals, grids=self.grid[None], device=self.device, **ea)
        self._loaded = (starts.tobytes(), goals.tobytes())
        # collect(): mapfx_runner_rollout takes no mapfx_partial_out, its invalid-action
        # report goes to the env's err word like the step's
        check(lib.mapfx_partial_bind_err(self.env._h, ptr(self.env.err)), "mapfx_partial_bind_err")
        if self._device_draw:
            self.env.set_scenarios(lines, n_lines, seed=seed)
        self.env_info = {"state_shape": 3, "obs_shape": self.env.obs_dim, "n_actions": 5,
                         "n_agents": self.n_agents, "episode_limit": self.env.episode_limit}
        self.episode_limit = self.env_info["episode_limit"]
        B, N, dev, z = self.batch_size, self.n_agents, self.device, self.env._zeros
        self._alive, self._alive_prev = z((B,), torch.uint8), z((B,), torch.uint8)
        self._bs = z((B,), torch.int64)
        self._counts = z((2,), torch.int32)
        self._ep_return, self._ep_length = z((B,), torch.float64), z((B,), torch.int64)
        self._env_steps = z((1,), torch.int64)
        self._env_actions = torch.full((B, N), 4, dtype=torch.int8, device=dev)
        # row of env b in bs (-1: not in it): the fused step reads b's actions there;
        # two halves by step parity (the compaction inside step k writes step k + 1's)
        self._bs_inv = torch.full((2, B), -1, dtype=torch.int32, device=dev)
        self._rs = _abi.RState(B=B, N=N, D=self.env.obs_dim, alive=ptr(self._alive),
                               alive_prev=ptr(self._alive_prev), bs=ptr(self._bs),
                               counts=ptr(self._counts), ep_return=ptr(self._ep_return),
                               ep_length=ptr(self._ep_length), env_steps=ptr(self._env_steps),
                               env_actions=ptr(self._env_actions), bs_inv=ptr(self._bs_inv))
        # counts {len(bs), running} of step k land in slot k % _RING of a mapped host
        # buffer, written by the compaction kernel itself (no copy launch); the slot's
        # event marks them final
        hp, dp = ctypes.c_void_p(), ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.mapfx_host_ring_alloc(2 * _RING, ctypes.byref(hp), ctypes.byref(dp)),
                  "mapfx_host_ring_alloc")
        self._ring_host = hp
        host = np.ctypeslib.as_array(ctypes.cast(hp, ctypes.POINTER(ctypes.c_int32)),
                                     shape=(_RING, 2))
        self._ring = [(torch.cuda.Event(), host[i], dp.value + 8 * i) for i in range(_RING)]
        if self._device_repair:
            if not lib.mapfx_partial_repair_offered(self.env._h):
                raise ValueError("runner_device_repair needs n_agents <= 64 and map sides <= 256")
            # the step's separate-kernel form (no bs_inv): its actions pass leaves every env's
            # actions in env_actions, which the repair then reads as the step did
            self._rs_repair = _abi.RState(B=B, N=N, D=self.env.obs_dim, alive=ptr(self._alive),
                                          alive_prev=ptr(self._alive_prev), bs=ptr(self._bs),
                                          counts=ptr(self._counts), ep_return=ptr(self._ep_return),
                                          ep_length=ptr(self._ep_length), env_steps=ptr(self._env_steps),
                                          env_actions=ptr(self._env_actions), bs_inv=None)
            self._old_pos = z((B, N, 2), torch.int32)
            self.repair_flags = z((B,), torch.uint8)
            self.repair_rounds_used = z((B, 2), torch.int32)
            self._repair = _abi.PRepair(seed=0, old_pos=ptr(self._old_pos), actions=ptr(self._env_actions),
                                        action_dtype=_abi.MAPFX_I8,
                                        max_rounds=int(getattr(args, "runner_repair_rounds", 16)),
                                        flags=ptr(self.repair_flags), rounds=ptr(self.repair_rounds_used))
        self.t = 0
        self.t_env = 0
        self.train_returns = []
        self.test_returns = []
        self.train_stats = {}
        self.test_stats = {}
        self.log_train_stats_t = -100000

    def _draw(self):
        if self._instance_fn is not None:
            st, gl = self._instance_fn(self._episode)
        else:
            st, gl = [], []
            for e in range(self.batch_size):
                s, g = _scen_draw(self._rngs[e], self.agents_path, self.n_agents)
                st.append(s)
                gl.append(g)
        return np.asarray(st, dtype=np.int32), np.asarray(gl, dtype=np.int32)

    def setup(self, scheme, groups, preprocess, mac):
        device = getattr(self.args, "device", "cuda")
        self.new_batch = partial(self._batch_cls(), scheme, groups, self.batch_size,
                                 self.episode_limit + 1, preprocess=preprocess, device=device)
        self.mac = mac
        self.scheme = scheme
        self.groups = groups
        self.preprocess = preprocess

    def _batch_cls(self):
        cls = getattr(self.args, "episode_batch_cls", None)
        if cls is None:
            from components.episode_buffer import EpisodeBatch  # PyMARL's, when run inside it
            cls = EpisodeBatch
        return cls

    def __del__(self):
        hp = getattr(self, "_ring_host", None)
        if hp is not None and hp.value:
            lib.mapfx_host_ring_free(hp)
            self._ring_host = None

    def get_env_info(self):
        return self.env_info

    def save_replay(self):
        pass

    def close_env(self):
        pass

    # ------------------------------------------------------------------ rows
    def _rows(self, batch):
        """mapfx_episode_rows over the batch's transition tensors (checked)."""
        td = batch.data.transition_data
        r = _abi.ERows(max_t=int(batch.max_seq_length))
        B, N, D = self.batch_size, self.n_agents, self.env.obs_dim
        shapes = {"obs": (N, D), "state": (3,), "avail_actions": (N, 5), "actions": (N, 1),
                  "actions_onehot": (N, 5), "reward": (1,), "terminated": (1,), "filled": (1,)}
        for key, field in _ROW_FIELDS.items():
            t = td.get(key)
            if t is None:
                if key != "actions_onehot":
                    raise KeyError("EpisodeBatch has no %r field" % key)
                continue
            if t.dtype != _ROW_DTYPES[key] or tuple(t.shape[2:]) != shapes[key] or \
                    t.shape[0] != B or t.device != self.device:
                raise ValueError("EpisodeBatch %r is %s %s on %s; the runner writes %s %s on %s"
                                 % (key, t.dtype, tuple(t.shape), t.device, _ROW_DTYPES[key],
                                    (B, r.max_t) + shapes[key], self.device))
            inner = 1
            for s in shapes[key]:
                inner *= s
            if t.stride(-1) != 1 or t.stride(1) < inner or (len(shapes[key]) > 1 and
                                                             t.stride(2) != shapes[key][1]):
                raise ValueError("EpisodeBatch %r rows are not contiguous" % key)
            setattr(r, field, ptr(t))
            setattr(r, field + "_sb", t.stride(0))
            setattr(r, field + "_st", t.stride(1))
        if "actions_onehot" in td:
            pre = (self.preprocess or {}).get("actions")
            tf = pre[1] if pre else []
            if not (pre and pre[0] == "actions_onehot" and len(tf) == 1
                    and type(tf[0]).__name__ == "OneHot" and getattr(tf[0], "out_dim", 5) == 5):
                raise ValueError("actions_onehot must come from the OneHot(out_dim=5) preprocess")
        return r

    def _call(self, fn, *args):
        return fn(*args, torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ loop
    def reset(self):
        """:62-76: new batch, every env reset (instances re-drawn, :130), row 0."""
        self.batch = self.new_batch()
        if self._device_draw:
            self.env.redraw()             # run r draws with the envs' episode counters == r
        else:
            starts, goals = self._draw()
            key = (starts.tobytes(), goals.tobytes())
            if key != self._loaded:       # same instances: the BFS tables still hold
                self.env.set_agents(starts, goals)
                self._loaded = key
        self._episode += 1
        self.env.reset()
        self._erows = self._rows(self.batch)
        check(self._call(lib.mapfx_runner_begin, ctypes.byref(self._rs),
                         ctypes.byref(self.env._obs_out), ctypes.byref(self._erows)),
              "mapfx_runner_begin")
        self.t = 0
        self.env_steps_this_run = 0

    def run(self, test_mode=False):
        """:78-206 with the envs stepped as one batch on the device.

        Iteration k of the reference calls the MAC (bs = envs running before step
        k - 1), writes the actions rows, then stops if no env is running after step
        k - 1, else steps and writes the step's rows.  Here iteration k first stops
        if the ring slot of launch k - 2 says no env is running: with the post pass
        and the next MAC call's compaction fused into the env step (one launch per
        step, mapfx_runner_step) that slot counts the envs running after step k - 3,
        else (the separate post / compaction kernels) after step k - 2 -- two
        iterations old either way, so no wait in the steady state.  The iterations
        the lag adds past the reference's last MAC call (one with the fused step, none
        with the separate kernels) find no running env (a `bs` that is all padding, no
        action rows, nothing stepped) and write nothing; the loop also ends when the
        batch has no row k (every env has met its episode limit by then).  With
        args.runner_exact_bs the loop waits for the count of step k - 1's compaction
        anyway (len(bs) of MAC call k) and stops when it is 0, so the MAC is called
        exactly as often as by the reference, with the reference's `bs`."""
        self.reset()
        self.mac.init_hidden(batch_size=self.batch_size)
        r, rs, env = self._erows, ctypes.byref(self._rs), self.env
        stream = torch.cuda.current_stream(self.device)
        sh = stream.cuda_stream
        repair = self._device_repair
        if repair:
            rs = ctypes.byref(self._rs_repair)
            base = int(getattr(self.args, "seed", 0) or 0)
            self._repair.seed = runner_repair_seed(base, self._episode - 1)
            rep_args = (env._h, ctypes.byref(env._state), ctypes.byref(self._repair),
                        ctypes.byref(env._obs_out), sh)
        fixed = (env._h, ctypes.byref(env._state), ctypes.byref(env._out), rs)
        step = lib.mapfx_runner_step
        # The MAC gets `bs` padded to B (no host sync per step); a stochastic selector
        # then draws random numbers for B rows, not len(bs) as the reference does
        # (parallel_runner.py:106), so its RNG stream diverges once an env has
        # terminated.  args.runner_exact_bs = True passes bs[:len(bs)] instead, at the
        # cost of one host sync per step (the count of the previous step's compaction).
        exact_bs = bool(getattr(self.args, "runner_exact_bs", False))
        # A selector with `bind` (mapfx.selectors) keys its random words by (run, env id,
        # step): it picks the same actions from the padded and from the exact `bs`.
        bind = getattr(getattr(self.mac, "action_selector", None), "bind", None)
        k = 0
        max_t = int(r.max_t)
        while k < max_t:
            if k >= 2:   # none running (after step k - 3 fused, k - 2 unfused): stop
                ev, hc, _ = self._ring[(k - 2) % _RING]
                ev.synchronize()
                if int(hc[1]) == 0:
                    break
            bs = self._bs
            if exact_bs and k >= 1:   # len(bs) from step k - 1's compaction (one sync)
                ev, hc, _ = self._ring[(k - 1) % _RING]
                ev.synchronize()
                if int(hc[0]) == 0:   # no env was running before step k - 1: the
                    break             # reference stopped after MAC call k - 1
                bs = self._bs[:int(hc[0])]
            if bind is not None:
                bind(env_ids=bs, t_ep=k, run=self._episode - 1, env_offset=env.env_offset)
            actions = self.mac.select_actions(self.batch, t_ep=k, t_env=self.t_env, bs=bs,
                                              test_mode=test_mode)
            # row j is env bs[j] (j < len(bs) read)
            a, adt = as_actions(actions.reshape(-1, self.n_agents), self.device)
            ev, _, dslot = self._ring[k % _RING]
            if repair:
                self._old_pos.copy_(env.pos)
            rc = step(*fixed, a.data_ptr(), adt, a.stride(0), k, dslot, ctypes.byref(r), sh)
            if rc:
                check(rc, "mapfx_runner_step")
            if repair:
                check(lib.mapfx_partial_repair(*rep_args), "mapfx_partial_repair")
                check(lib.mapfx_runner_reobserve(rs, ctypes.byref(env._obs_out), k, ctypes.byref(r), sh),
                      "mapfx_runner_reobserve")
            ev.record(stream)
            k += 1
        self.t = k
        return self._finish(test_mode)

    def collect(self, eps=0.0, seed=None, actions=None, test_mode=False, chunk=None, policy="descent"):
        """One run with no MAC: the episode loop as one launch (mapfx_runner_rollout), the
        actions from the on-device policy -- each agent descends its shortest path, a
        fraction `eps` of the moves uniform random (eps_q = round(eps * 2**32): eps=1.0 is
        PyMARL's initial epsilon, eps=0.0 the shortest-path baseline; rng.partial_policy_actions
        restates it, keyed by rng.runner_policy_seed(seed, run number), seed=None: args.seed)
        ; policy="pibt": the collision-free rule rng.partial_policy_pibt_actions instead of
        the descent, same eps and keys, ValueError where it is not offered --
        or from `actions`, a [max_t, B, N] int8 / int32 / int64 device tensor indexed by
        env.  The EpisodeBatch, t_env, the returns and the logged stats are those of `run()`
        with a MAC that returns the same actions.  chunk: steps per call (None: all max_t
        in one; a tuple: the successive call lengths).  Nothing is read on the host before
        the run's totals.  ValueError where the fused call is not offered (N > 64 or a side
        > 256; the policy also needs H * W <= 32767): use run() with a MAC there."""
        env = self.env
        if self._device_repair:
            raise ValueError("collect: the one-launch episode loop has no collision repair; with "
                             "runner_device_repair and output use run()")
        env.set_policy_rule(policy)
        policy = actions is None
        if not lib.mapfx_runner_rollout_offered(env._h, 1 if policy else 0):
            raise ValueError(
                "collect: the one-launch episode loop runs on the wave kernel only (n_agents <= 64 "
                "and map sides <= 256%s); this runner has n_agents = %d on a %d x %d map"
                % ("; the on-device policy also needs H * W <= 32767" if policy else "",
                   self.n_agents, self.grid.shape[0], self.grid.shape[1]))
        self.reset()
        r, max_t = self._erows, int(self._erows.max_t)
        if policy:
            if not 0.0 <= float(eps) <= 1.0:
                raise ValueError("eps must be in 0..1")
            base = int(getattr(self.args, "seed", 0) or 0) if seed is None else int(seed)
            pol = _abi.PPolicy(seed=runner_policy_seed(base, self._episode - 1),
                               eps_q=int(round(float(eps) * 2 ** 32)), t0=0)
            a, adt, polp = None, 0, ctypes.byref(pol)
        else:
            a, adt = as_actions(actions, self.device, (max_t, self.batch_size, self.n_agents))
            polp = None
        if chunk is None:
            chunks = [max_t]
        elif isinstance(chunk, (tuple, list)):
            chunks = [int(c) for c in chunk]
        else:
            chunks = [min(int(chunk), max_t - t) for t in range(0, max_t, int(chunk))]
        if any(c < 1 for c in chunks) or sum(chunks) != max_t:
            raise ValueError("chunk: the call lengths must be >= 1 and add up to max_t = %d" % max_t)
        sh = torch.cuda.current_stream(self.device).cuda_stream
        esz = a.element_size() * self.batch_size * self.n_agents if a is not None else 0
        ts = 0
        for c in chunks:
            rc = lib.mapfx_runner_rollout(env._h, ctypes.byref(env._state), ctypes.byref(self._rs),
                                          ts, c, a.data_ptr() + ts * esz if a is not None else None,
                                          adt, polp, None, ctypes.byref(r), sh)
            if rc:
                check(rc, "mapfx_runner_rollout")
            ts += c
        self.t = ts
        return self._finish(test_mode)

    def _finish(self, test_mode):
        """The end of a run (:175-204): t_env, returns, stats and the log, from the
        device's totals -- one transfer."""
        env = self.env
        env_steps = int(self._env_steps.item())
        # an env given an action outside 0..4 was not stepped (its rows say reward 0):
        # the reference asserts at marl_partial.py:177
        env.check_err()
        returns = self._ep_return.cpu().tolist()
        lengths = self._ep_length.cpu()
        self.env_steps_this_run = 0 if test_mode else env_steps
        if not test_mode:
            self.t_env += env_steps
        cur_stats = self.test_stats if test_mode else self.train_stats
        cur_returns = self.test_returns if test_mode else self.train_returns
        log_prefix = "test_" if test_mode else ""
        # infos of terminated envs carry `_step_count` (marl_partial.py:310) and every env
        # has terminated when the loop ends: their sum is the sum of the episode lengths
        total_len = int(lengths.sum())
        cur_stats["_step_count"] = total_len + cur_stats.get("_step_count", 0)
        cur_stats["n_episodes"] = self.batch_size + cur_stats.get("n_episodes", 0)
        cur_stats["ep_length"] = total_len + cur_stats.get("ep_length", 0)
        cur_returns.extend(returns)
        n_test_runs = max(1, getattr(self.args, "test_nepisode", self.batch_size)
                          // self.batch_size) * self.batch_size
        if test_mode and (len(self.test_returns) == n_test_runs):
            self._log(cur_returns, cur_stats, log_prefix)
        elif self.t_env - self.log_train_stats_t >= getattr(self.args, "runner_log_interval",
                                                            1 << 62):
            self._log(cur_returns, cur_stats, log_prefix)
            sel = getattr(self.mac, "action_selector", None)
            if self.logger is not None and hasattr(sel, "epsilon"):
                self.logger.log_stat("epsilon", sel.epsilon, self.t_env)
            self.log_train_stats_t = self.t_env
        return self.batch

    def _log(self, returns, stats, prefix):
        if self.logger is not None:
            self.logger.log_stat(prefix + "return_mean", np.mean(returns), self.t_env)
            self.logger.log_stat(prefix + "return_std", np.std(returns), self.t_env)
        returns.clear()
        for k, v in stats.items():
            if k != "n_episodes" and self.logger is not None:
                self.logger.log_stat(prefix + k + "_mean", v / stats["n_episodes"], self.t_env)
        stats.clear()
