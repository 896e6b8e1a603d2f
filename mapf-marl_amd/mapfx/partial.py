"""MarlPartialBatch -- E device-resident MARL_PARTIAL_ENV instances.

Batched counterpart of MARL-curve-main/src/envs/marl_partial.py over the C ABI
in include/mapfx_partial.h: goal-distance tables by a bit-parallel BFS kernel
(:906-928), reset (:125-163), step (:165-310) and get_obs / get_state /
get_avail_actions (:312-433) as HIP kernels.  Observations are float32 (the dtype
PyMARL's EpisodeBatch stores them in); rewards are fp64 in the reference's
operation order.  Nothing here computes env semantics on the host.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _abi
from ._abi import MAPFX_I8, check, lib, ptr
from ._base import DeviceBatch, as_actions, avail_bits, parse_agents, parse_map, u64
from ._base import env_mask as _env_mask    # (the methods' own `env_mask` argument hides it)

DEFAULTS = dict(  # MARL_PARTIAL_ENV.__init__ defaults (:25-47)
    obs_window=5, obs_knn_agents=5, episode_limit=100, move_reward=-0.01, stay_reward=-0.02,
    stay_goal_reward=0, node_collide_reward=-1, edge_collide_reward=-1, env_collide_reward=-1,
    complete_reward=1000, complete_fac=1.5, gamma=0.99)


class MarlPartialBatch(DeviceBatch):
    """E independent MARL_PARTIAL_ENV envs on one GPU.  `grids` [E|1, H, W]
    (nonzero = obstacle) or `bits` [E|1, map_stride]; init_pos / goals [E, N, 2]."""

    def __init__(self, init_pos, goals, grids=None, bits=None, hw=None, device=None, env_offset=0,
                 packed=False, *, output=False, repair_seed=0, repair_rounds=16, **params):
        unknown = set(params) - set(DEFAULTS)
        if unknown:
            raise TypeError("unknown MARL_PARTIAL_ENV parameters: %s" % sorted(unknown))
        p = dict(DEFAULTS)
        p.update(params)
        self.params = p
        super().__init__(device)
        self.E, self.N, init_pos, goals = parse_agents(init_pos, goals, "init_pos/goals")
        self.H, self.W, bits, self.map_shared = parse_map(grids, bits, hw, self.E)
        self.episode_limit = int(p["episode_limit"])
        self.env_offset = int(env_offset)
        cfg = _abi.PCfg(H=self.H, W=self.W, n_agents=self.N, n_envs=self.E,
                        env_offset=int(env_offset), episode_limit=self.episode_limit,
                        obs_window=int(p["obs_window"]), obs_knn_agents=int(p["obs_knn_agents"]),
                        map_shared=1 if self.map_shared else 0,
                        move_reward=float(p["move_reward"]), stay_reward=float(p["stay_reward"]),
                        stay_goal_reward=float(p["stay_goal_reward"]),
                        node_collide_reward=float(p["node_collide_reward"]),
                        edge_collide_reward=float(p["edge_collide_reward"]),
                        env_collide_reward=float(p["env_collide_reward"]),
                        complete_reward=float(p["complete_reward"]),
                        complete_fac=float(p["complete_fac"]), gamma=float(p["gamma"]))
        self._create(lib.mapfx_partial_create, lib.mapfx_partial_destroy, cfg)
        self.obs_dim = int(lib.mapfx_partial_obs_dim(self._h))
        E, N, dev, z = self.E, self.N, self.device, self._zeros
        self.bits = torch.as_tensor(bits).to(dev)
        self.init_pos = torch.as_tensor(init_pos).to(dev).contiguous()
        self.goal = torch.as_tensor(goals).to(dev).contiguous()
        # `packed`: what the drop-in env reads after a step (positions, flags and the
        # outputs) are views of ONE flat buffer, pulled to the host with one copy
        spec = {"pos": ((E, N, 2), torch.int32), "done": ((E, N), torch.uint8),
                "terminated": ((E,), torch.uint8), "t": ((E,), torch.int32),
                "err": ((1,), torch.int32), "reward": ((E,), torch.float64),
                "obs": ((E, N, self.obs_dim), torch.float32), "state": ((E, 3), torch.float32),
                "avail": ((E, N), torch.uint8)}
        v = self._alloc_spec(spec, packed)
        self.pos, self.done, self.terminated, self.t, self.err = (
            v["pos"], v["done"], v["terminated"], v["t"], v["err"])
        self.pos.copy_(self.init_pos)
        self.steps = z((E, N), torch.int32)
        self.at_goal = z((E, N), torch.uint8)
        self.goal_cost = z((E, N), torch.int32)
        self.node = z((E, N), torch.uint8)
        self.edge = z((E, N), torch.int32)
        self.total_coll = z((E,), torch.int32)
        # goal distance of each agent's current cell, carried by the kernels (INT32_MIN:
        # not known yet, looked up; reset / observe set it)
        self.pdist = torch.full((E, N), -2 ** 31, dtype=torch.int32, device=dev)
        # u8 (255 = -1) while H * W <= 255, int16 up to 32767 cells, else int32
        gd_dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[
            int(lib.mapfx_partial_goal_dist_elem_size(self.H, self.W))]
        self.goal_dist = z((E, N, self.H * self.W), gd_dt)
        # the goal distances of each agent's 4 neighbour cells, carried with pdist (u8 /
        # int16 tables): a step reads a moving agent's npd from it
        self.pnbr = z((E, N, 4), torch.int16) if gd_dt != torch.int32 else None
        self.out = {k: v[k] for k in ("reward", "obs", "state", "avail")}
        self._state = _abi.PState(
            pos=ptr(self.pos), goal=ptr(self.goal), init_pos=ptr(self.init_pos),
            steps=ptr(self.steps), at_goal=ptr(self.at_goal), done=ptr(self.done),
            goal_cost=ptr(self.goal_cost), node=ptr(self.node), edge=ptr(self.edge), t=ptr(self.t),
            terminated=ptr(self.terminated), total_coll=ptr(self.total_coll),
            map_bits=ptr(self.bits), goal_dist=ptr(self.goal_dist), pdist=ptr(self.pdist),
            pnbr=ptr(self.pnbr) if self.pnbr is not None else None)
        self._out = _abi.POut(reward=ptr(self.out["reward"]), obs=ptr(self.out["obs"]),
                              state=ptr(self.out["state"]), avail=ptr(self.out["avail"]),
                              err=ptr(self.err))
        self._obs_out = _abi.POut(reward=None, obs=ptr(self.out["obs"]),
                                  state=ptr(self.out["state"]), avail=ptr(self.out["avail"]),
                                  err=ptr(self.err))
        self._scen = None   # set_scenarios: the device scenario draw's table and counters
        self._traj_cache = {}   # rollout: (T, obs, policy mode) -> its trajectory tensors
        # output mode (:262-275): every step is followed by mapfx_partial_repair
        self.output = bool(output)
        if self.output:
            if not lib.mapfx_partial_repair_offered(self._h):
                raise ValueError("output mode's device repair is not offered for n_agents = %d on a "
                                 "%d x %d map (it needs n_agents <= 64 and sides <= 256)"
                                 % (self.N, self.H, self.W))
            if not 1 <= int(repair_rounds) <= 16:
                raise ValueError("repair_rounds must be in 1..16")
            self.repair_flags = z((E,), torch.uint8)
            self.repair_rounds_used = z((E, 2), torch.int32)
            self._old_pos = z((E, N, 2), torch.int32)
            self._repair = _abi.PRepair(seed=u64(repair_seed), old_pos=ptr(self._old_pos), actions=None,
                                        action_dtype=MAPFX_I8, max_rounds=int(repair_rounds),
                                        flags=ptr(self.repair_flags), rounds=ptr(self.repair_rounds_used))
        self.compute_goal_dist()

    # ------------------------------------------------------------------ API
    def compute_goal_dist(self, env_mask=None):
        """BFS tables of the (masked) envs' goals (:906-928)."""
        m = _env_mask(env_mask, self.E, self.device)
        check(self._call(lib.mapfx_partial_goal_dist, self._h, ctypes.byref(self._state), ptr(m)),
              "mapfx_partial_goal_dist")

    def set_agents(self, init_pos, goals, env_mask=None):
        """New starts / goals (the reference re-samples them at every reset, :130)
        for the masked envs, and their goal-distance tables."""
        ip = torch.as_tensor(np.array(init_pos, dtype=np.int32), device=self.device)
        gl = torch.as_tensor(np.array(goals, dtype=np.int32), device=self.device)
        if env_mask is None:
            self.init_pos.copy_(ip)
            self.goal.copy_(gl)
        else:
            m = torch.as_tensor(env_mask, device=self.device).bool()
            self.init_pos[m] = ip[m]
            self.goal[m] = gl[m]
        self.compute_goal_dist(env_mask)

    def set_scenarios(self, lines, n_lines, seed):
        """Upload the scenario table (maps.load_scen_table) that `redraw` draws from:
        `episode` [E] int32 counts each env's draws from 0."""
        lines = np.ascontiguousarray(lines, dtype=np.int16)
        n_lines = np.ascontiguousarray(n_lines, dtype=np.int32)
        if lines.ndim != 3 or lines.shape[2] != 4 or n_lines.shape != (lines.shape[0],):
            raise ValueError("lines must be [F, Lmax, 4] and n_lines [F]")
        if n_lines.size and (n_lines.min() < 0 or n_lines.max() > lines.shape[1]):
            raise ValueError("n_lines must be within 0..Lmax")
        self.scen_lines = torch.as_tensor(lines).to(self.device)
        self.scen_n_lines = torch.as_tensor(n_lines).to(self.device)
        self.episode = torch.zeros((self.E,), dtype=torch.int32, device=self.device)
        # the draw's own report (1 + a bad env), apart from the invalid-action one
        self.scen_err = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._scen = _abi.PScen(seed=u64(seed), lines=ptr(self.scen_lines),
                                n_lines=ptr(self.scen_n_lines), n_files=int(lines.shape[0]),
                                l_max=int(lines.shape[1]), init_pos=ptr(self.init_pos),
                                goal=ptr(self.goal), episode=ptr(self.episode), mask=None,
                                err=ptr(self.scen_err))

    def redraw(self, env_mask=None):
        """New starts / goals of the masked envs (all if None) drawn on the device
        (mapfx_partial_draw: a uniform scen file, a uniform ordered sample of its lines --
        rng.scen_draw names them) and their goal-distance tables.  No host sync, no copy
        of instances; a file with no more than n_agents lines shows in check_err()."""
        if self._scen is None:
            raise RuntimeError("redraw needs set_scenarios(lines, n_lines, seed) first")
        m = _env_mask(env_mask, self.E, self.device)
        self._scen.mask = ptr(m)
        check(self._call(lib.mapfx_partial_draw, self._h, ctypes.byref(self._scen)),
              "mapfx_partial_draw")
        self.compute_goal_dist(m)

    def reset(self, env_mask=None):
        """:125-163 for the masked envs (all if None); observations of every env."""
        m = _env_mask(env_mask, self.E, self.device)
        check(self._call(lib.mapfx_partial_reset, self._h, ctypes.byref(self._state), ptr(m),
                         ctypes.byref(self._obs_out)), "mapfx_partial_reset")
        return self.out

    def observe(self):
        check(self._call(lib.mapfx_partial_observe, self._h, ctypes.byref(self._state),
                         ctypes.byref(self._obs_out)), "mapfx_partial_observe")
        return self.out

    def step(self, actions):
        """One step of all E envs (:165-310).  actions: [E, N] int8/int32/int64."""
        a, dt = as_actions(actions, self.device, (self.E, self.N))
        if self.output:
            self._old_pos.copy_(self.pos)
        check(self._call(lib.mapfx_partial_step, self._h, ctypes.byref(self._state), a.data_ptr(),
                         dt, ctypes.byref(self._out)), "mapfx_partial_step")
        if self.output:   # the collision repair, then the observations of the repaired state
            self._repair.actions, self._repair.action_dtype = a.data_ptr(), dt
            check(self._call(lib.mapfx_partial_repair, self._h, ctypes.byref(self._state),
                             ctypes.byref(self._repair), ctypes.byref(self._obs_out)),
                  "mapfx_partial_repair")
        return self.out

    TRAJ_KEYS = ("reward", "obs", "state", "avail", "pos", "terminated", "actions")

    def rollout_fused(self):
        """True: `rollout` is one launch (the wave kernel); False: a loop of step launches
        (N > 64 or a side > 256)."""
        return bool(lib.mapfx_partial_rollout_fused(self._h))

    def _traj_spec(self, T, obs, policy):
        E, N = self.E, self.N
        spec = {"reward": ((T, E), torch.float64), "state": ((T, E, 3), torch.float32),
                "avail": ((T, E, N), torch.uint8), "pos": ((T, E, N, 2), torch.int32),
                "terminated": ((T, E), torch.uint8)}
        if obs:
            spec["obs"] = ((T, E, N, self.obs_dim), torch.float32)
        if policy:
            spec["actions"] = ((T, E, N), torch.int8)
        return spec

    def policy_rule_offered(self, policy):
        """True where the on-device policy rule `policy` ("descent" / "pibt") can be used."""
        rule = _abi.POLICY_RULES.get(policy)
        return rule is not None and bool(lib.mapfx_partial_policy_rule_offered(self._h, rule))

    def set_policy_rule(self, policy):
        """The rule of the next policy-mode launches of this batch (mapfx_partial_policy_rule):
        "descent" or "pibt".  ValueError for an unknown rule or one not offered here (pibt:
        n_agents <= 64, sides <= 256 and H * W <= 32767)."""
        if policy not in _abi.POLICY_RULES:
            raise ValueError("policy must be one of %s, not %r" % (sorted(_abi.POLICY_RULES), policy))
        if not self.policy_rule_offered(policy):
            raise ValueError("policy %r is not offered for n_agents = %d on a %d x %d map (it needs "
                             "n_agents <= 64, sides <= 256 and H * W <= 32767)"
                             % (policy, self.N, self.H, self.W))
        check(lib.mapfx_partial_policy_rule(self._h, _abi.POLICY_RULES[policy]), "mapfx_partial_policy_rule")

    def rollout(self, actions=None, T=None, *, eps=None, seed=0, t0=0, autoreset=False, obs=True,
                out=None, policy="descent"):
        """T steps in one call (mapfx_partial_rollout; one launch where `rollout_fused()`).

        actions: [T, E, N] int8 / int32 / int64 -- or actions=None with T and eps (a float in
        0..1, mapped to eps_q = round(eps * 2**32), or an int eps_q in 0..2**32): the
        on-device policy (rng.partial_policy_actions: shortest-path descent with eps-random
        moves keyed by (seed, global env, t0 + k, agent)) -- or, with policy="pibt", the
        collision-free rule rng.partial_policy_pibt_actions (priority inheritance with
        backtracking; the same eps and keys).  The rule is set per call; ValueError where it
        is not offered.  autoreset: an env whose
        terminated flag is set restarts from init_pos before it is stepped.  Returns a dict
        of trajectory tensors whose slot k is what the k-th of T `step` calls returns --
        reward [T, E], obs [T, E, N, D] (absent and not built with obs=False), state, avail,
        pos and terminated after that step, actions in policy mode -- allocated once per
        (T, obs, mode) and reused, or the caller's own `out` (the same keys; a missing one
        is not produced)."""
        if self.output:
            raise ValueError("rollout is not offered in output mode (the repair is not fused "
                             "into the rollout kernels): use step()")
        self.set_policy_rule(policy)
        policy = actions is None
        if policy:
            if T is None or eps is None:
                raise ValueError("rollout needs actions, or T and eps for the on-device policy")
            T = int(T)
            if isinstance(eps, (int, np.integer)) and not isinstance(eps, bool):
                eps_q = int(eps)
            else:
                if not 0.0 <= float(eps) <= 1.0:
                    raise ValueError("eps must be a float in 0..1 or an int eps_q in 0..2**32")
                eps_q = int(round(float(eps) * 2 ** 32))
            if not 0 <= eps_q <= 2 ** 32:
                raise ValueError("eps_q must be in 0..2**32")
            a, dt = None, MAPFX_I8
            pol = _abi.PPolicy(seed=u64(seed), eps_q=eps_q, t0=int(t0))
        else:
            a, dt = as_actions(actions, self.device)   # [T, E, N] with T its own: checked here
            if a.dim() != 3 or tuple(a.shape[1:]) != (self.E, self.N) or \
                    (T is not None and int(T) != a.shape[0]):
                raise AssertionError("actions must be [T, %d, %d]" % (self.E, self.N))
            T, pol = int(a.shape[0]), None
        spec = self._traj_spec(T, obs, policy)
        if out is None:
            key = (T, bool(obs), policy)
            out = self._traj_cache.get(key)
            if out is None:
                out = self._traj_cache[key] = self._zeros_of(spec)
        else:
            for k, t in out.items():
                if k not in spec:
                    raise AssertionError("rollout: no trajectory array %r in this mode" % (k,))
                shape, d = spec[k]
                if tuple(t.shape) != shape or t.dtype != d or not t.is_contiguous() or \
                        t.device != self.pos.device:
                    raise AssertionError("out[%r] must be a contiguous %s %s on %s"
                                         % (k, d, list(shape), self.pos.device))
        traj = _abi.PTraj(err=ptr(self.err), **{k: ptr(out.get(k)) for k in self.TRAJ_KEYS})
        check(self._call(lib.mapfx_partial_rollout, self._h, ctypes.byref(self._state), T, ptr(a), dt,
                         ctypes.byref(pol) if pol is not None else None, 1 if autoreset else 0,
                         ctypes.byref(traj)), "mapfx_partial_rollout")
        return out

    def check_err(self):
        e = self._take_err(self.scen_err) if self._scen is not None else 0
        if e:
            raise AssertionError("scenario file with no more than n_agents lines drawn for "
                                 "env %d" % (e - 1))
        super().check_err()

    def avail_actions(self):
        """[E, N, 5] int64 0/1 (get_avail_actions)."""
        return avail_bits(self.out["avail"])
