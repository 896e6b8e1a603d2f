"""PrimalBatch -- E device-resident PRIMAL worlds, sequential dynamics.

Batched counterpart of MARL-curve-main/src/envs/mapf_primal.py's
`MAPFEnv._step((agent_id, action))` (:549-637) over the C ABI in
include/mapfx_primal.h: every world takes K single-agent calls in order, each
one `State.moveAgent` (:103-135), the reward table (:579-596), `_observe`
(:343-386), `State.done` (:159-166) and `_listNextValidActions` (:639-667), all
in one HIP kernel.  `MAPFEnv` below is the single-world drop-in with the
reference's call signature.  Nothing here computes env semantics on the host.

`observe` is the read-only half: `_observe`, `_listNextValidActions`, on_goal and
`_complete` of any agents of the worlds as they stand (mapfx_primal_observe), all
queries of all worlds in one launch that writes nothing of the state.

`blocking=True` adds the stay-on-goal blocking penalty (`get_blocking_reward`,
:513-546) as a second HIP pass over the calls of a launch; see mapfx_primal.h for
the planner assumption (optimal 4-connected single-robot paths).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _abi
from ._abi import check, lib, ptr
from ._base import DeviceBatch, check_on_grid, env_mask, parse_agents, parse_map, u64
from .maps import map_stride, primal_gen_luts, primal_world

_OUT_KEYS = ("reward", "done", "next_mask", "on_goal", "valid", "obs", "vec")


def _check_placement(starts, goals, bits, H, W):
    """Distinct in-bounds starts and goals on free cells: PRIMAL keeps agents,
    goals and obstacles in one array per kind (:44-66), so the kernel assumes it."""
    for arr, what in ((starts, "starts"), (goals, "goals")):
        check_on_grid(arr, H, W, what)
        flat = arr[..., 0].astype(np.int64) * W + arr[..., 1]
        if any(len(np.unique(row)) != arr.shape[1] for row in flat):
            raise ValueError("%s must be distinct within a world" % what)
    cells = starts[..., 0].astype(np.int64) * W + starts[..., 1]
    b = bits if bits.shape[0] == cells.shape[0] else np.repeat(bits, cells.shape[0], 0)
    blocked = (np.take_along_axis(b, cells >> 3, 1) >> (cells & 7)) & 1
    if blocked.any():
        raise ValueError("an agent starts on an obstacle")


class PrimalBatch(DeviceBatch):
    """E PRIMAL worlds on one GPU.  `grids` [E|1, H, W] (negative = obstacle, as
    PRIMAL's world0) or `bits` [E|1, map_stride]; starts / goals [E, N, 2] (row, col)."""

    def __init__(self, starts, goals, grids=None, bits=None, hw=None, observation_size=10,
                 device=None, diagonal=False, past=None, blocking=False):
        super().__init__(device)
        E, N, starts, goals = parse_agents(starts, goals, "starts/goals")
        H, W, bits, map_shared = parse_map(grids, bits, hw, E, obstacle=lambda g: g < 0)
        _check_placement(starts, goals, bits, H, W)
        if diagonal:
            # agents_past (DIAGONAL_MOVEMENT): equal to the starts in a fresh world (:55-66).
            # The kernels read past as int2 at [e * N + i] and primal_seq_kernel packs it
            # as biased u8 (row, col) bytes: shape and bounds are checked here
            past = starts if past is None else np.array(past, dtype=np.int32)
            if past.shape != starts.shape:
                raise ValueError("past must be [E, N, 2] like the starts, got %s" % (past.shape,))
            check_on_grid(past, H, W, "past")
        self._init(E, N, H, W, map_shared, observation_size, diagonal, blocking,
                   (bits, starts, goals, past if diagonal else None))

    def _init(self, E, N, H, W, map_shared, observation_size, diagonal, blocking, host=None):
        """The handle and the device state: `host` = checked (bits, pos, goal, past) arrays
        (__init__), or None: zeroed on the device for the generator to fill (random; no copy,
        so no host synchronisation)."""
        self.blocking = bool(blocking)
        self.E, self.N, self.H, self.W, self.map_shared = E, N, H, W, map_shared
        self.s = int(observation_size)
        self.diagonal = bool(diagonal)
        self.n_actions = 9 if self.diagonal else 5
        cfg = _abi.QCfg(H=H, W=W, n_agents=N, n_envs=E, obs_size=self.s,
                        map_shared=1 if map_shared else 0, diagonal=1 if self.diagonal else 0)
        self._create(lib.mapfx_primal_create, lib.mapfx_primal_destroy, cfg)
        if host is None:
            z = self._zeros
            self.bits = z((E, map_stride(H, W)), torch.uint8)
            self.pos, self.goal = z((E, N, 2), torch.int32), z((E, N, 2), torch.int32)
            self.past = z((E, N, 2), torch.int32) if self.diagonal else None
        else:
            self.bits, self.pos, self.goal, self.past = (
                None if a is None else torch.as_tensor(a).to(self.device).contiguous()
                for a in host)
        self.err = self._zeros((1,), torch.int32)
        self._state = _abi.QState(pos=ptr(self.pos), goal=ptr(self.goal), map_bits=ptr(self.bits),
                                  past=ptr(self.past))
        self._K = -1
        self.out = None
        self._Q = -1
        self.obs_out = None
        # the device generator (regenerate): episode counters, and no tables until
        # set_generator / PrimalBatch.random names the seed and the distribution
        self.episode = self._zeros((self.E,), torch.int32)
        self.gen_seed, self.env_offset = 0, 0
        self.side_lut = self.prob_lut = None
        self._generated = False

    @classmethod
    def random(cls, E, N, hw, seed, SIZE=(10, 40), PROB=(0, .5), observation_size=10,
               diagonal=False, blocking=False, env_offset=0, device=None, luts=None):
        """E random PRIMAL worlds of N agents drawn ON THE DEVICE (mapfx_primal_generate:
        `_setWorld`, :248-341, by the rules of include/mapfx_primal.h) in an H x W handle,
        hw = (H, W) <= (64, 64): sides and obstacle densities distributed as the
        reference's SIZE / PROB (or by `luts` = (side_lut, prob_lut), power-of-two
        lengths), agents on random free cells, every goal in its agent's connected
        region.  World e is a function of (seed, env_offset + e, its episode counter)
        alone.  Nothing of the generated state is read back or checked on the host."""
        self = cls.__new__(cls)
        DeviceBatch.__init__(self, device)
        self._init(int(E), int(N), int(hw[0]), int(hw[1]), False, observation_size, diagonal,
                   blocking)
        self.set_generator(seed, SIZE=SIZE, PROB=PROB, env_offset=env_offset, luts=luts)
        self.regenerate()
        return self

    def set_generator(self, seed, SIZE=(10, 40), PROB=(0, .5), env_offset=0, luts=None):
        """The seed, the global id of world 0 and the world distribution `regenerate`
        draws from: the reference's SIZE / PROB (maps.primal_gen_luts), or `luts` =
        (side_lut, prob_lut) of power-of-two lengths.  Tables given on the host are
        checked here (every side in 1..min(H, W) with side^2 >= N: ValueError); device
        tensors are taken as they are, and a bad side is reported per world by check_err()."""
        self.gen_seed, self.env_offset = u64(seed), int(env_offset)
        side, prob = primal_gen_luts(SIZE, PROB) if luts is None else luts
        if not torch.is_tensor(side):
            side = np.asarray(side, dtype=np.int32).reshape(-1)
            lim = min(self.H, self.W)
            if ((side < 1) | (side > lim)).any() or (side.astype(np.int64) ** 2 < self.N).any():
                raise ValueError("world sides %s do not fit: need 1 <= side <= %d (the %dx%d handle) and "
                                 "side^2 >= %d agents" % (side.tolist(), lim, self.H, self.W, self.N))
            side = torch.as_tensor(side)
        if not torch.is_tensor(prob):
            prob = torch.as_tensor(np.asarray(prob, dtype=np.uint32).reshape(-1).view(np.int32))
        # (torch has no uint32 arithmetic: the table travels as its int32 bit pattern)
        self.side_lut = side.to(self.device).to(torch.int32).contiguous()
        self.prob_lut = prob.to(self.device).contiguous()
        if self.prob_lut.element_size() != 4 or self.prob_lut.ndim != 1 or self.side_lut.ndim != 1:
            raise ValueError("side_lut / prob_lut must be 1-d tables of 32-bit entries")

    def regenerate(self, mask=None, keep_map=False):
        """A new episode, drawn on the device in one launch and in place (pos, goal, past,
        the obstacle bitmaps, `episode`), for every world or for those with mask[e] != 0
        (mask: [E], any integer / bool dtype, on the device -- e.g. out["done"][:, -1]);
        a masked-out world is untouched.  keep_map=True is the reference's blank_world:
        the obstacle maps stay (a shared map is allowed) and only agents and goals are
        placed.  Asynchronous, no host synchronisation; a world that cannot be built (a
        side that does not fit the handle or the agents, too few free cells under
        keep_map) is left as it was and reported by check_err()."""
        if not keep_map:
            if self.map_shared:
                raise ValueError("a shared-map batch regenerates with keep_map=True only")
            if self.side_lut is None:
                raise ValueError("no world distribution: call set_generator(seed, SIZE, PROB) first")
        m = env_mask(mask, self.E, self.device)
        gen = _abi.QGen(seed=self.gen_seed, env_offset=self.env_offset,
                        side_lut=ptr(self.side_lut), n_side=0 if self.side_lut is None else self.side_lut.numel(),
                        prob_lut=ptr(self.prob_lut), n_prob=0 if self.prob_lut is None else self.prob_lut.numel(),
                        episode=ptr(self.episode), mask=ptr(m), map_bits=ptr(self.bits),
                        keep_map=1 if keep_map else 0, err=ptr(self.err))
        check(self._call(lib.mapfx_primal_generate, self._h, ctypes.byref(self._state),
                         ctypes.byref(gen)), "mapfx_primal_generate")
        self._generated = True

    def _alloc(self, K):
        E, s, z = self.E, self.s, self._zeros
        self.out = {"reward": z((E, K), torch.float64), "done": z((E, K), torch.uint8),
                    "next_mask": z((E, K), torch.int16 if self.diagonal else torch.uint8),
                    "on_goal": z((E, K), torch.uint8),
                    "valid": z((E, K), torch.uint8), "obs": z((E, K, 4, s, s), torch.uint8),
                    "vec": z((E, K, 3), torch.float64)}
        self._out = _abi.QOut(err=ptr(self.err), **{k: ptr(self.out[k]) for k in _OUT_KEYS})
        if self.blocking:
            self.out["blocking"] = z((E, K), torch.uint8)
            self.out["n_blocking"] = z((E, K), torch.int32)
        self._K = K

    def act(self, agent_ids, actions, events=None):
        """K calls of `_step((agent_id, action))` per world, in order.
        agent_ids (1-based) / actions: [E, K] ints.  Returns the output dict,
        each entry [E, K, ...] (buffers reused by the next call with the same K).
        events: optional (start, stop) torch.cuda.Event pair recorded at the
        kernel's own begin / end (mapfx_primal_act_timed).  With blocking=True the
        blocking pass follows on the same stream (outside the events): "reward"
        carries the term, and the dict has "blocking" / "n_blocking" [E, K]."""
        ids = torch.as_tensor(agent_ids, device=self.device).to(torch.int32).contiguous()
        acts = torch.as_tensor(actions, device=self.device).to(torch.int32).contiguous()
        if ids.ndim != 2 or ids.shape[0] != self.E or acts.shape != ids.shape:
            raise AssertionError("agent_ids / actions must be [%d, K]" % self.E)
        K = int(ids.shape[1])
        if K != self._K:
            self._alloc(K)
        args = (self._h, ctypes.byref(self._state), ptr(ids), ptr(acts), K)
        if events is None:
            check(self._call(lib.mapfx_primal_act, *args, ctypes.byref(self._out)),
                  "mapfx_primal_act")
        else:
            check(self._call(lib.mapfx_primal_act_timed, *args, ctypes.byref(self._out),
                             events[0].cuda_event, events[1].cuda_event), "mapfx_primal_act_timed")
        if self.blocking:
            o = self.out
            check(self._call(lib.mapfx_primal_blocking, *args, ptr(o["valid"]), ptr(o["on_goal"]),
                             ptr(o["reward"]), ptr(o["blocking"]), ptr(o["n_blocking"])),
                  "mapfx_primal_blocking")
        return self.out

    def observe(self, agent_ids=None, prev_actions=None):
        """`_observe` (:343-386), `_listNextValidActions` (:639-667), on_goal and
        `State.done` of the worlds as they stand, for Q (agent, previous action) queries
        per world; nothing of the worlds changes (pos, past, an earlier `act` result).
        agent_ids (1-based) / prev_actions: [E, Q] ints; agent_ids None: every agent
        (Q = N, query q is agent q + 1); prev_actions None: 0.  Returns a dict of
        [E, Q, ...] tensors obs, vec, next_mask, on_goal, done (its own buffers, reused
        by the next call with the same Q).  A bad query (id outside 1..N, prev_action
        outside the action range) is reported by check_err(); its elements are not
        written, every other query's are."""
        ids = acts = None
        if agent_ids is not None:
            ids = torch.as_tensor(agent_ids, device=self.device).to(torch.int32).contiguous()
            if ids.ndim != 2 or ids.shape[0] != self.E:
                raise AssertionError("agent_ids must be [%d, Q]" % self.E)
        if prev_actions is not None:
            acts = torch.as_tensor(prev_actions, device=self.device).to(torch.int32).contiguous()
            if acts.ndim != 2 or acts.shape[0] != self.E or (ids is not None and acts.shape != ids.shape):
                raise AssertionError("prev_actions must be [%d, Q] like agent_ids" % self.E)
        Q = int(ids.shape[1]) if ids is not None else (int(acts.shape[1]) if acts is not None else self.N)
        if ids is None and Q != self.N:
            raise AssertionError("without agent_ids every agent is queried: Q must be %d" % self.N)
        if Q != self._Q:
            E, s, z = self.E, self.s, self._zeros
            self.obs_out = {"obs": z((E, Q, 4, s, s), torch.uint8), "vec": z((E, Q, 3), torch.float64),
                            "next_mask": z((E, Q), torch.int16 if self.diagonal else torch.uint8),
                            "on_goal": z((E, Q), torch.uint8), "done": z((E, Q), torch.uint8)}
            self._obs_out = _abi.QOut(err=ptr(self.err), **{k: ptr(v) for k, v in self.obs_out.items()})
            self._Q = Q
        check(self._call(lib.mapfx_primal_observe, self._h, ctypes.byref(self._state), ptr(ids),
                         ptr(acts), Q, ctypes.byref(self._obs_out)), "mapfx_primal_observe")
        return self.obs_out

    def blocking_count(self, agent_ids):
        """num_blocking of `get_blocking_reward(agent_ids[e])` (:513-546) in every world
        as it stands: [E] int32.  agent_ids (1-based): [E] ints."""
        ids = torch.as_tensor(agent_ids, device=self.device).to(torch.int32).contiguous()
        if ids.shape != (self.E,):
            raise AssertionError("agent_ids must be [%d]" % self.E)
        counts = self._zeros((self.E,), torch.int32)
        check(self._call(lib.mapfx_primal_blocking_count, self._h, ctypes.byref(self._state),
                         ptr(ids), ptr(counts)), "mapfx_primal_blocking_count")
        return counts

    def check_err(self):
        e = self._take_err(self.err)
        if e:
            if self._generated:
                raise AssertionError("invalid (agent_id, action), or a world the generator could not "
                                     "build (a side that does not fit, too few free cells), for world %d"
                                     % (e - 1))
            raise AssertionError("invalid (agent_id, action) for world %d" % (e - 1))


class MAPFEnv:
    """Single-world drop-in for mapf_primal.py MAPFEnv (:168-667) on the device.
    World set-up follows _setWorld (:248-341): a given world0 / goals0 (PRIMAL's
    int arrays: -1 obstacle, agent id at its start / goal cell), agents and goals
    placed on a given world (blank_world), or a random world from SIZE / PROB --
    the last two drawn on the host by mapfx.maps.primal_world from the global
    np.random / random generators, as the reference draws them.  Rendering is
    outside the hot path."""

    def __init__(self, num_agents=1, observation_size=10, world0=None, goals0=None,
                 DIAGONAL_MOVEMENT=False, SIZE=(10, 40), PROB=(0, .5), FULL_HELP=False,
                 blank_world=False, device=None, blocking=False):
        self.blocking = bool(blocking)
        self.DIAGONAL_MOVEMENT = bool(DIAGONAL_MOVEMENT)
        self.n_actions = 9 if self.DIAGONAL_MOVEMENT else 5
        self.num_agents = int(num_agents)
        self.observation_size = int(observation_size)
        self.SIZE, self.PROB, self.FULL_HELP = SIZE, PROB, FULL_HELP
        self._device = device
        self._set_world(world0, goals0, blank_world)

    def _set_world(self, world0, goals0, blank_world=False):
        if world0 is None:
            world0, goals0 = primal_world(self.num_agents, SIZE=self.SIZE, PROB=self.PROB)
        elif blank_world:
            world0, goals0 = primal_world(self.num_agents, world0=world0, blank_world=True)
        elif goals0 is None:
            raise Exception("you gave a world with no goals!")
        world0 = np.asarray(world0)
        goals0 = np.asarray(goals0)
        starts, goals = [], []
        for a in range(1, self.num_agents + 1):
            starts.append(tuple(int(v) for v in np.argwhere(world0 == a)[0]))
            goals.append(tuple(int(v) for v in np.argwhere(goals0 == a)[0]))
        self.initial_world, self.initial_goals = world0.copy(), goals0.copy()
        self._grid = np.where(world0 < 0, -1, 0).astype(np.int8)
        self.batch = PrimalBatch([starts], [goals], grids=self._grid,
                                 observation_size=self.observation_size, device=self._device,
                                 diagonal=self.DIAGONAL_MOVEMENT, blocking=self.blocking)
        self.finished = False
        self.fresh = True
        self.individual_rewards = [0 for _ in range(self.num_agents)]

    def _reset(self, agent_id, world0=None, goals0=None):
        """:389-402 -> (next valid actions, on_goal, False)."""
        self._set_world(world0, goals0)
        o = self._query(agent_id, 0)  # a query: the new world (agents_past too) stays as set
        mask = int(o["next_mask"][0, 0].item())
        return ([a for a in range(self.n_actions) if (mask >> a) & 1],
                bool(o["on_goal"][0, 0].item()), False)

    def _query(self, agent_id, prev_action):
        assert agent_id in range(1, self.num_agents + 1)
        assert prev_action in range(self.n_actions)
        return self.batch.observe([[agent_id]], [[prev_action]])

    def _observe(self, agent_id):
        """:343-386 -> ([poss_map, goal_map, goals_map, obs_map], [dx, dy, mag])."""
        assert (agent_id > 0)
        o = self._query(agent_id, 0)
        obs = o["obs"][0, 0].cpu().numpy()
        return ([obs[i] for i in range(4)], o["vec"][0, 0].cpu().tolist())

    def _listNextValidActions(self, agent_id, prev_action=0, episode=0):
        """:639-667 -> the valid actions, ascending, without the opposite of prev_action."""
        mask = int(self._query(agent_id, prev_action)["next_mask"][0, 0].item())
        return [a for a in range(self.n_actions) if (mask >> a) & 1]

    def _complete(self):
        """:404-405 -> world.done()."""
        return bool(self.batch.observe([[1]])["done"][0, 0].item())

    def get_blocking_reward(self, agent_id):
        """:513-546 -> num_blocking * BLOCKING_COST of the world as it stands."""
        assert agent_id in range(1, self.num_agents + 1)
        return int(self.batch.blocking_count([agent_id])[0].item()) * -1.0

    def getObstacleMap(self):
        return (self._grid == -1).astype(int)

    def getGoals(self):
        return [tuple(int(v) for v in g) for g in self.batch.goal[0].tolist()]

    def getPositions(self):
        return [tuple(int(v) for v in p) for p in self.batch.pos[0].tolist()]

    def _step(self, action_input, episode=0):
        """:549-637 -> (state, reward, done, nextActions, on_goal, blocking, valid)."""
        assert len(action_input) == 2, 'Action input should be a tuple with the form (agent_id, action)'
        assert action_input[1] in range(self.n_actions), 'Invalid action'
        assert action_input[0] in range(1, self.num_agents + 1)
        agent_id, action = action_input
        o = self.batch.act([[agent_id]], [[action]])
        obs = o["obs"][0, 0].cpu().numpy()
        vec = o["vec"][0, 0].cpu().tolist()
        reward = float(o["reward"][0, 0].item())
        done = bool(o["done"][0, 0].item())
        mask = int(o["next_mask"][0, 0].item())
        self.individual_rewards[agent_id - 1] = reward
        self.finished |= done
        next_actions = [a for a in range(self.n_actions) if (mask >> a) & 1]
        state = ([obs[i] for i in range(4)], vec)
        blocking = bool(o["blocking"][0, 0].item()) if self.blocking else False
        return (state, reward, done, next_actions, bool(o["on_goal"][0, 0].item()), blocking,
                bool(o["valid"][0, 0].item()))
