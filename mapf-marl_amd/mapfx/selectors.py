"""Action selection on the device: PyMARL's EpsilonGreedyActionSelector and
MultinomialActionSelector (MARL-curve-main/src/components/action_selectors.py) as ONE launch
of mapfx_select_actions (include/mapfx_runner.h; the rule is mapfx.rng.select_actions).

The random words are counter-based and keyed by (seed, global env id, step, agent), like
every other stream of the library: an env's actions do not depend on which other rows the
call holds.  The batched ParallelRunner binds each call's keys (`bind`), so a run with the
padded `bs`, a run with args.runner_exact_bs and a sharded run pick the same actions.  The
distribution is the reference selectors'; the numbers are not torch's.

Register them in PyMARL with
    from mapfx.selectors import REGISTRY as MAPFX_SELECTORS
    action_REGISTRY.update(MAPFX_SELECTORS)      # action_selector: "mapfx_epsilon_greedy"
"""
from __future__ import annotations

import ctypes

import torch

from . import _abi
from ._abi import check, lib, ptr
from .rng import SELECT_MODES, runner_policy_seed


def _rows_ok(t, inner):
    """[rows, ...] with dense rows of `inner` elements, any row stride not below it."""
    want, ok = 1, True
    for d in range(t.dim() - 1, 0, -1):
        ok = ok and (t.shape[d] == 1 or t.stride(d) == want)
        want *= t.shape[d]
    return ok and (t.shape[0] <= 1 or t.stride(0) >= inner)


def select_actions(q, avail=None, *, eps, seed, t, env_ids=None, env_offset=0, mode="epsilon_greedy",
                   greedy=False, out=None):
    """Actions int64 [rows, N] from q [rows, N, A] (Q-values, or policies with
    mode="multinomial"), A <= 9, in one launch on q's device and current stream.

    avail: None (every action available), [rows, N, A] of any dtype (nonzero = available;
    int32, the EpisodeBatch's dtype, is read in place), or the env calls' packed masks [rows, N]
    (uint8, A <= 8; int16 / uint16, A == 9: bit i = action i).  eps in 0..1 is epsilon (unused
    by "multinomial"), `greedy` selects the greedy action only.  Row j is global env env_offset
    + (env_ids[j] if env_ids is given, a LongTensor [rows], else j); seed and the step counter
    t are the other keys.  A non-float32 or non-contiguous q is converted first."""
    if q.dim() != 3:
        raise ValueError("q must be [rows, N, A], got %s" % (tuple(q.shape),))
    rows, N, A = (int(s) for s in q.shape)
    if not q.is_cuda:
        raise ValueError("q must be a device tensor")
    if not 0.0 <= float(eps) <= 1.0:
        raise ValueError("eps must be in 0..1")
    if q.dtype != torch.float32 or not _rows_ok(q, N * A):
        q = q.to(torch.float32).contiguous()
    dev = q.device
    form, av_sr = _abi.MAPFX_AVAIL_I32, 0
    if avail is not None:
        if avail.device != dev:
            raise ValueError("avail is on %s, q on %s" % (avail.device, dev))
        if avail.dim() == 2:
            if tuple(avail.shape) != (rows, N) or avail.dtype not in (
                    (torch.uint8,) if A <= 8 else (torch.int16, getattr(torch, "uint16", torch.int16))):
                raise ValueError("packed avail must be [rows, N] uint8 (A <= 8) or int16 (A == 9)")
            form = _abi.MAPFX_AVAIL_BITS
            if not _rows_ok(avail, N):
                avail = avail.contiguous()
            av_sr = avail.stride(0) if rows > 1 else N
        else:
            if tuple(avail.shape) != (rows, N, A):
                raise ValueError("avail must be [rows, N, A] like q, got %s" % (tuple(avail.shape),))
            if avail.dtype != torch.int32:
                avail = (avail != 0).to(torch.int32)
            if not _rows_ok(avail, N * A):
                avail = avail.contiguous()
            av_sr = avail.stride(0) if rows > 1 else N * A
    if env_ids is not None:
        if env_ids.dtype != torch.int64 or env_ids.device != dev or tuple(env_ids.shape) != (rows,):
            raise ValueError("env_ids must be an int64 [rows] tensor on q's device")
        env_ids = env_ids.contiguous()
    if out is None:
        out = torch.empty((rows, N), dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or out.device != dev or tuple(out.shape) != (rows, N) or \
            not _rows_ok(out, N):
        raise ValueError("out must be an int64 [rows, N] tensor with dense rows on q's device")
    a = _abi.SelArgs(rows=rows, N=N, A=A, q=ptr(q), q_sr=q.stride(0) if rows > 1 else N * A,
                     avail=ptr(avail), avail_sr=av_sr, avail_form=form, env_ids=ptr(env_ids),
                     env_offset=int(env_offset), seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                     eps_q=int(round(float(eps) * 2 ** 32)), t=int(t) & 0xFFFFFFFF,
                     mode=SELECT_MODES[mode], greedy_only=1 if greedy else 0, actions=ptr(out),
                     actions_sr=out.stride(0) if rows > 1 else N)
    rc = lib.mapfx_select_actions(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        check(rc, "mapfx_select_actions")
    return out


class _DeviceSelector:
    """PyMARL's selector surface over select_actions: select_action(agent_inputs,
    avail_actions, t_env, test_mode), the `epsilon` attribute the runner logs, and the
    reference's DecayThenFlatSchedule(args.epsilon_start, args.epsilon_finish,
    args.epsilon_anneal_time, decay="linear"): epsilon(T) = max(finish, start - (start -
    finish) / anneal_time * T)."""
    mode = None

    def __init__(self, args):
        self.args = args
        self._start, self._finish = float(args.epsilon_start), float(args.epsilon_finish)
        self._delta = (self._start - self._finish) / args.epsilon_anneal_time
        self.epsilon = self._schedule(0)
        self._base_seed = int(getattr(args, "seed", 0) or 0)
        self._seed = (None, 0)      # (run, rng.runner_policy_seed(seed, run))
        self._bound = None
        self._calls = 0

    def _schedule(self, T):
        return max(self._finish, self._start - self._delta * T)

    def bind(self, env_ids, t_ep, run, env_offset=0):
        """The keys of the NEXT select_action call: row j is global env env_offset +
        env_ids[j] (the runner's `bs`), the step counter is t_ep and the seed
        rng.runner_policy_seed(args.seed, run).  Unbound (an EpisodeRunner, any other loop):
        rows are envs 0 .. rows - 1, the counter counts this object's calls and run is 0."""
        self._bound = (env_ids, int(t_ep), int(run), int(env_offset))

    def _keys(self):
        env_ids, t, run, off = self._bound or (None, self._calls, 0, 0)
        self._bound = None
        self._calls += 1
        if self._seed[0] != run:
            self._seed = (run, runner_policy_seed(self._base_seed, run))
        return dict(env_ids=env_ids, t=t, env_offset=off, seed=self._seed[1])


class DeviceEpsilonGreedySelector(_DeviceSelector):
    """EpsilonGreedyActionSelector (action_selectors.py:40-71) in one launch."""
    mode = "epsilon_greedy"

    def select_action(self, agent_inputs, avail_actions, t_env, test_mode=False):
        self.epsilon = 0.0 if test_mode else self._schedule(t_env)
        return select_actions(agent_inputs, avail_actions, eps=self.epsilon, mode=self.mode,
                              greedy=bool(test_mode), **self._keys())


class DeviceMultinomialSelector(_DeviceSelector):
    """MultinomialActionSelector (action_selectors.py:7-37) in one launch."""
    mode = "multinomial"

    def __init__(self, args):
        super().__init__(args)
        self.test_greedy = getattr(args, "test_greedy", True)

    def select_action(self, agent_inputs, avail_actions, t_env, test_mode=False):
        self.epsilon = self._schedule(t_env)
        return select_actions(agent_inputs, avail_actions, eps=0.0, mode=self.mode,
                              greedy=bool(test_mode and self.test_greedy), **self._keys())


REGISTRY = {"mapfx_epsilon_greedy": DeviceEpsilonGreedySelector,
            "mapfx_multinomial": DeviceMultinomialSelector}
