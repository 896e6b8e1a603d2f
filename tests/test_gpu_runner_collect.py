"""ParallelRunner.collect / mapfx_runner_rollout -- the runner's episode loop as ONE launch,
with the on-device policy or a given [T, B, N] action table (include/mapfx_runner.h, the
RUN x ROLL instances of csrc/partial.hip) -- byte for byte against

  * tests/runner_ref.py, the restatement of the reference runner loop, with a MAC that
    restates the policy (mapfx.rng.partial_policy_actions) or reads the table; and
  * the step form: T mapfx_runner_step calls on a second handle with the identity MAC
    (row j = table[ts][bs[j]]) -- every tensor of the batch, the runner state and the env
    state.

The batch is pre-filled with 0xA5: a store into a row the reference never writes fails.
tests/test_runner_collect_ref.py proves on the CPU that the expected episodes have the
terminations these comparisons need.
"""
import ctypes
import re
import types

import numpy as np
import pytest

import runner_collect_cases as cc
from test_gpu_runner_shapes import CASES, FILL, REWARDS, RUNS, Logger, _batch_classes

pytestmark = pytest.mark.gpu

RS_ARRAYS = ("_alive", "_alive_prev", "_bs", "_bs_inv", "_counts", "_ep_return", "_ep_length", "_env_steps",
             "_env_actions")
ST_ARRAYS = ("pos", "steps", "at_goal", "done", "goal_cost", "node", "edge", "t", "terminated", "total_coll",
             "pdist", "pnbr")
EINVAL = -1


def _runner(tmp_path, name, grid, runs, padded=False, seed=0, tag="m"):
    """A runner over `grid` playing runs[ep % RUNS]'s instances, with no MAC.  name: a matrix
    case, or a dict of its form (N, win, K, B, limit)."""
    import torch
    from mapfx.episode import OneHot
    from mapfx.runners import ParallelRunner
    case = name if isinstance(name, dict) else CASES[name]
    mp = tmp_path / (tag + ".map")
    mp.write_text("type octile\nheight %d\nwidth %d\nmap\n%s\n" % (len(grid), len(grid[0]), "\n".join(grid)))
    N, B = case["N"], case["B"]
    sentinel, padded_cls = _batch_classes()
    args = types.SimpleNamespace(
        env="marl_partial", batch_size_run=B, device="cuda", seed=seed,
        env_args=dict(REWARDS, grid_file_path=str(mp), agents_path=str(tmp_path / "x-"), n_agents=N,
                      obs_window=case["win"], obs_knn_agents=case["K"], episode_limit=case["limit"]),
        episode_batch_cls=padded_cls if padded else sentinel, test_nepisode=B, runner_log_interval=1)
    logger = Logger()
    runner = ParallelRunner(args, logger, instance_fn=lambda ep: (runs[ep % RUNS]["starts"],
                                                                 runs[ep % RUNS]["goals"]))
    info = runner.get_env_info()
    scheme = {"state": {"vshape": info["state_shape"]},
              "obs": {"vshape": info["obs_shape"], "group": "agents"},
              "actions": {"vshape": (1,), "group": "agents", "dtype": torch.long},
              "avail_actions": {"vshape": (info["n_actions"],), "group": "agents", "dtype": torch.int},
              "reward": {"vshape": (1,)}, "terminated": {"vshape": (1,), "dtype": torch.uint8}}
    runner.setup(scheme, {"agents": N}, {"actions": ("actions_onehot", [OneHot(out_dim=5)])}, None)
    return runner, logger


def _kernel(printed):
    m = re.search(r"(partial_runner_rollout_kernel)<([^>]*)>", printed)
    return (m.group(1), m.group(2).replace(" ", "")) if m else None


def _want_kernel(name, obs=True):
    """The instance mapfx_runner_rollout launches for a matrix case: the step's fast shape at
    u8 / int16 tables, else (int32 tables, the generic shapes) the generic window instance;
    without the rows one per fast lane group."""
    win, kf, lf, tw, _ = CASES[name]["kernel"][1].split(",")
    if not obs:
        return ("partial_runner_rollout_kernel", "0,5,%s,0,false" % lf if lf in ("8", "16", "32") and kf == "5"
                else "0,0,0,0,false")
    if kf == "0" or tw == "0":
        return ("partial_runner_rollout_kernel", "%s,0,0,0,true" % win)
    return ("partial_runner_rollout_kernel", "%s,%s,%s,%s,true" % (win, kf, lf, tw))


def _assert_batch(batch, want, what, skip=()):
    td = batch.data.transition_data
    assert list(td) == list(want)
    for k, v in td.items():
        if k in skip:
            continue
        got = v.cpu().numpy()
        assert got.shape == want[k].shape and got.dtype == want[k].dtype, (what, k)
        same = got.view(np.uint8) == want[k].view(np.uint8)
        assert same.all(), (what, k, "first differing (env, t): %s" % np.argwhere(
            ~same.reshape(got.shape[0], got.shape[1], -1).all(-1))[:8].tolist())


def _assert_totals(runner, run, r):
    assert np.array_equal(runner._ep_return.cpu().numpy().view(np.uint64), run["returns"].view(np.uint64)), r
    assert np.array_equal(runner._ep_length.cpu().numpy(), run["lengths"]), r
    assert runner.t_env == run["t_env"], r


def _snapshot(runner, batch):
    """Every tensor the equivalence speaks of, as host bytes."""
    out = {"rows." + k: v.cpu().numpy().copy() for k, v in batch.data.transition_data.items()}
    out.update({"rs." + k: getattr(runner, k).cpu().numpy().copy() for k in RS_ARRAYS})
    out.update({"st." + k: getattr(runner.env, k).cpu().numpy().copy() for k in ST_ARRAYS
                if getattr(runner.env, k, None) is not None})
    out["err"] = runner.env.err.cpu().numpy().copy()
    return out


def _assert_same(a, b, what):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k, np.argwhere(
            a[k].reshape(a[k].shape[0], -1) != b[k].reshape(b[k].shape[0], -1))[:6].tolist())


def _rollout(runner, ts0, T, table=None, pol=None, rows=None):
    """mapfx_runner_rollout on the runner's handle; returns the status."""
    import torch
    from mapfx import _abi
    from mapfx._abi import lib
    from mapfx._base import as_actions
    env = runner.env
    a, adt = (None, 0) if table is None else as_actions(table, runner.device)
    return lib.mapfx_runner_rollout(
        env._h, ctypes.byref(env._state), ctypes.byref(runner._rs), ts0, T,
        None if a is None else a.data_ptr(), adt, None if pol is None else ctypes.byref(_abi.PPolicy(*pol)),
        None, ctypes.byref(runner._erows if rows is None else rows),
        torch.cuda.current_stream(runner.device).cuda_stream)


def _steps(runner, ts0, T, table):
    """T mapfx_runner_step calls with the identity MAC: row j = table[ts][bs[j]]."""
    import torch
    from mapfx._abi import check, lib
    from mapfx._base import as_actions
    env = runner.env
    for ts in range(ts0, ts0 + T):
        a, adt = as_actions(table[ts][runner._bs], runner.device)
        check(lib.mapfx_runner_step(env._h, ctypes.byref(env._state), ctypes.byref(env._out),
                                    ctypes.byref(runner._rs), a.data_ptr(), adt, a.stride(0), ts, None,
                                    ctypes.byref(runner._erows),
                                    torch.cuda.current_stream(runner.device).cuda_stream), "mapfx_runner_step")


# ------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("eps_q", cc.EPS_QS)
@pytest.mark.parametrize("name", cc.POLICY_CASES)
def test_collect_policy_matches_reference_loop(tmp_path, name, eps_q):
    """collect(eps) -- mac=None, two runs -- fills the batch, the returns, lengths, t_env and
    the logged stats like the reference loop with the restated policy as its MAC."""
    from mapfx import _abi
    ref = cc.policy_reference(name, eps_q)
    assert not cc.unmet(CASES[name], ref)
    runner, logger = _runner(tmp_path, name, ref["grid"], ref["runs"], seed=ref["seed"])
    for r, run in enumerate(ref["runs"]):
        batch = runner.collect(eps=eps_q / 2.0 ** 32)
        assert _kernel(_abi.last_kernel()) == _want_kernel(name), _abi.last_kernel()
        _assert_batch(batch, run["batch"], (name, eps_q, r))
        _assert_totals(runner, run, r)
    assert logger.stats == ref["log"]


@pytest.mark.parametrize("dtype", ["int8", "int32", "int64"])
def test_collect_given_actions_matches_reference_loop(tmp_path, dtype):
    """collect(actions=table): the matrix's seeded table with its built-in early terminations
    (one at step 0), at N = 5 (odd element offsets of the 8-byte action-block decode)."""
    import torch
    from mapfx import _abi
    name = "fast8_n5"
    ref = cc.given_reference(name)
    assert not cc.unmet(CASES[name], ref)
    assert all((run["lengths"] == 1).any() for run in ref["runs"])
    runner, logger = _runner(tmp_path, name, ref["grid"], ref["runs"])
    for r, run in enumerate(ref["runs"]):
        table = torch.as_tensor(run["table"], device="cuda").to(getattr(torch, dtype))
        batch = runner.collect(actions=table)
        assert _kernel(_abi.last_kernel()) == _want_kernel(name), _abi.last_kernel()
        _assert_batch(batch, run["batch"], (name, dtype, r))
        _assert_totals(runner, run, r)
    assert logger.stats == ref["log"]


def test_int32_tables_take_given_actions_and_refuse_the_policy(tmp_path):
    """block200_n9 (H * W > 32767: int32 goal tables): given actions pass on the generic
    instance; the policy is not offered -- MAPFX_EINVAL before any launch, collect raises."""
    import torch
    from mapfx import _abi
    from mapfx._abi import lib
    name = "block200_n9"
    ref = cc.given_reference(name)
    runner, _ = _runner(tmp_path, name, ref["grid"], ref["runs"])
    for r, run in enumerate(ref["runs"]):
        batch = runner.collect(actions=torch.as_tensor(run["table"], device="cuda"))
        assert _kernel(_abi.last_kernel()) == _want_kernel(name), _abi.last_kernel()
        _assert_batch(batch, run["batch"], (name, r))
        _assert_totals(runner, run, r)
    assert lib.mapfx_runner_rollout_offered(runner.env._h, 0) == 1
    assert lib.mapfx_runner_rollout_offered(runner.env._h, 1) == 0
    runner.reset()
    before = _snapshot(runner, runner.batch)
    assert _rollout(runner, 0, 6, pol=(1, 0, 0)) == EINVAL
    _assert_same(before, _snapshot(runner, runner.batch), "policy on int32 tables")
    t_env = runner.t_env
    with pytest.raises(ValueError, match="32767"):
        runner.collect(eps=0.0)
    assert runner.t_env == t_env


# ------------------------------------------------------------------ against the step form
@pytest.mark.parametrize("name", ["fast8_n5", "fast16_n16", "gen_n3"])
def test_rollout_equals_the_step_form(tmp_path, name):
    """One call of T = max_t against max_t mapfx_runner_step calls on a second handle; and
    T = 3 on both, continued with mapfx_runner_step on both: every tensor of the rows, the
    runner state and the env state."""
    import torch
    ref = cc.given_reference(name)
    max_t = CASES[name]["limit"] + 1
    one, _ = _runner(tmp_path, name, ref["grid"], ref["runs"], tag="a")
    two, _ = _runner(tmp_path, name, ref["grid"], ref["runs"], tag="b")
    for split, run in zip((max_t, 3), ref["runs"]):       # (reset number r plays run r's instances)
        table = torch.as_tensor(run["table"], device="cuda")
        one.reset()
        two.reset()
        assert _rollout(one, 0, split, table=table) == 0
        _steps(two, 0, split, table)
        _assert_same(_snapshot(one, one.batch), _snapshot(two, two.batch), (name, "after", split))
        if split == max_t:
            _assert_batch(one.batch, run["batch"], (name, "one call"))
        else:
            _steps(one, split, max_t - split, table)
            _steps(two, split, max_t - split, table)
            _assert_same(_snapshot(one, one.batch), _snapshot(two, two.batch), (name, "continued"))
            _assert_batch(one.batch, run["batch"], (name, "continued"))


@pytest.mark.parametrize("name", ["fast32_n17", "gen_n3"])
def test_waves_that_leave_the_loop_equal_the_step_form(tmp_path, name):
    """Pure descent on the policy maps ends whole waves early (fast32_n17: 2 envs per wave,
    envs 0 and 1 end after 1 and 2 steps, envs 4 and 5 after 3 and 1): such a wave leaves the
    kernel's loop, yet the env state equals what the step form -- which goes on stepping
    terminated envs -- leaves after max_t steps.  The table is the reference's recorded
    actions of the policy, so the rows are the policy run's too."""
    import torch
    eps_q = 0
    ref = cc.policy_reference(name, eps_q)
    case = CASES[name]
    max_t = case["limit"] + 1
    one, _ = _runner(tmp_path, name, ref["grid"], ref["runs"], seed=ref["seed"], tag="a")
    two, _ = _runner(tmp_path, name, ref["grid"], ref["runs"], seed=ref["seed"], tag="b")
    for r, run in enumerate(ref["runs"]):
        if name == "fast32_n17":
            assert run["lengths"][[0, 1, 4, 5]].tolist() == [1, 2, 3, 1]
        table = np.full((max_t, case["B"], case["N"]), 4, np.int64)
        for t, bs, a, _ in run["macs"]:
            table[t, bs] = a
        table = torch.as_tensor(table, device="cuda")
        one.reset()
        two.reset()
        assert _rollout(one, 0, max_t, pol=(run["pseed"], eps_q, 0)) == 0
        _steps(two, 0, max_t, table)
        _assert_same(_snapshot(one, one.batch), _snapshot(two, two.batch), (name, r))
        _assert_batch(one.batch, run["batch"], (name, r))


@pytest.mark.parametrize("chunk", [1, 2, (1, 4, 1)])
def test_chunked_calls_equal_one_call(tmp_path, chunk):
    """ceil(max_t / chunk) calls leave what one call of max_t leaves, in policy mode (the
    counter is the absolute row) and with given actions."""
    import torch
    name, eps_q = "fast8_n6", 2 ** 31
    ref = cc.policy_reference(name, eps_q)
    one, _ = _runner(tmp_path, name, ref["grid"], ref["runs"], seed=ref["seed"], tag="a")
    two, _ = _runner(tmp_path, name, ref["grid"], ref["runs"], seed=ref["seed"], tag="b")
    b1, b2 = one.collect(eps=0.5), two.collect(eps=0.5, chunk=chunk)
    _assert_same(_snapshot(one, b1), _snapshot(two, b2), ("policy", chunk))
    _assert_batch(b2, ref["runs"][0]["batch"], ("policy", chunk))
    table = torch.randint(0, 5, (6, CASES[name]["B"], CASES[name]["N"]), device="cuda",
                          generator=torch.Generator("cuda").manual_seed(3))
    b1, b2 = one.collect(actions=table), two.collect(actions=table, chunk=chunk)
    _assert_same(_snapshot(one, b1), _snapshot(two, b2), ("given", chunk))


# ------------------------------------------------------------------ edges
def test_batch_of_views_of_wider_storage(tmp_path):
    """Every batch tensor a view of wider storage (time stride = row + 1 element for obs, + 3
    for the others): the per-step stride arithmetic, the staged copy-out at every 16-byte
    misalignment; the padding keeps its fill."""
    import torch
    name, eps_q = "fast8_n7", 2 ** 31
    ref = cc.policy_reference(name, eps_q)
    runner, _ = _runner(tmp_path, name, ref["grid"], ref["runs"], padded=True, seed=ref["seed"])
    for r, run in enumerate(ref["runs"]):
        batch = runner.collect(eps=0.5)
        _assert_batch(batch, run["batch"], (name, r))
        for k, wide in batch.storage.items():
            inner = int(np.prod(batch.data.transition_data[k].shape[2:]))
            assert bool((wide[:, :, inner:].contiguous().view(torch.uint8) == FILL).all()), (r, k)


def test_rows_without_obs(tmp_path):
    """rows->obs NULL: the observation rows are not built (the instance without them) and
    not written; every other field as with them."""
    from mapfx import _abi
    name, eps_q = "fast8_n5", 2 ** 31
    ref = cc.policy_reference(name, eps_q)
    run = ref["runs"][0]
    runner, _ = _runner(tmp_path, name, ref["grid"], ref["runs"], seed=ref["seed"])
    runner.reset()
    obs0 = runner.batch["obs"].cpu().numpy().copy()
    rows = type(runner._erows).from_buffer_copy(runner._erows)
    rows.obs = None
    assert _rollout(runner, 0, 6, pol=(run["pseed"], eps_q, 0), rows=rows) == 0
    assert _kernel(_abi.last_kernel()) == _want_kernel(name, obs=False), _abi.last_kernel()
    _assert_batch(runner.batch, run["batch"], name, skip=("obs",))
    got = runner.batch["obs"].cpu().numpy()
    assert np.array_equal(got.view(np.uint8), obs0.view(np.uint8))       # row 0 from reset, the rest fill
    assert (got[:, 1:].view(np.uint8) == FILL).all()
    assert np.array_equal(runner._ep_length.cpu().numpy(), run["lengths"])


def test_invalid_action_skips_its_env_for_that_step(tmp_path):
    """An action outside 0..4 at one (ts, env): that env is skipped for that step and err is
    set, exactly as the step form does it; the rows of its wave neighbours are those of the
    clean table."""
    import torch
    name = "fast8_n5"
    ref = cc.given_reference(name)
    run = ref["runs"][0]
    bad_t, bad_env = 1, 4                      # env 4: random instance, running at step 1
    assert run["lengths"][bad_env] > 2
    table = torch.as_tensor(run["table"], device="cuda").clone()
    table[bad_t, bad_env, 2] = 7
    one, _ = _runner(tmp_path, name, ref["grid"], ref["runs"], tag="a")
    two, _ = _runner(tmp_path, name, ref["grid"], ref["runs"], tag="b")
    one.reset()
    two.reset()
    assert _rollout(one, 0, 6, table=table) == 0
    _steps(two, 0, 6, table)
    s1 = _snapshot(one, one.batch)
    _assert_same(s1, _snapshot(two, two.batch), "invalid action")
    assert int(s1["err"][0]) == bad_env + 1
    assert s1["rows.reward"][bad_env, bad_t, 0] == 0.0 and s1["rows.actions"][bad_env, bad_t, 2, 0] == 7
    others = [b for b in range(CASES[name]["B"]) if b != bad_env]
    for k, v in run["batch"].items():
        assert np.array_equal(s1["rows." + k][others].view(np.uint8), v[others].view(np.uint8)), k
    one.env.err.zero_()
    two.env.err.zero_()


def test_refused_calls_launch_nothing(tmp_path):
    """The MAPFX_EINVAL cases return before any launch: the batch keeps its 0xA5 fill and the
    runner and env state stay as reset left them."""
    import torch
    from mapfx import _abi
    from mapfx._abi import lib
    name = "fast8_n5"
    ref = cc.given_reference(name)
    runner, _ = _runner(tmp_path, name, ref["grid"], ref["runs"])
    runner.reset()
    env, rs, r = runner.env, runner._rs, runner._erows
    table = torch.as_tensor(ref["runs"][0]["table"], device="cuda")
    before = _snapshot(runner, runner.batch)
    assert (before["rows.reward"].view(np.uint8) == FILL).all()
    pol = (5, 0, 0)
    assert _rollout(runner, 0, 0, table=table) == EINVAL                 # T < 1
    assert _rollout(runner, -1, 2, table=table) == EINVAL                # ts0 < 0
    assert _rollout(runner, 4, 3, table=table) == EINVAL                 # ts0 + T > max_t
    assert _rollout(runner, 0, 7, pol=pol) == EINVAL
    assert _rollout(runner, 0, 6) == EINVAL                              # actions and pol NULL
    sh = torch.cuda.current_stream(runner.device).cuda_stream
    st, rsp, rp, a = ctypes.byref(env._state), ctypes.byref(rs), ctypes.byref(r), table.data_ptr()
    polp = ctypes.byref(_abi.PPolicy(*pol))
    assert lib.mapfx_runner_rollout(env._h, st, rsp, 0, 6, a, 7, None, None, rp, sh) == EINVAL   # dtype
    assert lib.mapfx_runner_rollout(None, st, rsp, 0, 6, a, 2, None, None, rp, sh) == EINVAL
    assert lib.mapfx_runner_rollout(env._h, None, rsp, 0, 6, None, 0, polp, None, rp, sh) == EINVAL
    assert lib.mapfx_runner_rollout(env._h, st, None, 0, 6, None, 0, polp, None, rp, sh) == EINVAL
    assert lib.mapfx_runner_rollout(env._h, st, rsp, 0, 6, None, 0, polp, None, None, sh) == EINVAL
    _assert_same(before, _snapshot(runner, runner.batch), "refused calls")
    assert _rollout(runner, 0, 6, table=table) == 0                      # and the call itself works
    _assert_batch(runner.batch, ref["runs"][0]["batch"], "after the refusals")


def test_workgroup_path_is_refused(tmp_path):
    """N = 70 (the workgroup-per-env kernel): not offered, MAPFX_EINVAL, collect raises."""
    from mapfx._abi import lib
    name = "wg_n70"
    case = CASES[name]
    rng = np.random.RandomState(5)
    free = np.argwhere(cc.runner_ref.parse_map(case["grid"]) == 0)
    inst = dict(starts=free[rng.choice(len(free), case["N"], replace=False)][None].repeat(case["B"], 0).astype(np.int32),
                goals=free[rng.choice(len(free), case["N"], replace=False)][None].repeat(case["B"], 0).astype(np.int32))
    runner, _ = _runner(tmp_path, name, case["grid"], [inst] * RUNS)
    assert lib.mapfx_runner_rollout_offered(runner.env._h, 0) == 0
    assert lib.mapfx_runner_rollout_offered(runner.env._h, 1) == 0
    runner.reset()
    before = _snapshot(runner, runner.batch)
    assert _rollout(runner, 0, 6, pol=(1, 0, 0)) == EINVAL
    _assert_same(before, _snapshot(runner, runner.batch), "workgroup path")
    with pytest.raises(ValueError, match="n_agents"):
        runner.collect()
    with pytest.raises(ValueError, match="n_agents"):
        runner.collect(actions=np.zeros((6, case["B"], case["N"]), np.int64))


# ------------------------------------------------------------------ collect
def test_collect_reads_nothing_on_the_host_before_the_totals(tmp_path, monkeypatch):
    """Inside collect, between reset and the end-of-run totals, no .item() / .tolist() /
    .cpu() / bool() of a device tensor runs (the guard of test_gpu_runner.py)."""
    import torch
    name, eps_q = "fast8_n5", 2 ** 31
    ref = cc.policy_reference(name, eps_q)
    runner, _ = _runner(tmp_path, name, ref["grid"], ref["runs"], seed=ref["seed"])
    runner.collect(eps=0.5)            # warm: first batch, caches
    state = {"on": False, "totals": 0}
    real = {n: getattr(torch.Tensor, n) for n in ("item", "tolist", "cpu", "__bool__")}
    steps_ptr = runner._env_steps.data_ptr()

    def make(n):
        def f(self, *a, **k):
            if n == "item" and self.data_ptr() == steps_ptr:
                state["on"] = False    # the end-of-run totals: the loop is over
                state["totals"] += 1
            if state["on"] and self.is_cuda:
                raise AssertionError("%s() of a device tensor inside collect" % n)
            return real[n](self, *a, **k)
        return f

    for n in real:
        monkeypatch.setattr(torch.Tensor, n, make(n))
    real_reset = runner.reset

    def reset():
        real_reset()
        state["on"] = True

    monkeypatch.setattr(runner, "reset", reset)
    batch = runner.collect(eps=0.5)
    monkeypatch.undo()
    assert state["totals"] == 1 and not state["on"]
    _assert_batch(batch, ref["runs"][1]["batch"], "guarded run")


# ------------------------------------------------------------------ graph
def test_reset_begin_rollout_as_one_graph(tmp_path):
    """[the reset launch, mapfx_runner_begin, mapfx_runner_rollout] captured on one stream and
    replayed twice onto a re-filled batch: both replays equal the eager result, and nothing
    ran at capture time."""
    import torch
    from mapfx._abi import check, lib
    name, eps_q = "fast16_n16", 2 ** 31
    ref = cc.policy_reference(name, eps_q)
    run = ref["runs"][0]
    runner, _ = _runner(tmp_path, name, ref["grid"], ref["runs"], seed=ref["seed"])
    runner.reset()                       # the batch, its rows struct, run 0's instances and tables
    batch, env = runner.batch, runner.env

    def fill():
        for t in batch.data.transition_data.values():
            t.view(torch.uint8).fill_(FILL)

    def calls():
        env.reset()
        check(runner._call(lib.mapfx_runner_begin, ctypes.byref(runner._rs), ctypes.byref(env._obs_out),
                           ctypes.byref(runner._erows)), "mapfx_runner_begin")
        assert _rollout(runner, 0, 6, pol=(run["pseed"], eps_q, 0)) == 0

    fill()
    calls()
    eager = _snapshot(runner, batch)
    _assert_batch(batch, run["batch"], "eager")
    fill()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        calls()
    torch.cuda.synchronize()
    assert all(bool((t.view(torch.uint8) == FILL).all()) for t in batch.data.transition_data.values())
    for i in range(2):
        fill()
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(eager, _snapshot(runner, batch), ("replay", i))
