"""Graph replay and side-stream launches of every entry point, against the oracles.

Every other device test launches eagerly on the default stream.  There a launch that ignores
its `stream` argument cannot be told from a correct one, and nothing shows whether a wrapper
fixes at call time what INTEGRATION.md ("Graphs and streams") says lives in device buffers.
Here the wrapper calls of a case are captured into ONE HIP graph (torch.cuda.graph, a strictly
linear chain on one side stream) and replayed with other inputs written in place.

The protocol (`replay_protocol`, the same for every case):
  1  the batch is built on the default stream; actions, masks and a log with one slot per
     call (every state array and every output the family's `compare` reads) are static
     device tensors of the dtype the wrapper takes in place;
  2  one eager pass on the side stream with episode A loaded, compared with A's snapshots --
     the suite's eager off-default-stream run;
  3  outputs and log are filled with 0xA5, the state is copied, the calls are captured,
     each followed by the copies into its log slot;
  4  after the capture the state equals the copy and every output and log byte is still
     0xA5: nothing ran at capture time;
  5  mapfx_last_kernel (rollouts: mapfx_last_action_path too) read inside the capture equals
     the case table's expected instance, so the captured instance is the pinned one;
  6  replays with A, B, C and A again loaded in place, each compared slot by slot and bit
     for bit with that episode's snapshots; `err` names A's refused env and is 0 after B, C.

The cases and their three episodes come from tests/graph_replay_cases.py (what they reach:
tests/test_graph_replay_cases.py).  Four more graphs have no case table: the MARL_PARTIAL
scenario draw, the PRIMAL generator, the PRIMAL blocking pass, and -- not capturable, see
test_runner_on_a_side_stream -- the runner.
"""
import types

import numpy as np
import pytest

import graph_replay_cases as grc
import mapf_step_cases as msc
import partial_step_cases as psc
import primal_step_cases as qsc
from graph_replay_cases import case_id, episodes, of_family

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 256
LEAD = GUARD + 16          # a view starts 16-byte aligned, not 256-byte aligned
ORDER = ("A", "B", "C", "A")


@pytest.fixture(scope="module")
def mapfx_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mapfx
    return mapfx


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fill(tensors):
    import torch
    for t in tensors:
        t.view(torch.uint8).fill_(FILL)


def _all_fill(t):
    import torch
    return bool((t.view(torch.uint8) == FILL).all())


# ------------------------------------------------------------------ the protocol
def replay_protocol(plan, eps, order=ORDER):
    """Steps 2 to 6 of the module docstring for one built case.  `plan`:
      calls      [(kind, fn)]: the wrapper calls in order, fn() makes one on the current stream
      state      {name: tensor}: the state arrays (compared with their copy in step 4)
      outs       {name: tensor}: the outputs copied into a call's log slot
      fill       tensors refilled with 0xA5 before every pass (the outputs' whole storage)
      load(ep)   write an episode's inputs in place, set up what it needs outside the graph
      check(ep, log, what)   compare every slot with the episode's snapshots
      after(ep)  the error word
      kernels(seen)   step 5; seen = {kind: {(mapfx_last_kernel, mapfx_last_action_path)}}
    `eps`: {name: episode}; the eager pass and the capture run with order[0] loaded."""
    import torch
    from mapfx import _abi
    cur = torch.cuda.current_stream()
    logged = dict(plan.state, **plan.outs)
    log = [{n: torch.empty_like(t) for n, t in logged.items()} for _ in plan.calls]
    log_tensors = [t for slot in log for t in slot.values()]

    def run_calls(seen=None):
        for k, (kind, fn) in enumerate(plan.calls):
            fn()
            if seen is not None:
                seen.setdefault(kind, set()).add((_abi.last_kernel(), _abi.last_action_path()))
            for n, t in logged.items():
                log[k][n].copy_(t)

    first = eps[order[0]]
    # 2: eager, on the side stream
    side = torch.cuda.Stream()
    plan.load(first)
    _fill(plan.fill + log_tensors)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        run_calls()
    cur.wait_stream(side)
    torch.cuda.synchronize()
    plan.check(first, log, "eager on the side stream")
    plan.after(first)
    # 3: capture
    plan.load(first)
    _fill(plan.fill + log_tensors)
    torch.cuda.synchronize()
    before = {n: t.clone() for n, t in plan.state.items()}
    graph = torch.cuda.CUDAGraph()
    seen = {}
    with torch.cuda.graph(graph, stream=side):
        run_calls(seen)
    torch.cuda.synchronize()
    # 4: nothing ran at capture time
    for n, t in plan.state.items():
        assert torch.equal(t, before[n]), "state array %s changed during the capture" % n
    for k, t in enumerate(plan.fill):
        assert _all_fill(t), "output storage %d written during the capture" % k
    for k, slot in enumerate(log):
        for n, t in slot.items():
            assert _all_fill(t), "log slot %d / %s written during the capture" % (k, n)
    # 5: the captured instances
    assert set(seen) == {kind for kind, _ in plan.calls}
    plan.kernels(seen)
    # 6: replays
    for r, name in enumerate(order):
        ep = eps[name]
        plan.load(ep)
        _fill(plan.fill + log_tensors)
        graph.replay()
        torch.cuda.synchronize()
        plan.check(ep, log, "replay %d (%s)" % (r, name))
        plan.after(ep)
    del graph, side


def _one(seen, kind):
    assert len(seen[kind]) == 1, (kind, seen[kind])
    return next(iter(seen[kind]))


# ------------------------------------------------------------------ MAPF
def _mapf_batch(mapfx_mod, c, b, limit=None):
    return mapfx_mod.MapfGridBatch(np.array(b["init_pos"]), np.array(b["goals"]), bits=np.array(b["bits"]),
                                   hw=(c.H, c.W), episode_limit=msc.limit_of(c) if limit is None else limit,
                                   step_reward=c.rewards[0], collide_reward=c.rewards[1], obs=c.obs,
                                   window=c.window, primal_size=c.psize, env_offset=c.env_offset,
                                   track_steps=c.track)


def _mapf_actions(c, T):
    """The static [T, E, N] action tensor of the case's dtype; int8 with act_off: a view that
    many bytes into a 16-byte aligned allocation (the action path follows the alignment)."""
    import torch
    dt = getattr(torch, c.act)
    n = T * c.E * c.N
    if not c.act_off:
        a = torch.zeros((T, c.E, c.N), dtype=dt, device="cuda")
    else:
        raw = torch.zeros(c.act_off + n + 16, dtype=torch.int8, device="cuda")
        assert raw.data_ptr() % 16 == 0
        a = raw[c.act_off:c.act_off + n].view(T, c.E, c.N)
    assert a.is_contiguous() and a.data_ptr() % 16 == c.act_off % 16
    return a


def _mapf_got(c, slot, keys, state=True):
    from mapfx.batch import window_planes
    got = {k: _np(slot[k]) for k in keys}
    if "obs_window_occ" in keys:
        got["obs_window_occ_planes"] = _np(window_planes(slot["obs_window_occ"]))
    if state:
        got.update({k: _np(slot[k]) for k in ("pos", "done", "t") + (("steps",) if c.track else ())})
    return got


def _mapf_state(batch, c):
    s = {"pos": batch.pos, "done": batch.done, "t": batch.t}
    if c.track:
        s["steps"] = batch.steps
    return s


def _mapf_after(batch):
    def after(ep):
        e = int(batch.err.item())
        want = ep.bad[1] + 1 if ep.bad is not None else 0
        assert e == want, (ep.name, e, want)
        batch.err.zero_()
    return after


def _mapf_step_plan(mapfx_mod, c, reset=True, limit=None, T=None):
    """[reset, T steps] (an observe case: observe() after every step); reset=False: the
    [T steps] graph of the carried-state form."""
    b = msc.build(c)
    batch = _mapf_batch(mapfx_mod, c, b, limit)
    T = c.T if T is None else T
    acts = _mapf_actions(c, T)
    obs_keys = msc.launch_outs(c.obs, "observe")
    step_keys = msc.launch_outs(c.obs, "step")
    assert set(step_keys) == set(batch.out)
    other = [k for k in batch.out if k not in msc.OBS_KEYS]
    calls = [("reset", batch.reset)] if reset else []
    for t in range(T):
        calls.append(("step", lambda t=t: batch.step(acts[t])))
        if c.entry == "observe":
            calls.append(("observe", batch.observe))

    def load(ep):
        acts.copy_(_dev(np.array(ep.actions).astype(c.act)))

    def check(ep, log, what):
        k = 0
        if reset:
            d = msc.compare(_mapf_got(c, log[0], obs_keys), ep.snaps[0], "reset")
            assert d is None, (what, d)
            assert all(_all_fill(log[0][n]) for n in other), what
            k = 1
        for t in range(T):
            d = msc.compare(_mapf_got(c, log[k], step_keys), ep.snaps[t + 1], t)
            assert d is None, (what, d)
            k += 1
            if c.entry == "observe":
                d = msc.compare(_mapf_got(c, log[k], obs_keys), ep.snaps[t + 1], "observe %d" % t)
                assert d is None, (what, d)
                k += 1
        assert k == len(log)

    def kernels(seen):
        if reset:
            assert msc.kernel_args(_one(seen, "reset")[0]) == msc.expected_kernel(c, "observe"), seen
        if c.entry != "step":
            assert len(seen["step"]) == 1
        name, path = _one(seen, c.entry)
        assert msc.kernel_args(name) == msc.expected_kernel(c), name
        assert path == 0

    return types.SimpleNamespace(batch=batch, acts=acts, calls=calls, state=_mapf_state(batch, c),
                                 outs=dict(batch.out), fill=list(batch.out.values()), load=load, check=check,
                                 after=_mapf_after(batch), kernels=kernels)


def _guarded(batch, c, keys):
    """{name: (raw uint8 allocation, [T, ...] view at byte LEAD of it, lead, nbytes)}; the
    case's `misalign` buffer starts one byte later."""
    import torch
    bufs = {}
    for name, (shape, dt) in batch.out_spec(c.T).items():
        if name not in keys:
            continue
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
        lead = LEAD + (1 if name == c.misalign else 0)
        raw = torch.full((lead + nbytes + GUARD,), FILL, dtype=torch.uint8, device=batch.device)
        view = raw[lead:lead + nbytes].view(dt).view(shape)
        assert view.data_ptr() % 16 == (1 if name == c.misalign else 0)
        bufs[name] = (raw, view, lead, nbytes)
    assert set(bufs) == set(keys)
    return bufs


def _mapf_rollout_plan(mapfx_mod, c, pack=False):
    """[reset, one rollout launch] into trajectory buffers with 256 guard bytes either side.
    A generator case: [rollout] alone, the episode's positions set outside the graph
    (reset() zeroes done / t / steps, set_positions writes pos).  pack: mapfx_pack_compact
    behind the rollout, cell / done_bits against pack_compact_host of the oracle's trajectory."""
    import torch
    b = msc.build(c)
    batch = _mapf_batch(mapfx_mod, c, b)
    gen = c.act == "gen"
    acts = None if gen else _mapf_actions(c, c.T)
    keys = msc.launch_outs(c.obs, "rollout", c.select)
    bufs = _guarded(batch, c, keys)
    traj = {k: v[1] for k, v in bufs.items()}
    obs_keys = msc.launch_outs(c.obs, "observe")
    calls = [] if gen else [("reset", batch.reset)]
    calls.append(("rollout", lambda: batch.rollout(c.T, actions=acts, seed=c.seed, t0=c.t0,
                                                   autoreset=c.autoreset, traj=traj, outputs=keys)))
    packed = {}
    if pack:
        packed = {"cell": torch.zeros((c.T, c.E, c.N), dtype=torch.int16, device="cuda"),
                  "done_bits": torch.zeros((c.T, c.E, (c.N + 7) // 8), dtype=torch.uint8, device="cuda")}
        calls.append(("pack", lambda: batch.pack_compact(traj["traj_pos"], traj["traj_done"],
                                                         packed["cell"], packed["done_bits"])))

    def load(ep):
        if gen:
            batch.reset()
            batch.set_positions(np.array(ep.start))
        else:
            acts.copy_(_dev(np.array(ep.actions).astype(c.act)))

    def check(ep, log, what):
        if not gen:
            d = msc.compare(_mapf_got(c, log[0], obs_keys), ep.snaps[0], "reset")
            assert d is None, (what, d)
        for k, (raw, view, lead, nbytes) in bufs.items():
            r = _np(raw)
            assert (r[:lead] == FILL).all(), "%s: %s: bytes before the buffer written" % (what, k)
            assert (r[lead + nbytes:] == FILL).all(), "%s: %s: bytes behind the buffer written" % (what, k)
        for k in range(c.T):
            d = msc.compare(_mapf_got(c, {n: v[k] for n, v in traj.items()}, keys, state=False),
                            ep.snaps[k + 1], k)
            assert d is None, (what, d)
        slot = log[0 if gen else 1]
        d = msc.compare({n: _np(slot[n]) for n in _mapf_state(batch, c)}, ep.final, "final state")
        assert d is None, (what, d)
        if pack:
            from mapfx.dist import pack_compact_host
            pos = torch.from_numpy(np.stack([s["pos"] for s in ep.snaps[1:]]))
            done = torch.from_numpy(np.stack([s["done"] for s in ep.snaps[1:]]))
            cell = torch.zeros((c.T, c.E, c.N), dtype=torch.int16)
            bits = torch.zeros((c.T, c.E, (c.N + 7) // 8), dtype=torch.uint8)
            pack_compact_host(pos, done, c.W, cell, bits, H=c.H)
            assert torch.equal(log[-1]["cell"].cpu(), cell), what
            assert torch.equal(log[-1]["done_bits"].cpu(), bits), what

    def kernels(seen):
        if not gen:
            assert msc.kernel_args(_one(seen, "reset")[0]) == msc.expected_kernel(c, "observe"), seen
        name, path = _one(seen, "rollout")
        assert msc.kernel_args(name) == msc.expected_kernel(c), name
        assert path == msc.expected_action_path(c)

    return types.SimpleNamespace(batch=batch, acts=acts, calls=calls, state=_mapf_state(batch, c),
                                 outs=dict(batch.out, **packed),
                                 fill=list(batch.out.values()) + [v[0] for v in bufs.values()]
                                 + list(packed.values()),
                                 load=load, check=check, after=_mapf_after(batch), kernels=kernels)


def _eps(family, c):
    return {e.name: e for e in episodes(family, c)}


@pytest.mark.parametrize("c", of_family("mapf"), ids=lambda c: case_id("mapf", c))
def test_mapf_case_replays_as_the_oracle(mapfx_mod, c):
    plan = _mapf_rollout_plan(mapfx_mod, c) if c.entry == "rollout" else _mapf_step_plan(mapfx_mod, c)
    replay_protocol(plan, _eps("mapf", c))


def test_mapf_rollout_and_pack_compact_in_one_graph(mapfx_mod):
    """[reset, rollout, pack_compact]: the first selected runner rollout on an action buffer."""
    c = next(c for c in of_family("mapf") if c.entry == "rollout" and c.act != "gen" and c.select == "runner")
    replay_protocol(_mapf_rollout_plan(mapfx_mod, c, pack=True), _eps("mapf", c))


def _halves(ep, T):
    """A 2T-step episode as the two replays of a [T steps] graph: the first begins from
    reset() (made outside the graph), the second from what the first left."""
    out = {}
    for h, name in enumerate(("first", "second")):
        out[name] = types.SimpleNamespace(name=name, actions=ep.actions[h * T:(h + 1) * T],
                                          snaps=[None] + list(ep.snaps[h * T + 1:(h + 1) * T + 1]),
                                          bad=None, fresh=h == 0)
    return out


def test_mapf_state_and_t_carry_across_replays(mapfx_mod):
    """[T steps] without the reset, replayed twice back to back = one 2T-step episode
    (episode_limit raised to 2T - 2: it ends inside the second replay)."""
    c, limit, ep = grc.carry_episode("mapf")
    plan = _mapf_step_plan(mapfx_mod, c, reset=False, limit=limit)
    load = plan.load

    def load_half(half):
        if half.fresh:
            plan.batch.reset()
        load(half)

    plan.load = load_half
    replay_protocol(plan, _halves(ep, c.T), order=("first", "second"))
    assert np.array_equal(_np(plan.batch.t), np.asarray(ep.snaps[-1]["t"]))


# ------------------------------------------------------------------ MARL_PARTIAL
def _partial_plan(mapfx_mod, c, reset=True, limit=None):
    import torch
    from mapfx import _abi
    b = psc.build(c)
    kw = psc.params(c) if limit is None else dict(psc.params(c), episode_limit=limit)
    pb = mapfx_mod.MarlPartialBatch(np.array(b["starts"]), np.array(b["goals"]), grids=np.array(b["grids"]), **kw)
    assert psc.kernel_args(_abi.last_kernel()) == psc.expected_bfs_kernel(c), _abi.last_kernel()
    acts = torch.zeros((c.T, c.E, c.N), dtype=getattr(torch, c.dtype), device="cuda")
    masked = reset and grc.has_masked_reset(c)
    mask = torch.zeros((c.E,), dtype=torch.uint8, device="cuda")
    masks = grc.reset_masks(c) if masked else None
    calls = [("reset", pb.reset)] if reset else []
    for t in range(c.T):
        if masked and t == c.T // 2:
            calls.append(("masked reset", lambda: pb.reset(mask)))
        calls.append(("step", lambda t=t: pb.step(acts[t])))
    state = {f: getattr(pb, f) for f in psc.STATE_ARRAYS if f != "pnbr" or psc.carries_pnbr(pb)}

    def load(ep):
        acts.copy_(_dev(np.array(ep.actions).astype(c.dtype)))
        if masked:
            mask.copy_(_dev(np.array(masks[ep.name])))

    def check(ep, log, what):
        snaps = ep.snaps if reset else ep.snaps[1:]
        assert len(snaps) == len(log)
        for k, (slot, want) in enumerate(zip(log, snaps)):
            like = types.SimpleNamespace(**dict({"H": c.H, "W": c.W, "N": c.N, "pnbr": None},
                                                **{f: slot[f] for f in state}))
            d = psc.compare(like, slot, want, "%s %d" % (calls[k][0], k))
            assert d is None, (what, d)
        if reset:       # reset() writes no reward (a later slot holds the last step's)
            assert _all_fill(log[0]["reward"]), what

    def after(ep):
        pb.check_err()

    def kernels(seen):
        assert psc.kernel_args(_one(seen, "step")[0]) == psc.expected_step_kernel(c), seen

    return types.SimpleNamespace(batch=pb, acts=acts, calls=calls, state=state, outs=dict(pb.out),
                                 fill=list(pb.out.values()), load=load, check=check, after=after, kernels=kernels)


@pytest.mark.parametrize("c", of_family("partial"), ids=lambda c: case_id("partial", c))
def test_partial_case_replays_as_the_restatement(mapfx_mod, c):
    """[reset, T steps]; the three masked-reset cases [reset, T / 2 steps, reset(env_mask),
    T / 2 steps], the mask a static uint8 tensor whose contents change between the replays:
    all ones (A), the irregular mask (B), all zeros (C)."""
    replay_protocol(_partial_plan(mapfx_mod, c), _eps("partial", c))


def test_partial_state_and_t_carry_across_replays(mapfx_mod):
    """[T steps] without the reset, replayed twice back to back = one 2T-step episode
    (episode_limit 2T - 1)."""
    c, limit, ep = grc.carry_episode("partial")
    plan = _partial_plan(mapfx_mod, c, reset=False, limit=limit)
    load = plan.load

    def load_half(half):
        if half.fresh:
            plan.batch.reset()
        load(half)

    plan.load = load_half
    replay_protocol(plan, _halves(ep, c.T), order=("first", "second"))
    assert np.array_equal(_np(plan.batch.t).astype(np.int64), ep.snaps[-1]["t"])


def _scen_table(lengths, side, seed):
    """A scenario table of len(lengths) files on an open side x side map: a file's lines
    start on distinct cells and end on distinct cells, no line ends where it starts."""
    rng = np.random.default_rng(seed)
    lines = np.zeros((len(lengths), max(lengths), 4), np.int16)
    for f, L in enumerate(lengths):
        s = rng.permutation(side * side)[:L]
        g = rng.permutation(side * side)[:L]
        g = np.where(g == s, np.roll(g, 1), g)
        assert (g != s).all()
        lines[f, :L] = np.stack((s // side, s % side, g // side, g % side), 1)
    return lines, np.array(lengths, np.int32)


def test_partial_scenario_draw_in_the_graph(mapfx_mod):
    """[redraw(), reset(), T steps] after set_scenarios, three replays with no buffer touched
    in between: replay r plays the instance rng.scen_draw names at episode r (every env),
    its goal tables are bfs_goal_dist's, its steps the restatement's under the static
    actions; `episode` reads 3 afterwards.  (Two files of 30 and 8 lines on an 8 x 8 map,
    N = 3, E = 5: the BFS runs inside the graph here.)"""
    import torch
    from mapfx import rng as mrng
    from oracle.partial_oracle import bfs_goal_dist
    E, N, T, side, seed = 5, 3, 6, 8, 21
    lines, n_lines = _scen_table([30, 8], side, seed=6)
    grid = np.zeros((side, side), np.int8)
    c = psc.Case("draw", side, side, "open", N, 5, 5, E, T, True, "int8")
    actions = np.random.default_rng(9).integers(0, 5, size=(T, E, N))
    want = []
    for r in range(3):
        f, ln = mrng.scen_draw(seed, np.arange(E), r, n_lines, N)
        assert (ln >= 0).all()
        rows = lines[f[:, None], ln].astype(np.int32)
        st, gl = np.ascontiguousarray(rows[..., :2]), np.ascontiguousarray(rows[..., 2:])
        gd = np.stack([np.stack([bfs_goal_dist(grid, gl[e, a]) for a in range(N)]) for e in range(E)])
        b = {"grids": grid[None], "starts": st, "goals": gl, "goal_dist": gd}
        want.append(types.SimpleNamespace(name="draw %d" % r, starts=st, goals=gl, goal_dist=gd,
                                          snaps=psc.episode(c, b, actions)))
    assert all(not np.array_equal(want[i].starts, want[j].starts) for i, j in ((0, 1), (0, 2), (1, 2)))
    pb = mapfx_mod.MarlPartialBatch(want[0].starts, want[0].goals, grids=grid[None], **psc.params(c))
    pb.set_scenarios(lines, n_lines, seed=seed)
    acts = _dev(actions.astype(np.int8))
    state = {f: getattr(pb, f) for f in psc.STATE_ARRAYS if f != "pnbr" or psc.carries_pnbr(pb)}
    logged = dict(state, init_pos=pb.init_pos, goal=pb.goal, goal_dist=pb.goal_dist, **pb.out)
    calls = [pb.redraw, pb.reset] + [lambda t=t: pb.step(acts[t]) for t in range(T)]
    log = [{n: torch.empty_like(t) for n, t in logged.items()} for _ in calls]
    cur = torch.cuda.current_stream()

    def run_calls():
        for k, fn in enumerate(calls):
            fn()
            for n, t in logged.items():
                log[k][n].copy_(t)

    def check(w, what):
        gd = _np(log[0]["goal_dist"]).astype(np.int64)
        gd[gd == 255] = -1           # u8 tables: 255 = unreachable
        assert np.array_equal(_np(log[0]["init_pos"]), w.starts) and np.array_equal(_np(log[0]["goal"]), w.goals), what
        assert np.array_equal(gd, w.goal_dist), what
        for k, snap in enumerate(w.snaps):
            slot = log[k + 1]
            like = types.SimpleNamespace(**dict({"H": side, "W": side, "N": N, "pnbr": None},
                                                **{f: slot[f] for f in state}))
            d = psc.compare(like, slot, snap, k)
            assert d is None, (what, d)

    side_stream = torch.cuda.Stream()
    side_stream.wait_stream(cur)
    with torch.cuda.stream(side_stream):
        run_calls()
    cur.wait_stream(side_stream)
    torch.cuda.synchronize()
    check(want[0], "eager on the side stream")
    assert _np(pb.episode).tolist() == [1] * E
    pb.episode.zero_()
    _fill([t for slot in log for t in slot.values()] + list(pb.out.values()))
    torch.cuda.synchronize()
    before = {n: t.clone() for n, t in dict(state, episode=pb.episode, goal_dist=pb.goal_dist).items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side_stream):
        run_calls()
    torch.cuda.synchronize()
    for n, t in before.items():
        assert torch.equal(getattr(pb, n), t), "%s changed during the capture" % n
    assert all(_all_fill(t) for slot in log for t in slot.values())
    for r in range(3):
        graph.replay()
        torch.cuda.synchronize()
        check(want[r], "replay %d" % r)
    assert _np(pb.episode).tolist() == [3] * E
    pb.check_err()
    del graph, side_stream


# ------------------------------------------------------------------ PRIMAL
def _primal_plan(mapfx_mod, c):
    import torch
    from mapfx import _abi
    b = qsc.build(c)
    pb = mapfx_mod.PrimalBatch(np.array(b["starts"]), np.array(b["goals"]), grids=b["grids"],
                               observation_size=c.s, diagonal=c.diag)
    ids = torch.ones((c.E, c.K), dtype=torch.int32, device="cuda")
    acts = torch.zeros((c.E, c.K), dtype=torch.int32, device="cuda")
    starts = _dev(np.array(b["starts"]))
    pb.act(ids, acts)               # (K stays: the wrapper allocates its [E, K] outputs here)
    state = {"pos": pb.pos}
    if c.diag:
        state["past"] = pb.past

    def load(ep):
        ids.copy_(_dev(np.array(ep.ids)))
        acts.copy_(_dev(np.array(ep.actions)))
        for t in state.values():
            t.copy_(starts)

    def check(ep, log, what):
        got = {k: _np(log[0][k]) for k in qsc.FIELDS}
        got["pos"] = _np(log[0]["pos"])
        got["past"] = _np(log[0]["past"]) if c.diag else None
        want = {k: ep.snaps[k] for k in qsc.FIELDS}
        want["pos"], want["past"] = ep.snaps["pos"], ep.snaps["past"]
        d = qsc.compare(got, want)
        assert d is None, (what, d)

    def kernels(seen):
        name = _one(seen, "act")[0]
        assert c.kernel in name, name
        assert qsc.expected_kernel(c.H, c.W, c.N, c.s, c.E, c.diag, c.lanes, c.path, True) in name, name

    return types.SimpleNamespace(batch=pb, calls=[("act", lambda: pb.act(ids, acts))], state=state,
                                 outs={k: pb.out[k] for k in qsc.FIELDS}, fill=[pb.out[k] for k in qsc.FIELDS],
                                 load=load, check=check, after=lambda ep: pb.check_err(), kernels=kernels)


@pytest.mark.parametrize("c", of_family("primal"), ids=lambda c: case_id("primal", c))
def test_primal_case_replays_as_the_restatement(mapfx_mod, monkeypatch, c):
    """[act(ids, acts)] on static int32 [E, K] ids and actions; PRIMAL has no reset, so pos
    (and past) are put back to the starts in place before every pass."""
    monkeypatch.setenv("MAPFX_PRIMAL_LANES", c.lanes)
    monkeypatch.setenv("MAPFX_PRIMAL_PATH", c.path)
    replay_protocol(_primal_plan(mapfx_mod, c), _eps("primal", c))


@pytest.mark.parametrize("diag,observe", [(False, ""), (True, ""), (False, "waves"), (False, "lanes")],
                         ids=["plain", "diagonal", "observe-waves", "observe-lanes"])
def test_primal_generator_in_the_graph(mapfx_mod, monkeypatch, diag, observe):
    """[regenerate(), act(ids, acts), observe()] on a PrimalBatch.random batch (E = 9,
    12 x 13, N = 5, s = 4, K = 20), three replays with no buffer touched in between: replay
    r plays the worlds primal_gen_ref draws at episode r, the calls PrimalWorld's, the
    queries primal_obs's.  `episode` is a device counter: it reads 3 afterwards."""
    import torch
    import primal_gen_ref as ref
    from mapfx.maps import primal_gen_luts
    from oracle.mapf_oracle import primal_obs
    from oracle.primal_dyn_oracle import PrimalWorld
    monkeypatch.setenv("MAPFX_PRIMAL_OBSERVE", observe)
    E, H, W, N, s, K, seed = 9, 12, 13, 5, 4, 20, 77
    SIZE, PROB = (5, 12), (0, .4)
    luts = primal_gen_luts(SIZE, PROB)
    nact = 9 if diag else 5
    rng = np.random.default_rng(31 + diag)
    ids_h = rng.integers(1, N + 1, size=(E, K)).astype(np.int32)
    acts_h = rng.integers(0, nact, size=(E, K)).astype(np.int32)
    pb = mapfx_mod.PrimalBatch.random(E, N, (H, W), seed=seed, SIZE=SIZE, PROB=PROB, observation_size=s,
                                      diagonal=diag)
    ids, acts = _dev(ids_h), _dev(acts_h)
    pb.act(ids, acts)
    pb.observe()                    # (both allocate their output buffers at the first call)
    state = {"pos": pb.pos, "goal": pb.goal, "bits": pb.bits, "episode": pb.episode}
    if diag:
        state["past"] = pb.past
    logged = [dict(state), dict(state, **{"act_" + k: pb.out[k] for k in qsc.FIELDS}),
              dict(state, **{"obs_" + k: v for k, v in pb.obs_out.items()})]
    calls = [pb.regenerate, lambda: pb.act(ids, acts), pb.observe]
    log = [{n: torch.empty_like(t) for n, t in src.items()} for src in logged]
    outs = [pb.out[k] for k in qsc.FIELDS] + list(pb.obs_out.values())

    def run_calls():
        for k, fn in enumerate(calls):
            fn()
            for n, t in logged[k].items():
                log[k][n].copy_(t)

    want = {"bits": np.zeros((E, ref.stride(H, W)), np.uint8), "pos": np.zeros((E, N, 2), np.int32),
            "goal": np.zeros((E, N, 2), np.int32), "past": np.zeros((E, N, 2), np.int32) if diag else None,
            "episode": np.zeros(E, np.int32)}

    def check(r, what):
        want["episode"][:] = r
        assert ref.generate(want, seed, 0, N, H, W, luts) == []
        for k in ("bits", "pos", "goal", "episode") + (("past",) if diag else ()):
            assert np.array_equal(_np(log[0][k]), want[k]), (what, k)
        got = {k: _np(log[1]["act_" + k]) for k in qsc.FIELDS}
        q = {k: _np(log[2]["obs_" + k]) for k in pb.obs_out}
        for e in range(E):
            w = PrimalWorld(-ref.unpack(want["bits"][e], H, W).astype(np.int64), want["pos"][e], want["goal"][e],
                            s, diagonal=diag)
            for k in range(K):
                maps, vec, rew, done, mask, on_goal, _, valid = w.step(int(ids_h[e, k]) - 1, int(acts_h[e, k]))
                assert np.float64(rew).view(np.uint64) == got["reward"][e, k].view(np.uint64), (what, e, k)
                assert (done, mask, on_goal, valid) == (bool(got["done"][e, k]), int(got["next_mask"][e, k]),
                                                        bool(got["on_goal"][e, k]), bool(got["valid"][e, k])), (what, e, k)
                assert np.array_equal(maps, got["obs"][e, k]), (what, e, k)
                assert np.array_equal(np.asarray(vec, np.float64).view(np.uint64),
                                      got["vec"][e, k].view(np.uint64)), (what, e, k)
            assert np.array_equal(_np(log[1]["pos"])[e], np.array(w.pos, np.int32)), (what, e)
            for a in range(N):
                maps, vec = primal_obs(w._world_grid(), w.pos, w.goals, s, agents=[a])
                assert np.array_equal(maps[a], q["obs"][e, a]), (what, e, a)
                assert np.array_equal(vec[a].view(np.uint64), q["vec"][e, a].view(np.uint64)), (what, e, a)
                assert w.next_mask(a, 0) == int(q["next_mask"][e, a]), (what, e, a)
                assert (w.pos[a] == w.goals[a]) == bool(q["on_goal"][e, a]), (what, e, a)
                assert w.done() == bool(q["done"][e, a]), (what, e, a)
        return want["pos"].copy()

    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    pb.episode.zero_()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        run_calls()
    cur.wait_stream(side)
    torch.cuda.synchronize()
    check(0, "eager on the side stream")
    pb.episode.zero_()
    _fill([t for slot in log for t in slot.values()] + outs)
    torch.cuda.synchronize()
    before = {n: t.clone() for n, t in state.items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run_calls()
    torch.cuda.synchronize()
    for n, t in state.items():
        assert torch.equal(t, before[n]), "%s changed during the capture" % n
    assert all(_all_fill(t) for slot in log for t in slot.values()) and all(_all_fill(t) for t in outs)
    starts = []
    for r in range(3):
        graph.replay()
        torch.cuda.synchronize()
        starts.append(check(r, "replay %d" % r))
    assert all(not np.array_equal(starts[i], starts[j]) for i, j in ((0, 1), (0, 2), (1, 2)))
    assert _np(pb.episode).tolist() == [3] * E
    pb.check_err()
    del graph, side


@pytest.mark.parametrize("path", ["", "flat"])
def test_primal_blocking_in_the_graph(mapfx_mod, monkeypatch, path):
    """[act] with blocking=True (the step launch and the blocking pass behind it) on the
    14 x 14 rooms worlds of tests/test_gpu_primal_blocking.py cut to E = 9 and K = 20, two
    call scripts through static ids / acts, against the blocking restatement."""
    import torch
    from primal_blocking_ref import BlockingWorld, rooms_script, rooms_world
    monkeypatch.setenv("MAPFX_PRIMAL_BLOCKING", path)
    E, N, K, H, W, s = 9, 12, 20, 14, 14, 10
    rng = np.random.default_rng(2024)
    grids, starts, goals, scripts = [], [], [], ([], [])
    for e in range(E):
        g, st, gl, da = rooms_world(rng, H, W, N, 5)
        grids.append(g), starts.append(st), goals.append(gl)
        for sc in scripts:
            sc.append(rooms_script(rng, N, da, 6, 5)[:K])
    grids, starts, goals = np.stack(grids), np.array(starts, np.int32), np.array(goals, np.int32)
    eps = {}
    for name, sc in zip(("one", "two"), scripts):
        i = np.array([[c[0] for c in calls] for calls in sc], np.int32)
        a = np.array([[c[1] for c in calls] for calls in sc], np.int32)
        want = {k: np.zeros((E, K), dt) for k, dt in (("reward", np.float64), ("blocking", np.uint8),
                                                       ("n_blocking", np.int32), ("on_goal", np.uint8),
                                                       ("valid", np.uint8))}
        pos = np.zeros((E, N, 2), np.int32)
        for e in range(E):
            w = BlockingWorld(grids[e], starts[e], goals[e], size=s, diagonal=False)
            for k in range(K):
                _, _, r, _, _, on_goal, blocking, valid = w.step(int(i[e, k]) - 1, int(a[e, k]))
                want["reward"][e, k], want["blocking"][e, k], want["n_blocking"][e, k] = r, blocking, w.last_n
                want["on_goal"][e, k], want["valid"][e, k] = on_goal, valid
            pos[e] = np.array(w.pos, np.int32)
        stays = (a == 0) & (want["on_goal"] != 0)
        assert (want["n_blocking"][stays] > 0).any(), "%s: no penalised stay" % name
        eps[name] = types.SimpleNamespace(name=name, ids=i, actions=a, want=want, pos=pos)
    assert not np.array_equal(eps["one"].actions, eps["two"].actions)
    assert all(not np.array_equal(eps["one"].want[k], eps["two"].want[k]) for k in ("reward", "n_blocking"))
    assert not np.array_equal(eps["one"].pos, eps["two"].pos)
    pb = mapfx_mod.PrimalBatch(starts, goals, grids=grids, observation_size=s, blocking=True)
    ids = torch.ones((E, K), dtype=torch.int32, device="cuda")
    acts = torch.zeros((E, K), dtype=torch.int32, device="cuda")
    pb.act(ids, acts)
    d_starts = _dev(starts)
    keys = ("reward", "blocking", "n_blocking", "on_goal", "valid")

    def load(ep):
        ids.copy_(_dev(ep.ids))
        acts.copy_(_dev(ep.actions))
        pb.pos.copy_(d_starts)

    def check(ep, log, what):
        for k in keys:
            g, w = _np(log[0][k]), ep.want[k]
            if k == "reward":
                g, w = g.view(np.uint64), w.view(np.uint64)
            assert np.array_equal(g, w), (what, k, np.argwhere(g != w)[:4].tolist())
        assert np.array_equal(_np(log[0]["pos"]), ep.pos), what

    plan = types.SimpleNamespace(batch=pb, calls=[("act", lambda: pb.act(ids, acts))], state={"pos": pb.pos},
                                 outs={k: pb.out[k] for k in keys}, fill=[pb.out[k] for k in keys], load=load,
                                 check=check, after=lambda ep: pb.check_err(), kernels=lambda seen: None)
    replay_protocol(plan, eps, order=("one", "two", "one"))


# ------------------------------------------------------------------ the runner
def test_runner_on_a_side_stream(tmp_path):
    """BatchedRunner.run() cannot be captured: it waits on its ring events (a host wait on
    work of the stream being captured).  It runs here eagerly inside
    `with torch.cuda.stream(side)`, the ring events recorded on that stream, through the
    comparison of tests/test_gpu_runner_shapes.py against RefRunner, on the smallest case of
    its matrix (B * N * H * W; every case has envs that end at different steps)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from test_gpu_runner_shapes import CASES as RUNNER_CASES, _check as runner_check
    name = min(RUNNER_CASES, key=lambda n: (RUNNER_CASES[n]["B"] * RUNNER_CASES[n]["N"]
                                            * len(RUNNER_CASES[n]["grid"]) * len(RUNNER_CASES[n]["grid"][0])))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runner_check(tmp_path, name)
        assert torch.cuda.current_stream() == side
    side.synchronize()
    torch.cuda.synchronize()
    del side
