"""The core MAPF path -- mapfx_observe / mapfx_step / mapfx_rollout of csrc/mapfx.hip through
MapfGridBatch -- at every kernel instance its host dispatch can reach, bit-exactly against
the C oracle (oracle/mapf_oracle.c, pinned to the reference by the goldens).  The cases, their
scripted episodes, the dispatch restatement and the expected values come from
tests/mapf_step_cases.py; tests/test_mapf_step_cases.py holds what they cover.

Every case: mapfx_query against the restated geometry; reset() with the batch's outputs
pre-filled with 0xA5 (an element the launch does not write fails), the observe instance named
by mapfx_last_kernel, `compare` of the state and the observations; then the case's entry
point -- T step() calls, T observe() calls between steps, or ONE rollout launch of T steps
into caller-owned trajectory buffers with 256 guard bytes either side -- with `compare` after
every step (a rollout's slot k against the oracle after its step k, never against step() of
the library), the instance asserted by name, the `err` word, and for rollouts
mapfx_last_action_path.  Over the table: 84 of 84 instances (56 wave, 28 generic), each
asserted by name.

The reference indexes its grid as if it were square, and most cases are non-square -- a
square map hides every H / W / pitch / rows mix-up of the padded LDS image, the two map
builders and the index divisions: those cases pin the kernels to the oracle's semantics
only (tests/test_mapf_step_cases.py checks the C oracle against the Python restatement on
exactly these shapes).
"""
import numpy as np
import pytest

from mapf_step_cases import (ALL_KERNELS, CASES, OBS_KEYS, build, case_geometry, case_id, compare,
                             expected_action_path, expected_kernel, kernel_args, launch_outs, limit_of)

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 256
LEAD = GUARD + 16          # a view starts 16-byte aligned, not 256-byte aligned
SEEN = {}                  # case name -> the instances it launched


@pytest.fixture(scope="module")
def mapfx_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mapfx
    return mapfx


def _np(t):
    return t.detach().cpu().numpy()


def _fill(bufs):
    import torch
    for v in bufs.values():
        v.view(torch.uint8).fill_(FILL)


def _kept_fill(bufs, keys):
    import torch
    return [k for k in keys if not bool((bufs[k].view(torch.uint8) == FILL).all())]


def _state(batch, c):
    s = {"pos": _np(batch.pos), "done": _np(batch.done), "t": _np(batch.t)}
    if c.track:
        s["steps"] = _np(batch.steps)
    return s


def _outputs(bufs, keys, slot=None):
    from mapfx.batch import window_planes
    got = {k: _np(bufs[k] if slot is None else bufs[k][slot]) for k in keys}
    if "obs_window_occ" in keys:
        occ = bufs["obs_window_occ"] if slot is None else bufs["obs_window_occ"][slot]
        got["obs_window_occ_planes"] = _np(window_planes(occ))
    return got


def _device_actions(c, b):
    """[T, E, N] of the case's dtype on the device; int8 with act_off: a view that many bytes
    into a 16-byte aligned allocation."""
    import torch
    a = torch.from_numpy(np.array(b["actions"]).astype(c.act)).cuda()
    if c.act_off:
        raw = torch.zeros(c.act_off + a.numel() + 16, dtype=torch.int8, device="cuda")
        assert raw.data_ptr() % 16 == 0
        view = raw[c.act_off:c.act_off + a.numel()].view(a.shape)
        view.copy_(a)
        a = view
    assert a.is_contiguous() and a.data_ptr() % 16 == c.act_off % 16
    return a


def _check_err(batch, b, steps):
    """The err word after a launch that ran `steps`: 1 + the refused env when the refused
    action is among them, else 0; cleared for the next launch."""
    e = int(batch.err.item())
    want = b["bad"][1] + 1 if b["bad"] is not None and b["bad"][0] in steps else 0
    assert e == want, (e, want)
    batch.err.zero_()


def _guarded(batch, c, keys):
    """{name: (raw uint8 allocation, [T, ...] view at byte LEAD of it)} filled with FILL; the
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


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case_matches_oracle(mapfx_mod, c):
    import torch
    from mapfx import _abi
    b = build(c)
    batch = mapfx_mod.MapfGridBatch(np.array(b["init_pos"]), np.array(b["goals"]), bits=np.array(b["bits"]),
                                    hw=(c.H, c.W), episode_limit=limit_of(c), step_reward=c.rewards[0],
                                    collide_reward=c.rewards[1], obs=c.obs, window=c.window,
                                    primal_size=c.psize, env_offset=c.env_offset, track_steps=c.track)
    assert batch.map_shared == (c.shared and c.E > 1)
    g = case_geometry(c)        # mapfx_query against the restated geometry (lds_bytes: the fold decision)
    assert batch.info() == dict(lanes_per_env=g.L, agents_per_lane=g.apl, envs_per_block=g.EPB,
                                block_threads=g.BT, lds_bytes=g.gen_lds, cell_bytes=g.es, pad=g.P)
    seen = SEEN.setdefault(c.name, set())
    obs_keys = launch_outs(c.obs, "observe")
    other = [k for k in batch.out if k not in OBS_KEYS]
    # ---- reset(): the observe launch
    _fill(batch.out)
    batch.reset()
    seen.add(kernel_args(_abi.last_kernel()))
    assert kernel_args(_abi.last_kernel()) == expected_kernel(c, "observe"), _abi.last_kernel()
    d = compare(dict(_state(batch, c), **_outputs(batch.out, obs_keys)), b["snaps"][0], "reset")
    assert d is None, d
    assert _kept_fill(batch.out, other) == []
    if c.entry != "rollout":
        acts = _device_actions(c, b)
        step_keys = launch_outs(c.obs, "step")
        assert set(step_keys) == set(batch.out)
        for t in range(c.T):
            _fill(batch.out)
            batch.step(acts[t])
            if c.entry == "step":
                seen.add(kernel_args(_abi.last_kernel()))
                assert kernel_args(_abi.last_kernel()) == expected_kernel(c), _abi.last_kernel()
                assert _abi.last_action_path() == 0
            d = compare(dict(_state(batch, c), **_outputs(batch.out, step_keys)), b["snaps"][t + 1], t)
            assert d is None, d
            _check_err(batch, b, (t,))
            if c.entry == "observe":
                _fill(batch.out)
                batch.observe()
                seen.add(kernel_args(_abi.last_kernel()))
                assert kernel_args(_abi.last_kernel()) == expected_kernel(c), _abi.last_kernel()
                d = compare(dict(_state(batch, c), **_outputs(batch.out, obs_keys)), b["snaps"][t + 1],
                            "observe %d" % t)
                assert d is None, d
                assert _kept_fill(batch.out, other) == []
        return
    # ---- one rollout launch into guarded trajectory buffers
    keys = launch_outs(c.obs, "rollout", c.select)
    bufs = _guarded(batch, c, keys)
    traj = {k: v[1] for k, v in bufs.items()}
    acts = None if c.act == "gen" else _device_actions(c, b)
    batch.rollout(c.T, actions=acts, seed=c.seed, t0=c.t0, autoreset=c.autoreset, traj=traj, outputs=keys)
    seen.add(kernel_args(_abi.last_kernel()))
    assert kernel_args(_abi.last_kernel()) == expected_kernel(c), _abi.last_kernel()
    assert _abi.last_action_path() == expected_action_path(c)
    torch.cuda.synchronize()
    _check_err(batch, b, range(c.T))
    for k, (raw, view, lead, nbytes) in bufs.items():
        r = _np(raw)
        assert (r[:lead] == FILL).all(), "%s: bytes before the buffer written" % k
        assert (r[lead + nbytes:] == FILL).all(), "%s: bytes behind the buffer written" % k
    for k in range(c.T):
        d = compare(_outputs(traj, keys, k), b["snaps"][k + 1], k)
        assert d is None, d
    d = compare(_state(batch, c), b["final"], "final state")
    assert d is None, d


def test_instances_launched_are_the_reachable_set(request):
    """By name: what the cases above launched is every instance the dispatch can reach (84:
    56 wave, 28 generic).  Skips itself when only a selection of the cases ran."""
    launched = set().union(*SEEN.values()) if SEEN else set()
    assert launched <= ALL_KERNELS, launched - ALL_KERNELS
    if request.config.getoption("keyword") or len(SEEN) != len(CASES):
        pytest.skip("ran with a selection of the cases (%d of %d): the union is not the full set"
                    % (len(SEEN), len(CASES)))
    assert len(ALL_KERNELS) == 84
    assert launched == ALL_KERNELS, sorted(ALL_KERNELS - launched)
