"""The plain MARL_PARTIAL path -- mapfx_partial_goal_dist / _reset / _step / _observe of
csrc/partial.hip through MarlPartialBatch -- at every kernel instance its host dispatch can
pick, bit-exactly against the restatement (oracle/partial_oracle.py, pinned to the reference
by the mp_* goldens).  The cases, their scripted episodes and the expected values come from
tests/partial_step_cases.py; tests/test_partial_step_cases.py holds what they cover.

Every case: the BFS instance named by mapfx_last_kernel right after construction and the
goal tables cell for cell; then reset() and T steps, each call with obs / state / avail /
reward pre-filled with 0xA5 (an element the launch does not write fails) and followed by
`compare`: reward bits, every state array, obs / state / avail, the carried pdist and the
on-grid entries of pnbr; the step instance named by mapfx_last_kernel.  Over the table: 39
of 39 step instances (15 fast plain, 6 generic, 18 workgroup) and 7 of 7 BFS instances.

The reference raises on non-square maps (MARL_PARTIAL_ENV.__create_grid), and most cases
are non-square -- a square map hides every H / W mix-up of the padded LDS image and of the
neighbour-distance reads: those cases pin the kernels to the restatement's semantics only,
as tests/test_gpu_partial_full_range.py says of the shipped non-square maps.

Then, on one fast, one generic and one workgroup case: the three action dtypes from rows of
one tensor whose row bases take every residue mod 8, reset(env_mask) mid-episode,
observe(), and the error word for actions outside 0..4.
"""
import numpy as np
import pytest

from partial_step_cases import (ALL_BFS_KERNELS, ALL_STEP_KERNELS, BY_NAME, CASES, build, case_id,
                                compare, expected_bfs_kernel, expected_step_kernel, kernel_args,
                                make_refs, params, state_arrays)

pytestmark = pytest.mark.gpu

FILL = 0xA5
FAMILIES = ("act-fast", "act-gen", "act-wg")
SEEN_STEP, SEEN_BFS = {}, {}


@pytest.fixture(scope="module")
def mapfx_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mapfx
    return mapfx


def _np(t):
    return t.detach().cpu().numpy()


def _batch(mapfx_mod, c, b):
    return mapfx_mod.MarlPartialBatch(np.array(b["starts"]), np.array(b["goals"]), grids=np.array(b["grids"]),
                                      **params(c))


def _fill(pb):
    import torch
    for v in pb.out.values():
        v.view(torch.uint8).fill_(FILL)


def _reward_kept_fill(pb):
    import torch
    return bool((pb.out["reward"].view(torch.uint8) == FILL).all())


def _device_actions(c, b, dtype=None):
    """[T + 1, E, N] on the device, row t + 1 = the actions of step t; row 0 holds 7s."""
    import torch
    a = np.concatenate([np.full((1, c.E, c.N), 7), b["actions"]]).astype(dtype or c.dtype)
    return torch.as_tensor(a).cuda()


def _same_state(before, after):
    return [f for f in before if not np.array_equal(before[f], after[f])]


# ------------------------------------------------------------------ every instance
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case_matches_restatement(mapfx_mod, c):
    import torch
    from mapfx import _abi
    b = build(c)
    pb = _batch(mapfx_mod, c, b)
    bfs = _abi.last_kernel()
    assert kernel_args(bfs) == expected_bfs_kernel(c), bfs
    SEEN_BFS[c.name] = kernel_args(bfs)
    gd = _np(pb.goal_dist).astype(np.int64)
    if pb.goal_dist.dtype == torch.uint8:
        gd[gd == 255] = -1
    diff = np.argwhere(gd != b["goal_dist"])
    assert len(diff) == 0, "goal_dist (env, agent, cell) %s" % diff[:4].tolist()
    _fill(pb)
    out = pb.reset()
    d = compare(pb, out, b["snaps"][0], "reset")
    assert d is None, d
    assert _reward_kept_fill(pb)
    acts = _device_actions(c, b)
    assert (acts.data_ptr() + acts[1].numel() * acts.element_size()) == acts[1].data_ptr()
    for t in range(c.T):
        _fill(pb)
        out = pb.step(acts[t + 1])
        if t == 0:
            step = _abi.last_kernel()
            assert kernel_args(step) == expected_step_kernel(c), step
            SEEN_STEP[c.name] = kernel_args(step)
        d = compare(pb, out, b["snaps"][t + 1], t)
        assert d is None, d
    pb.check_err()


def test_instances_launched_are_the_full_sets():
    """By name: what the cases above launched (all of them when the whole module ran)."""
    assert len(ALL_STEP_KERNELS) == 39 and len(ALL_BFS_KERNELS) == 7
    assert set(SEEN_STEP.values()) <= ALL_STEP_KERNELS and set(SEEN_BFS.values()) <= ALL_BFS_KERNELS
    if len(SEEN_STEP) == len(CASES):
        assert set(SEEN_STEP.values()) == ALL_STEP_KERNELS
        assert set(SEEN_BFS.values()) == ALL_BFS_KERNELS


# ------------------------------------------------------------------ action dtypes
@pytest.mark.parametrize("dtype", ["int8", "int32", "int64"])
@pytest.mark.parametrize("name", FAMILIES)
def test_action_dtypes_at_every_row_alignment(mapfx_mod, name, dtype):
    """Row t + 1 of one [T + 1, E, N] tensor with E * N odd and T = 8: the int8 row bases
    take every residue mod 8, the int32 rows alternate 0 and 4 (the wave kernel fetches an
    action with one aligned 8-byte load and shifts)."""
    c = BY_NAME[name]
    b = build(c)
    assert (c.E * c.N) % 2 == 1 and c.T == 8
    acts = _device_actions(c, b, dtype)
    size = acts.element_size()
    residues = {(acts[t + 1].data_ptr() - acts.data_ptr()) % 8 for t in range(c.T)}
    assert residues == {1: set(range(8)), 4: {0, 4}, 8: {0}}[size]
    pb = _batch(mapfx_mod, c, b)
    pb.reset()
    for t in range(c.T):
        _fill(pb)
        out = pb.step(acts[t + 1])
        d = compare(pb, out, b["snaps"][t + 1], t)
        assert d is None, d
    pb.check_err()


# ------------------------------------------------------------------ reset(env_mask)
@pytest.mark.parametrize("name", FAMILIES)
def test_masked_reset_mid_episode(mapfx_mod, name):
    c = BY_NAME[name]
    b = build(c)
    refs = make_refs(c, b)
    pb = _batch(mapfx_mod, c, b)
    acts = _device_actions(c, b)
    pb.reset()
    for t in range(2):      # env 1 has completed (t = 2 < limit), the others run
        pb.step(acts[t + 1])
        for e, r in enumerate(refs):
            r.step(b["actions"][t, e])
    assert refs[1].terminated and not refs[0].terminated and not refs[c.E - 1].terminated
    mask = np.zeros(c.E, bool)
    mask[[0, 1, c.E - 1]] = True
    mask[5::7] = True
    assert not mask.all() and mask[0] and mask[-1]
    before = state_arrays(pb)
    for e in np.flatnonzero(mask):
        refs[e].reset()
    for r in refs:
        r.last_reward = None
    _fill(pb)
    out = pb.reset(mask)
    d = compare(pb, out, refs, "masked reset")      # every env's observations are written
    assert d is None, d
    assert _reward_kept_fill(pb)
    after = state_arrays(pb)
    for f in before:        # an unmasked env keeps every state array, pdist included
        assert np.array_equal(before[f][~mask], after[f][~mask]), f
    fresh = build(c)["snaps"][0]
    for f in ("pos", "steps", "at_goal", "done", "goal_cost", "node", "edge", "t", "terminated",
              "total_coll", "pdist"):
        assert np.array_equal(after[f][mask].astype(np.int64), fresh[f][mask]), f
    for t in range(2, 5):
        _fill(pb)
        out = pb.step(acts[t + 1])
        for e, r in enumerate(refs):
            r.step(b["actions"][t, e])
        d = compare(pb, out, refs, t)
        assert d is None, d
    pb.check_err()


# ------------------------------------------------------------------ observe()
@pytest.mark.parametrize("name", FAMILIES)
def test_observe_writes_outputs_and_keeps_the_state(mapfx_mod, name):
    c = BY_NAME[name]
    b = build(c)
    pb = _batch(mapfx_mod, c, b)
    acts = _device_actions(c, b)
    pb.reset()
    for t in range(3):
        pb.step(acts[t + 1])
    before = state_arrays(pb)
    _fill(pb)
    out = pb.observe()
    want = dict(b["snaps"][3], reward_ok=np.zeros(c.E, bool))
    d = compare(pb, out, want, "observe")
    assert d is None, d
    assert _reward_kept_fill(pb)
    assert _same_state(before, state_arrays(pb)) == []
    _fill(pb)
    out = pb.step(acts[4])
    d = compare(pb, out, b["snaps"][4], 3)
    assert d is None, d
    pb.check_err()


# ------------------------------------------------------------------ the error word
BAD = {"int8": (5, -1, 127), "int32": (-2 ** 31, 5, -1), "int64": (2 ** 32 + 2, -1, 5)}


@pytest.mark.parametrize("dtype", ["int8", "int32", "int64"])
@pytest.mark.parametrize("name", FAMILIES)
def test_action_outside_0_4_skips_the_env_and_sets_the_error_word(mapfx_mod, name, dtype):
    """int64 2^32 + 2 has a valid low word under a set high word.  The offending envs keep
    every state array (t included), get reward 0.0 and the observations of the unchanged
    state; err - 1 is one of them (atomicCAS: not necessarily the lowest); check_err()
    raises once and clears the word; the others, and the next step of all, are the
    restatement's."""
    import torch
    c = BY_NAME[name]
    b = build(c)
    refs = make_refs(c, b)
    pb = _batch(mapfx_mod, c, b)
    a = np.array(b["actions"]).astype(np.int64)
    pb.reset()
    pb.step(torch.as_tensor(a[0].astype(dtype)).cuda())
    for e, r in enumerate(refs):
        r.step(a[0, e])
    pb.check_err()
    offenders = (0, c.E // 2, c.E - 1)                  # first, a middle one, last env
    agents = (c.N - 1, 0, c.N // 2)                     # last, first, a middle agent
    step = a[1].copy()
    for e, ag, v in zip(offenders, agents, BAD[dtype]):
        step[e, ag] = v
    dev = torch.as_tensor(step.astype(dtype)).cuda()
    assert [int(dev[e, ag]) for e, ag in zip(offenders, agents)] == list(BAD[dtype])
    before = state_arrays(pb)
    _fill(pb)
    out = pb.step(dev)
    for e, r in enumerate(refs):
        if e in offenders:
            r.refuse()
        else:
            r.step(a[1, e])
    d = compare(pb, out, refs, "bad actions")
    assert d is None, d
    after = state_arrays(pb)
    for f in before:
        assert np.array_equal(before[f][list(offenders)], after[f][list(offenders)]), f
    assert _np(out["reward"])[list(offenders)].view(np.uint64).tolist() == [0, 0, 0]
    assert int(pb.err.item()) - 1 in offenders, int(pb.err.item())
    with pytest.raises(AssertionError, match="invalid action"):
        pb.check_err()
    assert int(pb.err.item()) == 0
    pb.check_err()
    _fill(pb)
    out = pb.step(torch.as_tensor(a[2].astype(dtype)).cuda())
    for e, r in enumerate(refs):
        r.step(a[2, e])
    d = compare(pb, out, refs, 2)
    assert d is None, d
    pb.check_err()
