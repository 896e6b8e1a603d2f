"""mapfx_primal_act at every kernel instance, on worlds that finish, and at its edges.

The cases, their goal-seeking call scripts and the expected outputs come from
tests/primal_step_cases.py (the CPU restatement, oracle/primal_dyn_oracle.py);
tests/test_primal_step_cases.py holds what those scripts cover.  Every case compares every
output of every call of every world bit-exactly (rewards and goal vectors as fp64 bit
patterns), pos / past after the launch, and asserts the instance it reached from
mapfx_last_kernel: 8 of 8 primal_seq_kernel<S, DIAG> and 24 of 24
primal_act_kernel<S, LS, DIAG, MA>.

The C-ABI tests at the end run on the test's own buffers: every output is a view into a
larger tensor filled with 0xA5, 256 guard bytes each side, so an element the kernel does
not write, a write past a world's records and the untouched tail of a stopped world show.
The guards find stray writes after the fact; no case here leaves the ABI's limits.
"""
import ctypes

import numpy as np
import pytest

from primal_step_cases import CASES, FIELDS, build, case_id, compare, expected_kernel

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5
MAPFX_EINVAL = -1   # include/mapfx.h


@pytest.fixture(scope="module")
def mapfx_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mapfx
    return mapfx


def _np(t):
    return t.detach().cpu().numpy()


def _pin(monkeypatch, c):
    monkeypatch.setenv("MAPFX_PRIMAL_LANES", c.lanes)
    monkeypatch.setenv("MAPFX_PRIMAL_PATH", c.path)


def _want(b, sl=slice(None)):
    return {k: b[k][:, sl] for k in FIELDS}


# ------------------------------------------------- a) - e): PrimalBatch, every instance
@pytest.mark.parametrize("c", [c for c in CASES if not c.name.startswith("abi-")], ids=case_id)
def test_step_case_matches_restatement(mapfx_mod, monkeypatch, c):
    from mapfx import _abi
    _pin(monkeypatch, c)
    b = build(c)
    pb = mapfx_mod.PrimalBatch(np.array(b["starts"]), np.array(b["goals"]), grids=b["grids"],
                               observation_size=c.s, diagonal=c.diag)
    o = pb.act(np.array(b["ids"]), np.array(b["actions"]))
    kernel = _abi.last_kernel()
    assert expected_kernel(c.H, c.W, c.N, c.s, c.E, c.diag, c.lanes, c.path, True) in kernel, kernel
    assert c.kernel in kernel, kernel
    got = {k: _np(o[k]) for k in FIELDS}
    got["pos"] = _np(pb.pos)
    got["past"] = _np(pb.past) if c.diag else None
    pb.check_err()
    want = _want(b)
    want["pos"], want["past"] = b["pos"], b["past"]
    d = compare(got, want)
    assert d is None, d


def test_world_past_the_lds_limit_is_refused_at_create(mapfx_mod):
    """1 x 16384 at s = 32: 33 padded rows of 16416 bytes, past the 160 KB of LDS a
    workgroup can have.  Refused with a message before anything is launched."""
    from mapfx import _abi
    before = _abi.last_kernel()
    g = np.zeros((1, 1, 16384), np.int8)
    with pytest.raises(_abi.MapfxError, match="too much LDS"):
        mapfx_mod.PrimalBatch([[[0, 0], [0, 9]]], [[[0, 5], [0, 20]]], grids=g, observation_size=32)
    assert _abi.last_kernel() == before


# ------------------------------------------------- f) the C ABI on the test's own buffers
ABI_CASES = [c for c in CASES if c.name.startswith("abi-")]


class _Handle:
    """mapfx_primal_create + the state tensors of a case, through mapfx._abi alone."""

    def __init__(self, c, b):
        import torch
        from mapfx import _abi
        from mapfx.maps import pack_bits
        self.abi, self.torch, self.c = _abi, torch, c
        cfg = _abi.QCfg(H=c.H, W=c.W, n_agents=c.N, n_envs=c.E, obs_size=c.s, map_shared=0,
                        diagonal=1 if c.diag else 0)
        self.h = ctypes.c_void_p()
        _abi.check(_abi.lib.mapfx_primal_create(ctypes.byref(cfg), ctypes.byref(self.h)), "create")
        dev = "cuda"
        self.pos = torch.as_tensor(np.array(b["starts"])).to(dev).contiguous()
        self.goal = torch.as_tensor(np.array(b["goals"])).to(dev).contiguous()
        self.past = self.pos.clone() if c.diag else None
        self.bits = torch.as_tensor(np.array(pack_bits(b["grids"] < 0), dtype=np.uint8)).to(dev).contiguous()
        self.err = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.state = _abi.QState(pos=_abi.ptr(self.pos), goal=_abi.ptr(self.goal),
                                 map_bits=_abi.ptr(self.bits), past=_abi.ptr(self.past))

    def close(self):
        if self.h.value:
            self.abi.lib.mapfx_primal_destroy(self.h)
            self.h = ctypes.c_void_p()

    def buffers(self, K, produce=FIELDS, obs_shift=0):
        """One 0xA5-filled uint8 tensor per output: guard, [E][K] elements, guard.  The
        obs elements start 16-byte aligned, plus obs_shift."""
        c, torch = self.c, self.torch
        item = {"reward": 8, "done": 1, "next_mask": 2 if c.diag else 1, "on_goal": 1, "valid": 1,
                "obs": 4 * c.s * c.s, "vec": 24}
        raw, off = {}, {}
        for k in produce:
            n = c.E * K * item[k]
            raw[k] = torch.full((GUARD + n + GUARD + 16,), FILL, dtype=torch.uint8, device="cuda")
            off[k] = GUARD + (obs_shift if k == "obs" else 0)
            assert raw[k].data_ptr() % 16 == 0
        return {"raw": raw, "off": off, "item": item, "K": K}

    def qout(self, buf, err=True):
        p = {k: buf["raw"][k].data_ptr() + buf["off"][k] for k in buf["raw"]}
        return self.abi.QOut(err=self.abi.ptr(self.err) if err else None, **p)

    def act(self, ids, acts, out):
        torch, abi = self.torch, self.abi
        ids = torch.as_tensor(np.array(ids, dtype=np.int32, order="C")).cuda()     # (copies: the
        acts = torch.as_tensor(np.array(acts, dtype=np.int32, order="C")).cuda()   # cases are read-only)
        rc = abi.lib.mapfx_primal_act(self.h, ctypes.byref(self.state), abi.ptr(ids), abi.ptr(acts),
                                      int(ids.shape[1]), ctypes.byref(out) if out is not None else None,
                                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    def read(self, buf):
        """The guards are intact; returns {field: [E, K, ...] array} and, per field, the
        [E, K] mask of elements that still hold the fill in every byte."""
        c, K = self.c, buf["K"]
        dt = {"reward": np.float64, "vec": np.float64, "next_mask": np.int16 if c.diag else np.uint8}
        shape = {"obs": (c.E, K, 4, c.s, c.s), "vec": (c.E, K, 3)}
        got, untouched = {}, {}
        for k, t in buf["raw"].items():
            a = _np(t)
            o, n = buf["off"][k], c.E * K * buf["item"][k]
            assert (a[:o] == FILL).all(), "%s: a write before the first element" % k
            assert (a[o + n:] == FILL).all(), "%s: a write past the last element" % k
            body = a[o:o + n].copy()
            got[k] = body.view(dt.get(k, np.uint8)).reshape(shape.get(k, (c.E, K)))
            untouched[k] = (body.reshape(c.E, K, -1) == FILL).all(-1)
        return got, untouched

    def state_now(self):
        return {"pos": _np(self.pos), "past": _np(self.past) if self.c.diag else None}


@pytest.fixture
def handle(mapfx_mod, monkeypatch, request):
    c = request.param
    _pin(monkeypatch, c)
    h = _Handle(c, build(c))
    yield h
    h.close()


def _abi_param(cases):
    return pytest.mark.parametrize("handle", cases, ids=case_id, indirect=True)


@_abi_param(ABI_CASES)
def test_abi_guard_bands_and_every_element_written(handle):
    c, b = handle.c, build(handle.c)
    buf = handle.buffers(c.K)
    assert handle.act(b["ids"], b["actions"], handle.qout(buf)) == 0
    assert c.kernel in handle.abi.last_kernel(), handle.abi.last_kernel()
    got, _ = handle.read(buf)
    got.update(handle.state_now())
    want = _want(b)
    want["pos"], want["past"] = b["pos"], b["past"]
    d = compare(got, want)
    assert d is None, d
    assert int(_np(handle.err)[0]) == 0


@_abi_param(ABI_CASES)
def test_abi_bad_call_stops_its_world_and_writes_nothing_more(handle):
    """A bad call at k = 70 of 130 (an agent id past N; action 9 with DIAGONAL_MOVEMENT)
    in world 4: its elements from k = 70 on keep the caller's bytes in every output, its
    pos / past are the state after 70 calls, err names it, the other worlds are complete."""
    c, b = handle.c, build(handle.c)
    bad, kbad = 4, 70
    ids, acts = np.array(b["ids"]), np.array(b["actions"])
    if c.diag:
        acts[bad, kbad] = 9
    else:
        ids[bad, kbad] = c.N + 1
    buf = handle.buffers(c.K)
    assert handle.act(ids, acts, handle.qout(buf)) == 0
    assert c.kernel in handle.abi.last_kernel()
    got, untouched = handle.read(buf)
    assert int(_np(handle.err)[0]) == bad + 1
    for k, u in untouched.items():
        assert u[bad, kbad:].all(), "%s: written after the bad call" % k
    upto = np.full(c.E, c.K)
    upto[bad] = kbad
    want = _want(b)
    want["pos"], want["past"] = np.array(b["pos"]), np.array(b["past"])
    want["pos"][bad], want["past"][bad] = b["pos_at"][bad, kbad - 1], b["past_at"][bad, kbad - 1]
    got.update(handle.state_now())
    d = compare(got, want, upto)
    assert d is None, d


@_abi_param([c for c in ABI_CASES if c.name == "abi-seq10"])
def test_abi_obs_not_16_byte_aligned_takes_the_lane_group_kernel(handle):
    """obs 4 bytes past a 16-byte boundary: the production fallback of the seq kernel."""
    c, b = handle.c, build(handle.c)
    buf = handle.buffers(c.K, obs_shift=4)
    out = handle.qout(buf)
    assert out.obs % 16 == 4
    assert handle.act(b["ids"], b["actions"], out) == 0
    name = expected_kernel(c.H, c.W, c.N, c.s, c.E, c.diag, c.lanes, c.path, obs_aligned=False)
    assert name == "primal_act_kernel<10, 6, false, 1>" and name in handle.abi.last_kernel()
    got, _ = handle.read(buf)
    got.update(handle.state_now())
    want = _want(b)
    want["pos"], want["past"] = b["pos"], b["past"]
    d = compare(got, want)
    assert d is None, d


@_abi_param([c for c in ABI_CASES if c.name == "abi-seq10"])
def test_abi_obs_not_4_byte_aligned_is_refused(handle):
    """MAPFX_EINVAL, as mapfx_primal_observe: nothing is launched, nothing is written."""
    c, b = handle.c, build(handle.c)
    before = handle.abi.last_kernel()
    for shift in (1, 2, 3):
        buf = handle.buffers(c.K, obs_shift=shift)
        assert handle.act(b["ids"], b["actions"], handle.qout(buf)) == MAPFX_EINVAL
        assert b"4-byte aligned" in handle.abi.lib.mapfx_last_error()
        _, untouched = handle.read(buf)
        assert all(u.all() for u in untouched.values())
    assert handle.abi.last_kernel() == before
    assert np.array_equal(_np(handle.pos), b["starts"])


@_abi_param(ABI_CASES)
@pytest.mark.parametrize("produce", ["no-obs", "obs-only", "no-out"])
def test_abi_null_outputs(handle, produce):
    c, b = handle.c, build(handle.c)
    fields = {"no-obs": tuple(f for f in FIELDS if f != "obs"), "obs-only": ("obs",), "no-out": ()}[produce]
    buf = handle.buffers(c.K, produce=fields)
    out = handle.qout(buf, err=produce != "obs-only") if fields else None
    assert handle.act(b["ids"], b["actions"], out) == 0
    assert c.kernel in handle.abi.last_kernel()
    got, _ = handle.read(buf)
    assert sorted(got) == sorted(fields)
    got.update(handle.state_now())
    want = _want(b)
    want["pos"], want["past"] = b["pos"], b["past"]
    d = compare(got, want)
    assert d is None, d


@_abi_param(ABI_CASES)
def test_abi_chunked_launches_carry_the_world_over(handle):
    """The 130 calls as launches of 1, 63, 64 and 2 on one handle: each launch recounts
    the agents on their goals from pos, so `done` goes on where the last launch left it."""
    c, b = handle.c, build(handle.c)
    k0 = 0
    for n in (1, 63, 64, 2):
        sl = slice(k0, k0 + n)
        buf = handle.buffers(n)
        assert handle.act(b["ids"][:, sl], b["actions"][:, sl], handle.qout(buf)) == 0
        assert c.kernel in handle.abi.last_kernel()
        got, _ = handle.read(buf)
        got.update(handle.state_now())
        want = _want(b, sl)
        want["pos"], want["past"] = b["pos_at"][:, k0 + n - 1], b["past_at"][:, k0 + n - 1]
        d = compare(got, want)
        assert d is None, (k0, d)
        k0 += n
    assert k0 == c.K and int(_np(handle.err)[0]) == 0
