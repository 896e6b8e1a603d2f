"""The argument handling the three batches share (mapfx._base) and the scenario-line
helpers of mapfx.maps, on tiny host inputs (CPU): E = 2, N = 3, a 4 x 5 grid."""
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN

from mapfx import _base, maps
from mapfx._abi import MAPFX_I8, MAPFX_I32, MAPFX_I64

E, N, H, W = 2, 3, 4, 5
CPU = torch.device("cpu")


def _grids():
    g = np.zeros((E, H, W), dtype=np.int8)
    g[0, 1, 2] = g[0, 3, 4] = g[1, 0, 0] = -1
    return g


def test_parse_map_grids_equal_bits():
    g = _grids()
    h, w, bits, shared = _base.parse_map(g, None, None, E)
    assert (h, w, shared) == (H, W, False)
    assert bits.dtype == np.uint8 and bits.shape == (E, maps.map_stride(H, W))
    assert bits.tobytes() == maps.pack_bits(g).tobytes()
    h2, w2, bits2, shared2 = _base.parse_map(None, maps.pack_bits(g), (H, W), E)
    assert (h2, w2, shared2) == (H, W, False) and bits2.tobytes() == bits.tobytes()
    # a 2-d grid is one map: [1, stride], byte-equal to its 1-d bits
    _, _, b2d, _ = _base.parse_map(g[0], None, None, 1)
    _, _, b1d, _ = _base.parse_map(None, maps.pack_bits(g[0])[0], (H, W), 1)
    assert b2d.shape == (1, maps.map_stride(H, W))
    assert b2d.tobytes() == b1d.tobytes() == bits[0].tobytes()


def test_parse_map_shared_and_stride():
    g = _grids()
    assert _base.parse_map(g[:1], None, None, 2)[3] is True
    assert _base.parse_map(g[:1], None, None, 1)[3] is False
    assert _base.parse_map(g[0], None, None, 2)[3] is True
    good = maps.pack_bits(g)
    with pytest.raises(ValueError, match="bits must be"):
        _base.parse_map(None, good[:, :-1], (H, W), E)
    with pytest.raises(ValueError, match="bits must be"):
        _base.parse_map(None, good, (H, W), E + 1)        # neither 1 nor E maps


def test_parse_map_obstacle_predicates():
    g = np.zeros((1, H, W), dtype=np.int64)
    g[0, 0, 1], g[0, 2, 3] = -1, 2
    nonzero = maps.unpack_bits(_base.parse_map(g, None, None, 1)[2], H, W)
    negative = maps.unpack_bits(_base.parse_map(g, None, None, 1, obstacle=lambda a: a < 0)[2], H, W)
    assert np.array_equal(nonzero != 0, g != 0)
    assert np.array_equal(negative != 0, g < 0)
    assert not np.array_equal(nonzero, negative)


def test_parse_agents():
    a = np.arange(E * N * 2).reshape(E, N, 2)
    e, n, x, y = _base.parse_agents(a.tolist(), a + 1, "starts/goals")
    assert (e, n) == (E, N) and x.dtype == y.dtype == np.int32
    assert np.array_equal(x, a) and np.array_equal(y, a + 1)
    for bad in (a[0], a[..., :1]):
        with pytest.raises(ValueError, match=r"starts/goals must both be \[E, N, 2\]"):
            _base.parse_agents(bad, bad, "starts/goals")
    with pytest.raises(ValueError, match="init_pos/goals"):
        _base.parse_agents(a, a[:1], "init_pos/goals")


ACTION_INPUTS = {
    "int8": (torch.int8, MAPFX_I8), "int32": (torch.int32, MAPFX_I32),
    "int64": (torch.int64, MAPFX_I64), "int16": (torch.int16, MAPFX_I64),
}
VALUES = [[0, 1, 2], [3, 4, 0]]


@pytest.mark.parametrize("name", sorted(ACTION_INPUTS))
def test_as_actions_dtypes(name):
    dt, code = ACTION_INPUTS[name]
    src = torch.tensor(VALUES, dtype=dt)
    a, c = _base.as_actions(src, CPU, (E, N))
    assert c == code and a.is_contiguous() and a.tolist() == VALUES
    assert a.dtype == (torch.int64 if name == "int16" else dt)
    # the fast path: a tensor that needs nothing is returned itself
    assert (a is src) == (name != "int16")
    assert _base.as_actions(src, CPU)[0].tolist() == VALUES       # shape None: not checked


def test_as_actions_list_and_slice():
    a, c = _base.as_actions(VALUES, CPU, (E, N))
    assert c == MAPFX_I64 and a.dtype == torch.int64 and a.tolist() == VALUES
    wide = torch.arange(E * 2 * N, dtype=torch.int32).reshape(E, 2 * N)
    s = wide[:, ::2]
    assert not s.is_contiguous()
    a, c = _base.as_actions(s, CPU, (E, N))
    assert c == MAPFX_I32 and a.is_contiguous() and a is not s and torch.equal(a, s)


@pytest.mark.parametrize("shape", [(E, N + 1), (N, E), (E * N,), (1, E, N)])
def test_as_actions_wrong_shape(shape):
    with pytest.raises(AssertionError, match="actions must be"):
        _base.as_actions(torch.zeros(shape, dtype=torch.int8), CPU, (E, N))


def test_env_mask():
    assert _base.env_mask(None, E, CPU) is None
    m = _base.env_mask(torch.tensor([True, False]), E, CPU)
    assert m.dtype == torch.uint8 and m.tolist() == [1, 0]
    m = _base.env_mask(torch.tensor([256, 0], dtype=torch.int64), E, CPU)
    assert m.dtype == torch.uint8 and m.tolist() == [1, 0]
    assert _base.env_mask([0, 3], E, CPU).tolist() == [0, 1]
    u = torch.tensor([2, 0], dtype=torch.uint8)
    assert _base.env_mask(u, E, CPU) is u
    for n in (E - 1, E + 1):
        with pytest.raises(AssertionError, match=r"mask must be \[E\]"):
            _base.env_mask(torch.ones(n, dtype=torch.uint8), E, CPU)
    with pytest.raises(AssertionError, match=r"mask must be \[E\]"):
        _base.env_mask(torch.ones((E, 1), dtype=torch.bool), E, CPU)


def test_u64():
    assert _base.u64(-1) == 2 ** 64 - 1
    assert _base.u64(2 ** 64 + 5) == 5 and _base.u64(np.int64(7)) == 7


def test_check_on_grid():
    ok = np.array([[[H - 1, W - 1], [0, 0], [H - 1, 0]]], dtype=np.int32)
    _base.check_on_grid(ok, H, W, "starts")
    _base.check_on_grid(ok[:, :0], H, W, "starts")            # no agents: nothing to check
    for r, c in ((H, 0), (0, -1), (-1, 0), (0, W)):
        bad = ok.copy()
        bad[0, 1] = (r, c)
        with pytest.raises(ValueError, match="starts outside the %dx%d grid" % (H, W)):
            _base.check_on_grid(bad, H, W, "starts")


def test_avail_bits():
    m = torch.tensor([[0b10101, 0b00010, 31]], dtype=torch.uint8)
    a = _base.avail_bits(m)
    assert a.dtype == torch.int64 and a.shape == (1, 3, 5)
    assert a.tolist() == [[[1, 0, 1, 0, 1], [0, 1, 0, 0, 0], [1, 1, 1, 1, 1]]]


SCEN_PREFIX = os.path.join(GOLDEN, "scen", "maze-32-32-4-random-")


def test_scen_fields_agree_with_parse_scen_lines():
    lines = maps.read_scen(SCEN_PREFIX + "10.scen")
    with open(SCEN_PREFIX + "10.scen") as f:
        assert lines == [row.rstrip() for row in f.readlines()][1:] and len(lines) > N
    fields = maps.scen_fields(lines)
    assert all(isinstance(v, int) for row in fields for v in row)
    assert [((a, b), (c, d)) for a, b, c, d in fields] == maps.parse_scen_lines(lines)
    with pytest.raises(AssertionError):
        maps.read_scen(SCEN_PREFIX + "11.scen")               # not shipped


class _File10(random.Random):
    """A Random whose randint(1, 25) names the one shipped file; sample is Random's own."""

    def randint(self, a, b):
        assert (a, b) == (1, 25)
        return 10


def test_draw_scen_draws_like_the_envs():
    lines = maps.read_scen(SCEN_PREFIX + "10.scen")
    want = maps.scen_fields(_File10(5).sample(lines, N))
    rng = _File10(5)
    assert maps.draw_scen(rng, SCEN_PREFIX, N) == want
    twin = _File10(5)
    twin.sample(lines, N)
    assert rng.random() == twin.random()                       # one sample, nothing else drawn
    # more_than_n: a file of exactly n lines is refused (marl_partial) or drawn whole (MAPF_GRID)
    with pytest.raises(AssertionError):
        maps.draw_scen(_File10(5), SCEN_PREFIX, len(lines))
    whole = maps.draw_scen(_File10(5), SCEN_PREFIX, len(lines), more_than_n=False)
    assert sorted(whole) == sorted(maps.scen_fields(lines))
