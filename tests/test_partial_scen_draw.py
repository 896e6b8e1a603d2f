"""The device scenario draw's host side (CPU): the scenario table and the numpy
restatement of mapfx_partial_draw (include/mapfx_partial.h, mapfx.rng.scen_draw).

The kernel is compared with the restatement bit for bit in tests/test_gpu_partial_draw.py;
here the restatement itself is pinned: its table is what the runner's host draw parses, its
samples are valid, deterministic, shard-invariant and uniform (a uniform file, then a uniform
ordered sample of N distinct lines -- random.randint + random.sample's distribution,
marl_partial.py:902-929).
"""
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN

SCEN = os.path.join(GOLDEN, "scen")


def _renumber(tmp_path, names, prefix="s-"):
    for k, name in enumerate(names, start=1):
        shutil.copy(os.path.join(SCEN, name), str(tmp_path / ("%s%d.scen" % (prefix, k))))
    return str(tmp_path / prefix)


class _Slice:
    """A `random.Random` stand-in: file k, then the n lines from `off` on."""

    def __init__(self, k, off):
        self.k, self.off = k, off

    def randint(self, a, b):
        return self.k

    def sample(self, lines, n):
        return lines[self.off:self.off + n]


def _host_parse(prefix, k):
    """Every line of file k as runners._scen_draw parses it: [L, 4] (sr, sc, gr, gc)."""
    from mapfx import runners
    L = len(runners._scen_lines(prefix + str(k) + ".scen"))
    s0, g0 = runners._scen_draw(_Slice(k, 0), prefix, L - 1)
    s1, g1 = runners._scen_draw(_Slice(k, 1), prefix, L - 1)
    return np.concatenate([np.array(s0 + s1[-1:]), np.array(g0 + g1[-1:])], axis=1)


def test_scen_table_equals_host_parsing(tmp_path):
    from mapfx.maps import load_scen_table
    names8 = sorted(n for n in os.listdir(SCEN) if n.startswith("empty-8-8-random-"))
    prefix = _renumber(tmp_path, names8)
    lines, n_lines = load_scen_table(prefix, 8, 8, n_files=len(names8))
    assert lines.dtype == np.int16 and n_lines.dtype == np.int32
    assert lines.shape == (len(names8), 32, 4) and n_lines.tolist() == [32] * len(names8)
    for k in range(1, len(names8) + 1):
        assert np.array_equal(lines[k - 1], _host_parse(prefix, k)), k
    # the row / col swap: the file's fields 4..7 are start x, y, goal x, y
    with open(prefix + "1.scen") as f:
        v = f.readlines()[1].split("\t")
    assert lines[0, 0].tolist() == [int(v[5]), int(v[4]), int(v[7]), int(v[6])]
    # unequal lengths: zero-padded past each file's own
    prefix = _renumber(tmp_path, ["random-32-32-10-random-19.scen", "maze-32-32-4-random-10.scen"],
                       prefix="m-")
    lines, n_lines = load_scen_table(prefix, 32, 32, n_files=2)
    assert n_lines.tolist() == [461, 395] and lines.shape == (2, 461, 4)
    assert not lines[1, 395:].any()
    for k in (1, 2):
        assert np.array_equal(lines[k - 1, :n_lines[k - 1]], _host_parse(prefix, k)), k


def test_scen_table_errors(tmp_path):
    from mapfx.maps import load_scen_table, write_synthetic_scen
    prefix = _renumber(tmp_path, ["empty-8-8-random-2.scen", "empty-8-8-random-3.scen"])
    with pytest.raises(AssertionError):
        load_scen_table(prefix, 8, 8, n_files=3)          # 3.scen is missing
    with pytest.raises(AssertionError):
        load_scen_table(prefix, 8, 8)                     # the default wants 25 files
    big = _renumber(tmp_path, ["random-32-32-10-random-19.scen"], prefix="b-")
    with pytest.raises(ValueError, match=r"b-1\.scen line \d+"):
        load_scen_table(big, 8, 8, n_files=1)             # a 32 x 32 file on an 8 x 8 grid
    with pytest.raises(ValueError, match=r"b-1\.scen line \d+"):
        load_scen_table(big, 32, 31, n_files=1)
    load_scen_table(big, 32, 32, n_files=1)
    grid = np.zeros((8, 8), dtype=np.int8)
    write_synthetic_scen(str(tmp_path / "l-"), grid, [4096, 4097], seed=3)
    lines, n_lines = load_scen_table(str(tmp_path / "l-"), 8, 8, n_files=1)
    assert lines.shape == (1, 4096, 4)
    with pytest.raises(ValueError, match="4096"):
        load_scen_table(str(tmp_path / "l-"), 8, 8, n_files=2)


def test_synthetic_scen_lines_are_free_cells(tmp_path):
    from mapfx.maps import load_scen_table, synthetic_instances, write_synthetic_scen
    grid = synthetic_instances(1, 9, 13, 2, p_obstacle=0.3, seed=5)["grid"][0]
    write_synthetic_scen(str(tmp_path / "g-"), grid, [17, 40, 3], seed=2)
    lines, n_lines = load_scen_table(str(tmp_path / "g-"), 9, 13, n_files=3)
    assert n_lines.tolist() == [17, 40, 3]
    for k, L in enumerate(n_lines):
        for c in (0, 2):
            assert (grid[lines[k, :L, c], lines[k, :L, c + 1]] == 0).all()


N_LINES = np.array([17, 33, 461, 1000, 100, 65, 9, 8, 7, 250], dtype=np.int32)


def test_scen_draw_properties():
    from mapfx import rng
    assert (rng.STREAM_SCEN_FILE, rng.STREAM_SCEN_LINE) == (0x500, 0x600)
    N, seed = 8, 0x5EED1234
    ids = np.arange(64)
    f, ln = rng.scen_draw(seed, ids, 0, N_LINES, N)
    assert f.shape == (64,) and ln.shape == (64, N)
    assert f.min() >= 0 and f.max() < len(N_LINES)
    bad = N_LINES[f] <= N
    assert bad.any() and (~bad).any()
    assert (ln[bad] == -1).all()                              # L <= N (8 and 7 lines): no draw
    for e in np.flatnonzero(~bad):
        assert len(set(ln[e].tolist())) == N                  # distinct
        assert ln[e].min() >= 0 and ln[e].max() < N_LINES[f[e]]
    assert (N_LINES[f] == N + 1).any()                        # L = N + 1 is drawn
    # deterministic; another episode / seed is another draw
    f2, ln2 = rng.scen_draw(seed, ids, 0, N_LINES, N)
    assert np.array_equal(f, f2) and np.array_equal(ln, ln2)
    f3, ln3 = rng.scen_draw(seed, ids, 1, N_LINES, N)
    assert not np.array_equal(f, f3) and not np.array_equal(ln, ln3)
    f4, ln4 = rng.scen_draw(seed + 1, ids, 0, N_LINES, N)
    assert not np.array_equal(f, f4) and not np.array_equal(ln, ln4)
    # per-env episode counters
    eps = np.where(ids % 2 == 0, 0, 1)
    f5, ln5 = rng.scen_draw(seed, ids, eps, N_LINES, N)
    assert np.array_equal(ln5[0::2], ln[0::2]) and np.array_equal(ln5[1::2], ln3[1::2])
    assert np.array_equal(f5[0::2], f[0::2]) and np.array_equal(f5[1::2], f3[1::2])
    # shard invariance: an env's draw depends on its global id alone
    fa, la = rng.scen_draw(seed, np.arange(0, 4), 3, N_LINES, N)
    fb, lb = rng.scen_draw(seed, np.arange(4, 8), 3, N_LINES, N)
    fw, lw = rng.scen_draw(seed, np.arange(8), 3, N_LINES, N)
    assert np.array_equal(fw, np.concatenate([fa, fb]))
    assert np.array_equal(lw, np.concatenate([la, lb]))


def test_scen_draw_edge_lengths():
    from mapfx import rng
    f, ln = rng.scen_draw(7, np.arange(32), 0, [9], 8)        # L = N + 1: all but one line
    assert (f == 0).all()
    for e in range(32):
        assert len(set(ln[e].tolist())) == 8 and ln[e].max() < 9
    assert len({tuple(r) for r in ln.tolist()}) > 1
    f, ln = rng.scen_draw(7, np.arange(4), 0, [8], 8)         # L = N: the reference asserts
    assert (ln == -1).all()
    f, ln = rng.scen_draw(7, np.arange(4), 0, [2], 1)
    assert ln.shape == (4, 1) and set(ln.reshape(-1).tolist()) <= {0, 1}


def test_scen_draw_matches_scalar_definition():
    """The definition of include/mapfx_partial.h in plain Python integers."""
    from mapfx import rng
    M = (1 << 64) - 1

    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    def key(seed, gid, ep, stream, idx):
        return mix(seed ^ (gid * int(rng.K_ENV) & M) ^ (ep * int(rng.K_T) & M)
                   ^ (idx * int(rng.K_CELL) & M) ^ (stream * int(rng.K_STREAM) & M))

    seed, N = 0xDEADBEEFCAFE, 5
    gids, eps = [0, 3, 1 << 33, 123456789], [0, 1, 7, 2]
    f, ln = rng.scen_draw(seed, gids, eps, N_LINES, N)
    for i, (gid, ep) in enumerate(zip(gids, eps)):
        fk = ((key(seed, gid, ep, 0x500, 0) >> 32) * len(N_LINES)) >> 32
        assert f[i] == fk
        s = sorted((key(seed, gid, ep, 0x600, j) & ~0xFFFF) | j for j in range(int(N_LINES[fk])))
        assert ln[i].tolist() == [x & 0xFFFF for x in s[:N]]


UNIFORM_SEED = 20261020


def test_scen_draw_is_uniform():
    """20,000 envs at a fixed seed: every count within 5 sigma of the uniform law's
    (binomial sigma = sqrt(n p (1 - p)))."""
    from mapfx import rng
    n = 20000
    ids = np.arange(n)

    def within(counts, p):
        sigma = np.sqrt(n * p * (1 - p))
        return np.abs(counts - n * p).max() <= 5 * sigma

    f, _ = rng.scen_draw(UNIFORM_SEED, ids, 0, np.full(25, 40), 8)
    assert within(np.bincount(f, minlength=25), 1 / 25)
    f, ln = rng.scen_draw(UNIFORM_SEED, ids, 0, [40], 8)
    assert (f == 0).all()
    assert within(np.bincount(ln.reshape(-1), minlength=40), 8 / 40)   # a line is in the sample
    assert within(np.bincount(ln[:, 0], minlength=40), 1 / 40)         # agent 0's line
    assert within(np.bincount(ln[:, 7], minlength=40), 1 / 40)         # the last agent's line
