"""What the MARL_PARTIAL plain-step cases (tests/partial_step_cases.py) cover, checked on the
restatement alone -- no device, no libmapfx.so: the table reaches all 39 step instances and
all 7 BFS instances, both orientations of a non-square map per kernel family, every table
width with and without the LDS sqrt table per fast (WIN, LF) pair, partial last waves and
blocks; every episode holds the stacked swap (an edge count of 2), a node collision, an env
collision on each side and on an obstacle, a bonus below the limit, a run to the limit,
a stay-on-goal reward and steps on a terminated env; and the comparer can fail.
tests/test_gpu_partial_step_shapes.py runs the same cases on the device.

Two things no episode can hold, by the env's own rules: with N = 1 there is no node
collision and no stay-on-goal reward (the one agent's arrival completes the env, and a done
agent collects nothing).  N = 1 and N = 2 have no stacked swap (it takes three agents)."""
import collections

import numpy as np
import pytest

import partial_step_cases as psc
from partial_step_cases import (ALL_BFS_KERNELS, ALL_STEP_KERNELS, CASES, FAST_PAIRS, as_device, build,
                                case_id, compare, expected_bfs_kernel, expected_geometry,
                                expected_step_kernel, family, lane_group, limit_of, table_bytes)


def test_table_reaches_every_instance():
    step = {expected_step_kernel(c) for c in CASES}
    assert step == ALL_STEP_KERNELS and len(step) == 39
    assert len({k for k in step if k[1].endswith("false")}) == 15           # fast plain
    assert len({k for k in step if k[1].endswith("0,0,0,true")}) == 6       # generic
    assert len({k for k in step if k[0] == "partial_wg_kernel"}) == 18
    bfs = {expected_bfs_kernel(c) for c in CASES}
    assert bfs == ALL_BFS_KERNELS and len(bfs) == 7


def test_kernel_args_reads_the_printed_form():
    p = "void (anonymous namespace)::"
    assert psc.kernel_args(p + "partial_kernel<5, 5, 16, 2, false>(PGeo, PArgs)") == \
        ("partial_kernel", "5,5,16,2,false")
    assert psc.kernel_args(p + "partial_wg_kernel<9, 4>(PGeo, PArgs)") == ("partial_wg_kernel", "9,4")
    assert psc.kernel_args(p + "partial_bfs_big_kernel<unsigned char>(PGeo, unsigned char const*, int const*, "
                           "unsigned char const*, unsigned char*)") == ("partial_bfs_big_kernel", "unsignedchar")
    assert psc.kernel_args(p + "partial_bfs_kernel<short>(PGeo)") == ("partial_bfs_kernel", "short")
    assert psc.kernel_args(p + "pdist_invalidate_kernel(long long)") is None


def test_dispatch_rule_table():
    """The rule on rows written out by hand (pick(), launch(), wg_apl, mapfx_partial_goal_dist)."""
    R = collections.namedtuple("R", "H W N win K")
    rows = [
        (R(32, 32, 16, 5, 5), ("partial_kernel", "5,5,16,2,false"), ("partial_bfs_kernel", "short")),
        (R(12, 12, 5, 5, 5), ("partial_kernel", "5,5,8,1,false"), ("partial_bfs_kernel", "unsignedchar")),
        (R(200, 200, 9, 5, 5), ("partial_kernel", "5,5,16,0,false"), ("partial_bfs_big_kernel", "int")),
        (R(3, 80, 8, 5, 5), ("partial_kernel", "5,5,8,1,false"), ("partial_bfs_big_kernel", "unsignedchar")),
        (R(16, 16, 12, 3, 5), ("partial_kernel", "3,5,16,2,false"), ("partial_bfs_kernel", "short")),
        (R(16, 16, 8, 3, 5), ("partial_kernel", "3,0,0,0,true"), ("partial_bfs_kernel", "short")),
        (R(16, 16, 12, 7, 4), ("partial_kernel", "7,0,0,0,true"), ("partial_bfs_kernel", "short")),
        (R(10, 10, 64, 5, 5), ("partial_kernel", "5,0,0,0,true"), ("partial_bfs_kernel", "unsignedchar")),
        (R(70, 9, 33, 5, 5), ("partial_kernel", "5,0,0,0,true"), ("partial_bfs_big_kernel", "short")),
        (R(10, 10, 65, 9, 5), ("partial_wg_kernel", "9,1"), ("partial_bfs_kernel", "unsignedchar")),
        (R(40, 40, 257, 0, 5), ("partial_wg_kernel", "0,2"), ("partial_bfs_kernel", "short")),
        (R(40, 40, 513, 1, 5), ("partial_wg_kernel", "1,4"), ("partial_bfs_kernel", "short")),
        (R(40, 40, 1024, 1, 5), ("partial_wg_kernel", "1,4"), ("partial_bfs_kernel", "short")),
        (R(257, 6, 4, 5, 5), ("partial_wg_kernel", "5,1"), ("partial_bfs_huge_kernel", "short")),
        (R(128, 257, 4, 5, 5), ("partial_wg_kernel", "5,1"), ("partial_bfs_huge_kernel", "int")),
    ]
    for c, step, bfs in rows:
        assert expected_step_kernel(c) == step and expected_bfs_kernel(c) == bfs, c


def test_geometry_restates_the_documented_staging_classes():
    """The rows derived in tests/test_gpu_runner_shapes.py's table comment (win 5, K 5)."""
    G = collections.namedtuple("G", "H W N win K")
    g = expected_geometry(G(12, 12, 5, 5, 5))
    assert (g["per_env"], g["EPW"], g["stage_lanes"], g["wpb"], g["sqrt_table"]) == (1184, 8, 64, 4, True)
    g = expected_geometry(G(32, 32, 16, 5, 5))
    assert (g["per_env"], g["EPW"], g["stage_lanes"], g["wpb"], g["sqrt_table"]) == (4048, 4, 64, 4, False)
    g = expected_geometry(G(64, 64, 16, 5, 5))
    assert (g["per_env"], g["EPW"], g["stage_lanes"], g["wpb"]) == (11344, 4, 32, 3)
    g = expected_geometry(G(200, 200, 9, 5, 5))
    assert (g["EPW"], g["stage_lanes"], g["wpb"]) == (1, 0, 1)


def test_table_covers_orientations_widths_and_staging():
    fams = {}
    for c in CASES:
        fams.setdefault(family(c), []).append(c)
    assert set(fams) == {"fast", "generic", "workgroup"}
    for name, cs in fams.items():
        assert any(c.H > c.W for c in cs) and any(c.W > c.H for c in cs), name
    fast = fams["fast"]
    for win, L in FAST_PAIRS:
        mine = [c for c in fast if (c.win, lane_group(c.N)) == (win, L)]
        have = {(table_bytes(c.H, c.W), expected_geometry(c)["sqrt_table"]) for c in mine}
        assert {(1, True), (1, False), (2, True), (2, False), (4, False)} <= have, (win, L, have)
        assert any(c.W > 32 and table_bytes(c.H, c.W) == 1 for c in mine) or \
            any(c.H > 32 and table_bytes(c.H, c.W) == 1 for c in mine), (win, L)
    # u8 tables with bitmap rows that straddle 32-bit words (W > 32), and the transposes
    assert any(c.W > 32 and table_bytes(c.H, c.W) == 1 for c in fast)
    assert {(c.H, c.W) for c in fast if table_bytes(c.H, c.W) == 4} == {(129, 256), (256, 129)}
    # the three staging classes of the fast path
    assert {expected_geometry(c)["stage_lanes"] for c in fast} == {64, 32, 0}
    for c in fast:      # as the case table's comment derives them
        g = expected_geometry(c)
        if table_bytes(c.H, c.W) == 4:
            assert (g["stage_lanes"], g["EPW"], g["wpb"]) == (0, 1, 2), c
        elif c.name != "fast-half-64x60":
            assert (g["stage_lanes"], g["EPW"], g["wpb"]) == \
                (32 if c.win == 7 else 64, 64 // lane_group(c.N), 4), c
    g = expected_geometry(psc.BY_NAME["fast-half-64x60"])
    assert (g["stage_lanes"], g["EPW"], g["wpb"]) == (32, 4, 3)
    # the generic kernel's lane groups, the workgroup kernel's agent rows
    assert {lane_group(c.N) for c in fams["generic"]} >= {1, 2, 4, 8, 16, 64}
    wg = fams["workgroup"]
    assert any(512 < c.N <= 768 for c in wg) and any(c.H > 256 for c in wg) and any(c.W > 256 for c in wg)
    assert sum(c.N < 3 for c in CASES) <= 2
    assert {c.dtype for c in CASES} == {"int8", "int32", "int64"}
    assert any(c.shared for c in CASES) and any(not c.shared for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_last_wave_and_last_block_are_partial(c):
    g = expected_geometry(c)
    if g["big"]:
        assert (g["EPW"], g["wpb"]) == (1, 1)       # one workgroup per env: nothing partial
        return
    per_block = g["EPW"] * g["wpb"]
    assert g["lds"] * g["wpb"] <= 160 * 1024 and per_block > 1
    assert c.E % per_block != 0 and (g["EPW"] == 1 or c.E % g["EPW"] != 0)
    assert c.E > per_block, "more than one block"


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_episode_holds_what_the_case_claims(c):
    b = build(c)
    limit, T, N = limit_of(c), c.T, c.N
    snaps = b["snaps"]
    assert len(snaps) == T + 1 and limit == T - 2 >= 2
    grids = b["grids"]
    for e in range(c.E):        # the reference's domain
        g = grids[0 if c.shared else e]
        assert (g[tuple(b["starts"][e].T)] == 0).all() and (g[tuple(b["goals"][e].T)] == 0).all()
        assert len({tuple(p) for p in b["starts"][e]}) == N == len({tuple(p) for p in b["goals"][e]})
    edge = np.stack([s["edge"] for s in snaps[1:]])
    node = np.stack([s["node"] for s in snaps[1:]])
    term = np.stack([s["terminated"] for s in snaps[1:]])            # [T, E]
    at_goal = np.stack([s["at_goal"] for s in snaps[1:]])
    if N >= 3:      # the gadget: env 0, agents 0, 1, 2
        assert edge[1, 0, :3].tolist() == [2, 1, 1], edge[1, 0, :3]
        assert node[0, 0, 1:3].tolist() == [1, 1] and node[1, 0, 1:3].tolist() == [1, 1]
    if N >= 2:
        assert node.any()
    assert (b["bumps"].sum(0) > 0).all(), b["bumps"].sum(0)          # four sides, an obstacle
    if N >= 2:
        assert b["stays"][:limit].sum() > 0, "no stay-on-goal reward"
    first = np.where(term.any(0), term.argmax(0) + 1, 0)            # t of the first terminated = 1
    assert (first > 0).all() and (first <= limit).all()
    early = np.flatnonzero(first < limit)
    assert len(early) and all(at_goal[first[e] - 1, e].all() for e in early), "no bonus below the limit"
    assert first[1] < limit and first[2] == limit and at_goal[limit - 1, 2].all()
    assert (first == limit).any() and (T - first >= 2).all()
    # the bonus is in the reward: the run-out env at t = limit, limit + 1, limit + 2
    for t in (limit, limit + 1, limit + 2):
        r = float(snaps[t]["reward"].view(np.float64)[2])
        bonus = (psc.KW["complete_reward"] / (psc.KW["gamma"] ** (limit - t))) * psc.KW["complete_fac"]
        assert r > N * bonus - 10 * N, (t, r)


def _flip(arr, idx, bit):
    a = np.array(arr)
    raw = a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32) if a.dtype == np.float32 else a
    raw[idx] ^= np.array(bit).astype(raw.dtype)
    return a


def test_compare_names_each_flipped_element():
    c = psc.BY_NAME["act-fast"]
    b = build(c)
    snap = b["snaps"][3]
    batch, out = as_device(c, snap)
    assert compare(batch, out, snap, 3) is None
    N, D = c.N, 2 * c.win * c.win + 13 * c.K
    where = {"pos": ((4, 2, 1), 1, 5), "steps": ((20, 8), 1, 8), "at_goal": ((0, 0), 1, 0),
             "done": ((7, 3), 1, 3), "goal_cost": ((9, 1), 2, 1), "node": ((3, 4), 1, 4),
             "edge": ((5, 5), 2, 5), "t": ((6,), 1, 0), "terminated": ((20,), 1, 0),
             "total_coll": ((1,), 4, 0), "pdist": ((2, 7), 1, 7)}
    for f, (idx, bit, flat) in where.items():
        setattr(batch, f, _flip(getattr(batch, f), idx, bit))
        d = compare(batch, out, snap, 3)
        assert d is not None and (d.call, d.field, d.env, d.index) == (3, f, idx[0], flat), (f, d)
        assert d.got != d.want
        batch, out = as_device(c, snap)
    for f, idx, bit, flat in (("reward", (11,), 1, 0), ("obs", (12, 6, 77), 1 << 22, 6 * D + 77),
                              ("obs", (0, 0, 0), 1, 0), ("obs", (20, N - 1, D - 1), 1 << 31, N * D - 1),
                              ("state", (8, 2), 1, 2), ("avail", (13, 2), 16, 2)):
        out[f] = _flip(out[f], idx, bit)
        d = compare(batch, out, snap, 3)
        assert d is not None and (d.field, d.env, d.index) == (f, idx[0], flat), (f, d)
        batch, out = as_device(c, snap)
    # pnbr: an on-grid entry is compared, an off-grid one is not (it holds junk already)
    ok = snap["pnbr_ok"]
    assert not ok.all() and (batch.pnbr[~ok] == 0x5A5A).all()
    e, i, a = (int(v) for v in np.argwhere(ok)[-1])
    batch.pnbr[e, i, a] ^= 1
    d = compare(batch, out, snap, 3)
    assert (d.field, d.env, d.index) == ("pnbr", e, 4 * i + a), d
    batch, out = as_device(c, snap)
    e, i, a = (int(v) for v in np.argwhere(~ok)[0])
    batch.pnbr[e, i, a] ^= 1
    assert compare(batch, out, snap, 3) is None
    # the first field in FIELDS order wins; a reward is compared only after a step
    batch.edge = _flip(batch.edge, (0, 0), 1)
    batch.pos = _flip(batch.pos, (9, 0, 0), 1)
    assert compare(batch, out, snap, 3)[:3] == (3, "pos", 9)
    batch, out = as_device(c, b["snaps"][0])
    out["reward"][:] = 123.0
    assert compare(batch, out, b["snaps"][0], "reset") is None
    # the workgroup kernel keeps no pnbr, int32 tables have none
    w = psc.BY_NAME["act-wg"]
    wb, wo = as_device(w, build(w)["snaps"][1])
    wb.pnbr[:] = 77
    assert compare(wb, wo, build(w)["snaps"][1], 1) is None
    i32 = psc.BY_NAME["fast-w5-l16-i32"]
    assert as_device(i32, build(i32)["snaps"][0])[0].pnbr is None
