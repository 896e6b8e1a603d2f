"""What the core MAPF cases (tests/mapf_step_cases.py) cover, checked without a device and
without libmapfx.so: the table reaches every kernel instance the restated dispatch can reach
(84: 56 wave, 28 generic -- the enumeration decides) and every axis the kernels branch on,
all computed from the table; the restated geometry equals the figures the project already
states; the comparer can fail; and the C oracle equals the Python restatement on the table's
shapes.  tests/test_gpu_mapf_step_shapes.py runs the same cases on the device.

The reference itself only works on square maps (it indexes `_grid[i][j]` with i < shape[1],
j < shape[0]) and most of the table is non-square, so these cases pin the
kernels to the RESTATEMENT's semantics only.  `test_c_oracle_matches_python_restatement` is
what gives the non-square expected values a second source: oracle/mapf_oracle.c (the
expected values) against oracle/mapf_oracle.py (GridEnvState, window_obs, primal_obs,
goal_vectors) on every distinct (H, W, window, primal_size) of the table with N <= 16, the
scripted roles included.
"""
import collections

import numpy as np
import pytest

import mapf_step_cases as msc
from mapf_step_cases import (ALL_KERNELS, BY_NAME, CASES, GENERIC_T, ODD_REWARDS, SPLIT_T, build, case_geometry,
                             case_id, case_launches, compare, dispatch, expected_action_path,
                             expected_kernel, geometry, kernel_args, launch_outs, limit_of, split_lds_of)
from oracle import mapf_oracle as O


@pytest.fixture(scope="module", autouse=True)
def _built():
    from oracle import corc
    corc.lib()


def _own(c):
    """The dispatch result of a case's own entry point."""
    return dict(case_launches(c))[c.entry]


def _wave_args(c):
    d = _own(c)
    if d["path"] != "wave":
        return None
    win, roll, fullw, runner, ll, split, occ, abt = d["kernel"][1].split(",")
    return dict(WIN=int(win), roll=roll == "true", fullw=fullw == "true", runner=runner == "true",
                LL=int(ll), split=split == "true", occ=occ == "true", ABT=int(abt))


# ------------------------------------------------------------------ instances
def test_enumeration_counts():
    """The reachable set, and the compiled instances no input reaches (DESIGN.md lists them):
    the four WIN = 0 runner instances -- a runner output set always carries a window -- and
    the fourteen one-byte-cell APL 2 / 4 instances -- one-byte cells mean N <= 127, hence
    L = 128 and one agent per lane."""
    assert len(ALL_KERNELS) == 84
    assert len(msc.WAVE_KERNELS) == 56 and len(msc.GENERIC_KERNELS) == 28
    assert ALL_KERNELS <= msc.COMPILED_WAVE | msc.COMPILED_GENERIC
    assert len(msc.COMPILED_WAVE) == 60 and len(msc.COMPILED_GENERIC) == 42
    un = msc.UNREACHABLE
    assert len(un) == 18
    assert {k for k in un if k[0] == "mapf_wave_kernel"} == {
        ("mapf_wave_kernel", "0,true,%s,true,%s,false,false,0" % fl) for fl in
        (("false", "0"), ("true", "0"), ("true", "16"), ("true", "64"))}
    assert all(k[1].startswith("unsignedchar,") and k[1].split(",")[1] in "24" for k in un
               if k[0] != "mapf_wave_kernel")


def test_table_reaches_every_instance():
    """Deleting a case that is the only one of its instance fails here."""
    seen = collections.defaultdict(list)
    for c in CASES:
        for _, d in case_launches(c):
            seen[d["kernel"]].append(c.name)
    assert set(seen) == ALL_KERNELS, (sorted(ALL_KERNELS - set(seen)), sorted(set(seen) - ALL_KERNELS))
    own = {expected_kernel(c) for c in CASES}
    missing = ALL_KERNELS - own       # every instance is also some case's OWN entry point
    assert not missing, sorted(missing)


def test_kernel_args_reads_the_printed_form():
    p = "void (anonymous namespace)::"
    tail = "(int*, int const*, unsigned char*, unsigned char const*, void const*, int*, unsigned int, " \
           "unsigned int, (anonymous namespace)::Args, (anonymous namespace)::Geo)"
    assert kernel_args(p + "mapf_wave_kernel<5, true, true, true, 16, true, false, 8>" + tail) == \
        ("mapf_wave_kernel", "5,true,true,true,16,true,false,8")
    assert kernel_args(p + "mapf_rollout_kernel<unsigned short, 1, 4>" + tail) == \
        ("mapf_rollout_kernel", "unsignedshort,1,4")
    assert kernel_args(p + "mapf_step_kernel<unsigned char, 1, 0>" + tail) == ("mapf_step_kernel", "unsignedchar,1,0")
    assert kernel_args(p + "reset_kernel(int, int)") is None


def test_dispatch_rule_rows():
    """The rule on rows written out by hand: the instances the existing device tests name
    (tests/test_gpu_parity.py, test_gpu_rollout_store_path.py, test_gpu_rollout_action_staging.py)."""
    runner = launch_outs(("window",), "rollout", "runner")
    everything = launch_outs(("window",), "rollout")
    g2 = geometry(32, 32, 16, 5)
    for T, abt in ((20, 8), (32, 8), (33, 0), (64, 0)):
        d = dispatch(g2, 4096, "rollout", T, runner, act="int8")
        assert d["kernel"] == ("mapf_wave_kernel", "5,true,true,true,16,true,false,%d" % abt)
        assert d["action_path"] == 2
    assert dispatch(g2, 4096, "rollout", 65, runner, act="int8")["action_path"] == 1
    assert dispatch(g2, 4096, "rollout", 20, runner, act="int8", act_aligned=False)["action_path"] == 1
    assert dispatch(g2, 4096, "rollout", 20, runner, act="int32")["action_path"] == 1
    assert dispatch(g2, 4096, "rollout", 20, everything)["action_path"] == 0
    assert dispatch(g2, 4095, "rollout", 20, runner)["kernel"] == \
        ("mapf_wave_kernel", "5,true,false,true,0,false,false,0")
    assert dispatch(g2, 8, "step", 1, launch_outs(("window",), "step"))["kernel"] == \
        ("mapf_wave_kernel", "5,false,true,false,16,false,false,0")
    occ = launch_outs(("window_occ",), "rollout")
    assert dispatch(g2, 4, "rollout", 16, occ)["kernel"] == ("mapf_wave_kernel", "5,true,true,true,16,true,true,8")
    assert dispatch(g2, 4, "step", 1, launch_outs(("window_occ",), "step"))["kernel"] == \
        ("mapf_step_kernel", "unsignedchar,1,0")
    g3 = geometry(64, 64, 64, 5)
    assert dispatch(g3, 2048, "rollout", 64, runner)["kernel"] == \
        ("mapf_wave_kernel", "5,true,true,true,64,true,false,0")
    g5 = geometry(128, 128, 256, 5)
    run5 = launch_outs(("window_occ",), "rollout", "runner")
    assert dispatch(g5, 1024, "rollout", 64, run5)["kernel"] == ("mapf_rollout_kernel", "unsignedshort,1,4")
    assert dispatch(g5, 6, "rollout", 6, launch_outs(("window_occ",), "rollout"))["kernel"] == \
        ("mapf_rollout_kernel", "unsignedshort,1,0")
    assert dispatch(geometry(64, 64, 600, 5), 6, "rollout", 10, run5)["kernel"] == \
        ("mapf_rollout_kernel", "unsignedshort,4,4")
    g4 = geometry(8, 8, 4, 5)
    assert dispatch(g4, 8, "step", 1, launch_outs(("window",), "step"))["kernel"][1].startswith("5,false")


def test_geometry_equals_the_stated_figures():
    """the split's LDS at C2 (32 x 32, 16 agents) is 31,168 B and 35,280 B
    with T = 64 staged; at C3 (64 x 64, 64 agents) 36,672 B and 40,784 B.  mapfx_info as the
    device tests state it: one env per block for the generic rollouts of
    test_generic_rollout_every_step, four agents per lane at N = 1024, pad = 2 for window 5."""
    g = geometry(32, 32, 16, 5)
    assert (g.L, g.EPW, g.es, g.P, g.pl, g.pitch, g.rows) == (16, 4, 1, 2, 4, 40, 36) and g.wv_fast and g.wave_ok
    assert split_lds_of(g, False) == 31168 and split_lds_of(g, False) + 16 + 64 * 64 == 35280
    d = dispatch(g, 4096, "rollout", 64, launch_outs(("window",), "rollout", "runner"), act="int8")
    assert d["staged"] and d["lds"] == 35280
    g = geometry(64, 64, 64, 5)
    assert split_lds_of(g, False) == 36672 and split_lds_of(g, False) + 16 + 64 * 64 == 40784
    for S, N in ((128, 256), (24, 256), (64, 300), (64, 600), (160, 100)):
        g = geometry(S, S, N, 5)
        assert g.EPB == 1, (S, N)
    g = geometry(64, 64, 1024, 5, obs_mode=3)
    assert (g.apl, g.APL, g.L, g.es) == (4, 4, 256, 2)
    assert geometry(24, 24, 100, 5).EPB == 2 and geometry(24, 24, 100, 5).L == 128
    assert geometry(8, 8, 6, 5, obs_mode=3).P == 2 and geometry(8, 8, 6, 5, obs_mode=1).P == 1
    assert geometry(10, 10, 3, 5, 10, 4).P == 5 and geometry(10, 10, 3, 5, 7, 6).P == 3


# ------------------------------------------------------------------ axes
def test_shapes_stay_small_and_mostly_non_square():
    skew = [c for c in CASES if c.H != c.W and c.H % 8 and c.W % 8]
    assert len(skew) > 0.9 * len(CASES), len(skew)
    assert {c.H > c.W for c in skew} == {False, True}
    for c in CASES:
        assert c.T <= 40 and c.E <= 300 and (c.N < 1024 or c.E <= 8), c
        assert c.E >= msc.min_envs(c.N), c


def test_lane_groups_cell_widths_and_windows():
    wave = [c for c in CASES if _own(c)["path"] == "wave"]
    assert {1, 2, 3, 4, 8, 16, 32, 33, 64} <= {c.N for c in wave}
    for N in (1, 2, 3, 4, 8, 16, 32, 33, 64):      # crossed with a non-square map
        assert any(c.N == N and c.H != c.W for c in wave), N
    gen = [c for c in CASES if _own(c)["path"] == "generic"]
    apl = {N: (case_geometry(c).es, case_geometry(c).apl, case_geometry(c).APL) for c in gen for N in [c.N]}
    assert {N: apl[N] for N in (65, 127, 128, 129, 256, 257, 512, 513, 769, 1024)} == {
        65: (1, 1, 1), 127: (1, 1, 1), 128: (2, 1, 1), 129: (2, 1, 1), 256: (2, 1, 1), 257: (2, 2, 2),
        512: (2, 2, 2), 513: (2, 3, 4), 769: (2, 4, 4), 1024: (2, 4, 4)}
    assert {_wave_args(c)["WIN"] for c in wave} == {0, 3, 5, 7}
    refused = {c.window for c in gen if c.N <= 64 and "window" in c.obs and case_geometry(c).pitch < 256}
    assert {1, 4, 9} <= refused
    # the occupancy window on a step, both formats at once: generic even where the wave path is open
    assert any(c.entry == "step" and c.obs == ("window_occ",) and case_geometry(c).wave_ok for c in gen)
    assert any(set(c.obs) >= {"window", "window_occ"} and case_geometry(c).wave_ok for c in gen)
    assert any(c.N <= 64 and not case_geometry(c).wave_ok and case_geometry(c).pitch >= 256 for c in gen)
    assert any(c.N <= 64 and "primal" in c.obs for c in gen)


def test_both_map_builders_on_every_wave_family():
    fam = collections.defaultdict(set)
    for c in CASES:
        a = _wave_args(c)
        if a is None:
            continue
        g = case_geometry(c)
        assert g.wv_fast == (c.W <= 64), c
        name = "split" if a["split"] else "runner" if a["runner"] else "rollout" if a["roll"] else c.entry
        fam[name].add(g.wv_fast)
    assert dict(fam) == {k: {False, True} for k in ("observe", "step", "rollout", "runner", "split")}
    # the split on the fallback builder (the M0 -> M1 copy) at both lane groups, odd steps included
    for LL in (16, 64):
        assert any(_wave_args(c) and _wave_args(c)["split"] and c.N == LL and c.W > 64 and c.T >= 2
                   for c in CASES), LL


def test_partial_last_wave_or_block():
    for c in CASES:
        d, g = _own(c), case_geometry(c)
        per = g.EPW if d["path"] == "wave" else g.EPB
        assert c.E > per or per == 1 or d["fullw"], c            # more than one wave / block
    # every not-fullw wave instance with a partial last wave, every multi-env generic block shape
    assert any(_own(c)["path"] == "wave" and c.E % case_geometry(c).EPW for c in CASES)
    assert any(_own(c)["path"] == "generic" and case_geometry(c).EPB > 1 and c.E % case_geometry(c).EPB
               for c in CASES)


def test_runner_without_split_both_ways():
    got = collections.defaultdict(set)
    for c in CASES:
        a = _wave_args(c)
        if a and a["runner"] and a["fullw"] and not a["split"] and a["LL"] in (16, 64):
            d = _own(c)
            got[a["LL"]].add("misaligned" if c.misalign else "lds" if d["split_lds"] > 64 * 1024 else "?")
            if not c.misalign:
                assert case_geometry(c).wv_lds <= 64 * 1024 < d["split_lds"]
    assert dict(got) == {16: {"misaligned", "lds"}, 64: {"misaligned", "lds"}}


def test_launch_lengths():
    pairs = collections.defaultdict(set)
    for c in CASES:
        a = _wave_args(c)
        if a and a["split"]:
            assert a["ABT"] == (8 if c.T <= 32 else 0)
            pairs[(a["WIN"], a["LL"], a["occ"])].add(c.T)
    assert len(pairs) == 12
    for k, ts in pairs.items():
        assert set(SPLIT_T) <= ts, (k, ts)
    # the last step of a launch moves live agents at every length that is a boundary (a launch
    # whose envs all ended two steps earlier would hide its last action block), and some
    # launches end on finished envs
    live = collections.defaultdict(set)
    for c in CASES:
        a = _wave_args(c)
        if a and a["split"] and build(c)["stats"]["live_last"] > 0:
            live[(a["WIN"], a["LL"], a["occ"])].add(c.T)
    for k in pairs:
        assert {1, 2, 16, 32, 33} <= live[k], (k, live[k])
    assert any(_own(c)["split"] and c.T >= 5 and build(c)["stats"]["live_last"] == 0 for c in CASES)
    gen_roll = [c for c in CASES if c.entry == "rollout" and _own(c)["path"] == "generic"]
    assert set(GENERIC_T) <= {c.T for c in gen_roll if build(c)["stats"]["live_last"] > 0}
    for path in ("wave", "generic"):
        tails = {build(c)["stats"]["live_last"] > 0 for c in CASES
                 if c.entry == "rollout" and _own(c)["path"] == path and not _own(c)["split"] and c.T >= 5}
        assert tails == {False, True}, path
    fold = [c for c in gen_roll if case_geometry(c).fold_R == 8]
    assert any(8 < c.T <= 16 for c in fold) and any(c.T > 16 for c in fold)
    assert {case_geometry(c).L for c in fold} == {64, 128, 256}
    # edge counts of 4 and more under the deferred fold (codes >= 32: the rows added without
    # the table), at both code widths of the ring's reader
    big = [c for c in fold if build(c)["stats"]["edge"] >= 4]
    assert {case_geometry(c).L for c in big} >= {64, 256} and {case_geometry(c).APL for c in big} >= {1, 4}
    assert {case_geometry(c).APL for c in fold} == {1, 2, 4}
    for L in (64, 256):
        assert any(case_geometry(c).L == L and c.T > 16 for c in fold), L
    # fold_R = 0 with finite rewards: one env per block, L >= 64, the ring would cost a block
    f0 = [c for c in gen_roll if case_geometry(c).EPB == 1 and case_geometry(c).L >= 64
          and case_geometry(c).fold_R == 0]
    assert any(c.T > 8 for c in f0) and {case_geometry(c).APL for c in f0} == {1, 2, 4}
    assert any(case_geometry(c).EPB > 1 for c in gen_roll)       # and the per-step fold of shared blocks


def test_action_sources_and_paths():
    by = collections.defaultdict(set)
    for c in CASES:
        d = _own(c)
        fam = "split" if d["split"] else d["path"]
        if c.entry == "rollout":
            by[fam].add(c.act)
            if c.act == "gen":
                by[fam + "-gen-offset"].add(c.env_offset != 0 and c.t0 != 0)
        elif c.entry == "step":
            by[fam + "-step"].add(c.act)
    for fam in ("split", "wave", "generic"):
        assert by[fam] == {"gen", "int8", "int32", "int64"}, (fam, by[fam])
        assert True in by[fam + "-gen-offset"], fam
    assert by["wave-step"] == by["generic-step"] == {"int8", "int32", "int64"}
    paths = collections.defaultdict(set)
    for c in CASES:
        if _own(c)["split"]:
            paths[c.N].add((expected_action_path(c), c.act, c.act_off % 16 == 0))
    for LL in (16, 64):
        assert {p for p, _, _ in paths[LL]} == {0, 1, 2}
        assert (2, "int8", True) in paths[LL] and (1, "int8", False) in paths[LL]
        assert (1, "int32", True) in paths[LL] and (1, "int64", True) in paths[LL] and (0, "gen", True) in paths[LL]
    # unaligned int8 rows outside the split too (a row base at every residue mod 4)
    assert {c.act_off % 4 for c in CASES if c.act == "int8" and not _own(c)["split"] and c.entry == "rollout"} \
        == {0, 1, 2, 3}


def test_state_options_and_rewards():
    for fam in ("split", "wave", "generic"):
        cs = [c for c in CASES if (_own(c)["split"], _own(c)["path"]) ==
              {"split": (True, "wave"), "wave": (False, "wave"), "generic": (False, "generic")}[fam]]
        assert {c.track for c in cs} == {False, True}, fam
        assert {c.shared for c in cs} == {False, True}, fam
        assert {c.rewards for c in cs} == {msc.DEFAULT_REWARDS, ODD_REWARDS}, fam
        assert {c.autoreset for c in cs if c.entry == "rollout"} == {False, True}, fam
    for r in ODD_REWARDS:
        assert float(np.float32(r)) != r        # not representable: the fold's order is in the bits
    for c in CASES:
        assert not c.autoreset or c.entry == "rollout"


def test_full_map_rows_as_words():
    """W % 4 == 0: obs_full leaves as whole words, the row found with m_W4 -- on a non-square
    map in the wave and the generic kernel, with W / 4 = 1 as well."""
    for path in ("wave", "generic"):
        cs = [c for c in CASES if _own(c)["path"] == path and "full" in c.obs and c.W % 4 == 0
              and c.H != c.W and case_geometry(c).es == 1]
        assert any(c.W == 4 for c in cs) and any(c.W > 4 for c in cs), path
        assert any(c.entry == "rollout" for c in cs), path


# ------------------------------------------------------------------ episodes
def test_scripted_episodes_hold_their_events():
    bumps = np.zeros(5, np.int64)
    tot = collections.Counter()
    bad_dtypes, gadgets = set(), 0
    for c in CASES:
        b = build(c)
        bumps += b["bumps"].sum(0)
        for k in ("done_below", "done_at", "resets", "past_done"):
            tot[k, c.autoreset] += b["stats"][k]
        s0, s1 = b["snaps"][0], b["snaps"][1]
        if c.act != "gen":
            assert b["bad"] is not None, c
            t, e, a = b["bad"]
            bad_dtypes.add(c.act)
            assert not 0 <= b["actions"][t, e, a] <= 4
            before, after = b["snaps"][t], b["snaps"][t + 1]       # the refused env: unchanged, reward 0.0
            for f in ("pos", "done", "t", "steps"):
                assert np.array_equal(before[f][e], after[f][e]), (c, f)
            assert after["reward"][e].view(np.uint64) == 0 and not after["node"][e].any()
            if c.N >= 3:              # the stacked swap (a random agent of env 0 may add to it)
                assert s1["node"][0, 1:3].tolist() == [1, 1], c
                if c.T >= 2:
                    e0 = b["snaps"][2]["edge"][0, :3]
                    assert e0[0] >= 2 and e0[1] >= 1 and e0[2] >= 1, c
                    gadgets += e0.tolist() == [2, 1, 1]
            if c.T >= 2 and limit_of(c) > 2:                       # completion below the limit
                assert b["snaps"][2]["term"][1] == 1 and b["snaps"][2]["t"][1] == 2 < limit_of(c), c
            slots = dict(zip(msc.role_slots(c.N), msc.ROLES))
            g_of = lambda e: msc.grid_of(c.H, c.W, 0 if c.shared else e % msc.VARIANTS)  # noqa: E731
            for (e, i), role in slots.items():
                p0, p1 = s0["pos"][e, i], s1["pos"][e, i]
                if role == "on-obstacle":
                    assert g_of(e)[p0[0], p0[1]] != 0
                elif role == "stacked":
                    assert c.N == 1 or np.array_equal(p0, s0["pos"][e, (i - 1) % c.N])
                elif role.startswith("corner"):
                    assert p0[0] in (0, c.H - 1) and p0[1] in (0, c.W - 1) and np.array_equal(p0, p1)
                else:
                    assert np.array_equal(p0, p1), (c, role)      # the bump: it stays where it was
    assert (bumps > 0).all(), bumps
    assert bad_dtypes == {"int8", "int32", "int64"} and gadgets > 100
    for ar in (False, True):
        assert tot["done_below", ar] > 0 and tot["done_at", ar] > 0, ar
    assert tot["past_done", False] > 0 and tot["resets", True] > 0 and tot["resets", False] == 0


# ------------------------------------------------------------------ the comparer
def _as_got(c, snap, keys):
    """A snapshot in the device's dtypes, as `compare` is given it."""
    dt = {"pos": np.int32, "done": np.uint8, "t": np.int32, "steps": np.int32, "node": np.uint8,
          "edge": np.uint8 if c.N <= 256 else np.int16, "traj_pos": np.int32, "traj_done": np.uint8,
          "traj_t": np.int32}
    return {k: snap[k].astype(dt[k]) if k in dt else snap[k].copy() for k in keys}


@pytest.mark.parametrize("name", ["split-w5-l16-win-T16", "gen16-n300-primal-roll", "wave-roll-w5-part",
                                  "gen8-occ-step-n16"])
def test_comparer_fails_on_one_wrong_element(name):
    c = BY_NAME[name]
    b = build(c)
    snap = b["snaps"][2]
    keys = ("pos", "done", "t", "steps") + launch_outs(c.obs, c.entry, c.select)
    assert compare(_as_got(c, snap, keys), snap, 1) is None
    for f in keys:          # one element of each field, last env
        got = _as_got(c, snap, keys)
        flat = got[f].reshape(c.E, -1)
        if got[f].dtype.kind == "f":
            u = flat.view(np.uint64 if got[f].dtype == np.float64 else np.uint32)
            u[-1, -1] ^= 1                                       # one flipped mantissa bit
        else:
            flat[-1, -1] += 1
        d = compare(got, snap, 1)
        assert d is not None and d.field in (f, f + "_planes") and d.env == c.E - 1 and d.call == 1, (f, d)
    # a swapped row / column of one agent, and one wrong cell of one window
    got = _as_got(c, snap, keys)
    e, i = next((e, i) for e in range(c.E) for i in range(c.N) if snap["pos"][e, i, 0] != snap["pos"][e, i, 1])
    got["pos"][e, i] = got["pos"][e, i, ::-1]
    d = compare(got, snap, 1)
    assert d.field == "pos" and d.env == e and d.index == 2 * i
    wkey = "obs_window_occ" if "window_occ" in c.obs else "obs_window"
    got = _as_got(c, snap, keys)
    got[wkey][0, 0].reshape(-1)[3] ^= 1
    d = compare(got, snap, 1)
    assert d.field == wkey and d.env == 0 and d.index == 3
    if wkey == "obs_window_occ":    # the caller's decoder is compared too
        got = _as_got(c, snap, keys)
        got["obs_window_occ_planes"] = msc.window_planes(got[wkey])
        assert compare(got, snap, 1) is None
        got["obs_window_occ_planes"][1, 0, 1, 0, 0] += 1
        assert compare(got, snap, 1).field == "obs_window_occ_planes"
    with pytest.raises(AssertionError):
        compare({"pos ": snap["pos"]}, snap)


# ------------------------------------------------------------------ C oracle vs Python restatement
def _small_shape_cases():
    first = {}
    for c in CASES:
        if c.N <= 16:
            first.setdefault((c.H, c.W, c.window, c.psize if "primal" in c.obs else 0), c)
    return list(first.values())


@pytest.mark.parametrize("c", _small_shape_cases(), ids=case_id)
def test_c_oracle_matches_python_restatement(c):
    """The expected values of `build` (C oracle) against oracle/mapf_oracle.py, step by step,
    on the case's own maps, roles and actions: the first envs (the scripted ones), the last
    and the refused one."""
    b = build(c)
    envs = sorted(set(range(min(c.E, 18))) | {c.E - 1} | ({b["bad"][1]} if b["bad"] else set()))
    refs = {e: O.GridEnvState(-b["grids"][0 if c.shared else e].astype(np.int8), b["init_pos"][e], b["goals"][e],
                              episode_limit=limit_of(c), step_reward=c.rewards[0],
                              collide_reward=c.rewards[1]) for e in envs}

    def check(snap, t):
        for e, r in refs.items():
            assert np.array_equal(np.array(r.pos), snap["pos"][e]), (t, e)
            assert np.array_equal(np.array(r.done, np.uint8), snap["done"][e]), (t, e)
            assert r.t == snap["t"][e] and np.array_equal(r.steps, snap["steps"][e]), (t, e)
            assert np.array_equal(r.full_obs(), snap["obs_full"][e]), (t, e)
            assert np.array_equal(O.window_obs(r.occ, r.pos, c.window), snap["obs_window"][e]), (t, e)
            w = O.window_obs(r.occ, r.pos, c.window)
            assert np.array_equal(msc.window_planes(snap["obs_window_occ"][e]), w), (t, e)
            assert np.array_equal((np.array(r.avail()) << np.arange(5)).sum(-1), snap["avail"][e]), (t, e)
            assert bool(snap["term"][e]) == all(r.done), (t, e)
            if "primal" in c.obs:
                maps, vec = O.primal_obs(r.grid, r.pos, r.goals, c.psize)
                assert np.array_equal(maps, snap["obs_primal"][e]), (t, e)
                assert np.array_equal(vec.view(np.uint64), snap["primal_vec"][e].view(np.uint64)), (t, e)
                # goal_vectors (mapf_gridworld.py:451-463) is the same vector through sqrt, where
                # PRIMAL's goes through libm pow: each correctly rounded to within 1 ulp, the
                # quotient one rounding more -- 2 ulp apart at the most
                for i, ((d0, d1), norm) in enumerate(O.goal_vectors(r.pos, r.goals)):
                    for x, y in zip((d0, d1, norm), vec[i]):
                        assert abs(x - y) <= 2 * np.spacing(abs(y)), (t, e, i)

    check(b["snaps"][0], "reset")
    for t in range(c.T):
        snap = b["snaps"][t + 1]
        for e, r in refs.items():
            if b["bad"] and b["bad"][:2] == (t, e):
                with pytest.raises(AssertionError):      # the reference asserts (:91-92)
                    r.step(b["actions"][t, e])
                continue
            R, _, node, edge, _ = r.step(b["actions"][t, e])
            assert np.float64(R).view(np.uint64) == snap["reward"][e].view(np.uint64), (t, e)
            assert np.array_equal(node, snap["node"][e]) and np.array_equal(edge, snap["edge"][e]), (t, e)
        check(snap, t)
        if c.autoreset:
            for r in refs.values():
                if all(r.done):
                    r.reset()
    for e, r in refs.items():
        assert np.array_equal(np.array(r.pos), b["final"]["pos"][e]) and r.t == b["final"]["t"][e]
