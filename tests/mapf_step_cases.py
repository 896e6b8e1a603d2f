"""Cases, scripted episodes, the dispatch rule and the comparer of the core MAPF tests
(tests/test_mapf_step_cases.py on the CPU, tests/test_gpu_mapf_step_shapes.py on the device):
mapfx_observe / mapfx_step / mapfx_rollout of csrc/mapfx.hip at every kernel instance the
host dispatch can reach.  TEST INFRASTRUCTURE ONLY; no test lives here, and nothing here
imports mapfx or torch.

Every expected value is the C oracle's (oracle/mapf_oracle.c through oracle.corc.OracleBatch,
pinned to the reference by the goldens, tests/test_oracle_c.py), which takes H and W
separately.  The reference itself indexes its grid as if it were square, so
the non-square cases -- most of the table: a square map hides every H / W / pitch / rows
mix-up -- pin the kernels to the oracle's semantics only; tests/test_mapf_step_cases.py gives
those expected values their second source, the Python restatement (oracle/mapf_oracle.py).

`geometry` restates layout()'s sums, `dispatch` restates pick_wave(), launch(), pick_wave_kernel
and pick_kernel; `expected_kernel` / `expected_action_path` answer for a case's launch.  A
kernel comes back as (name, template arguments without spaces), the form `kernel_args`
reduces a mapfx_last_kernel string to; the demangler prints every template argument, the
defaulted ones included.  `ALL_KERNELS` is the enumeration of `dispatch` over `DOMAIN`.

A case is one batch and one entry point:
  observe   reset(), then `T` steps each followed by observe(): reset's launch and every
            observe launch are compared (the state must stay as the step left it);
  step      reset(), then `T` step() calls;
  rollout   reset(), then ONE launch of T steps into caller-owned trajectory buffers: slot k
            is compared with the oracle after its step k, the state with the oracle's last.
Random actions are the base of every episode; on top of them `build` scripts
  env 0      the stacked-swap gadget (N >= 3): agent 0 waits on Y, agents 1 and 2 stand on two
             other neighbours of Y's neighbour X; step 0 both move into X (node = 1, 1), step 1
             agent 0 moves to X while both move to Y: edge = [2, 1, 1].  N = 2: the two movers.
  env 1      completion below the limit: every goal one free move from its start, all stay
             at step 0 and make the move at step 1, then random actions on a finished env
             (or, with autoreset, a fresh episode);
  env 2      nothing scripted: it runs through episode_limit like every env that does not
             complete (`limit_of`: two steps past it, a second episode, or at the last step);
  envs 3..   eleven roles, one agent each (`role_slots`): a bump into each border and one
             into an obstacle, an agent that starts ON an obstacle (quirk 1), one stacked on
             its neighbour's start, and one in each corner that walks out over both of its borders;
  one env    (buffer actions only) gets an action outside 0..4 at step min(1, T - 1): the
             oracle refuses the env as the kernels do (state unchanged, reward 0.0, the
             observations of the unchanged state) and the `err` word names it.
"""
from __future__ import annotations

import functools
import itertools
import math
import re
import types
from collections import namedtuple

import numpy as np

from oracle import corc

OBS_FULL, OBS_WINDOW, OBS_PRIMAL = 1, 2, 4
OBS_MODES = {"full": OBS_FULL, "window": OBS_WINDOW, "window_occ": OBS_WINDOW, "primal": OBS_PRIMAL}
STEP_KEYS = ("reward", "reward_f32", "term", "node", "edge", "avail")
OBS_KEYS = ("term", "avail", "obs_full", "obs_window", "obs_window_occ", "obs_primal", "primal_vec")
TRAJ_KEYS = ("traj_pos", "traj_done", "traj_t")
RUNNER_KEYS = ("reward", "term", "node", "edge", "avail") + TRAJ_KEYS
KIND_KEYS = {"full": ("obs_full",), "window": ("obs_window",), "window_occ": ("obs_window_occ",),
             "primal": ("obs_primal", "primal_vec")}
DEFAULT_REWARDS = (-0.01, -10.0)
ODD_REWARDS = (0.1, -0.7)         # not representable, different magnitudes: the fold order shows
DELTAS = ((-1, 0), (1, 0), (0, -1), (0, 1), (0, 0))
VARIANTS = 5                      # distinct maps a per-env case cycles through


def _up(x, m):
    return (x + m - 1) // m * m


# --------------------------------------------------------------------------- geometry
@functools.lru_cache(maxsize=None)
def geometry(H, W, N, window=5, primal_size=10, obs_mode=OBS_WINDOW, rewards=DEFAULT_REWARDS):
    """layout()'s sums (names as in csrc/mapfx.hip's Geo), or None where mapfx_create refuses the
    configuration (one env over 160 KB of LDS)."""
    es = 1 if N <= 127 else 2                          # mapfx_obs_elem_size: bytes per cell
    L = 1
    while L < N and L < 256:
        L <<= 1
    apl = -(-N // L)
    APL = 1 if apl <= 1 else 2 if apl <= 2 else 4      # the instance an APL of 3 runs
    P = 1
    if obs_mode & OBS_WINDOW:
        P = max(P, window // 2, window - 1 - window // 2)
    if obs_mode & OBS_PRIMAL:
        P = max(P, primal_size // 2, primal_size - 1 - primal_size // 2)
    cpw = 4 // es
    pl = _up(P, cpw)
    pitch = _up(pl + W + P, 8) if es == 1 else _up(W + pl, cpw)
    rows = H + 2 * P
    tail = 0 if es == 1 else pl + P
    wpr = pitch // cpw
    map_words = (rows * pitch + tail + cpw - 1) // cpw
    bits_words = (H * W + 31) // 32
    map_env_bytes = _up(map_words * 4, 16)
    bits_env_bytes = _up(bits_words * 4, 16)
    wlen = 2 * window * window
    prim = bool(obs_mode & OBS_PRIMAL)

    def lds_for(epb):
        return (epb * map_env_bytes + (4 if prim else 2) * _up(epb * N * 4, 16)
                + max(epb * bits_env_bytes, _up(epb * N * 8, 16)) + _up(epb * 12 * 4, 16))

    EPB = 256 // L
    while EPB > 1 and lds_for(EPB) > 48 * 1024:
        EPB -= 1
    if lds_for(EPB) > 160 * 1024:
        return None
    gen_lds = lds_for(EPB)
    rew_bytes = max(EPB * bits_env_bytes, _up(EPB * N * 8, 16))
    fold_R = 0
    code_pitch = _up(2 * N, 16) + 16
    if EPB == 1 and L >= 64 and all(math.isfinite(r) for r in rewards):
        ring = max(rew_bytes, 8 * code_pitch)
        lds_f = gen_lds - rew_bytes + ring + 32 * 8 + 8 * 4
        if 160 * 1024 // lds_f >= 160 * 1024 // gen_lds:    # the blocks per CU stay
            fold_R, gen_lds = 8, lds_f
    g = dict(H=H, W=W, N=N, window=window, es=es, L=L, APL=APL, apl=apl, P=P, pl=pl, pitch=pitch,
             rows=rows, wpr=wpr, map_words=map_words, bits_words=bits_words,
             map_env_bytes=map_env_bytes, bits_env_bytes=bits_env_bytes, wlen=wlen, EPB=EPB,
             BT=EPB * L, gen_lds=gen_lds, fold_R=fold_R, wave_ok=False, EPW=0, wv_fast=False,
             wv_lds=0, wv_split_ok=False)
    if L <= 64 and es == 1:                            # the wave-local layout: EPW envs per wave
        EPW = 64 // L
        wv_bits = _up(bits_words * 4 + 4, 16)
        fast = W <= 64 and wpr <= 24 and wpr % 2 == 0 and 1 <= pl <= 32
        o = 2 * EPW * map_env_bytes + (0 if fast else EPW * wv_bits)
        rew_base = max((N + 1) // 2 * 2, L)
        rew_row = rew_base + (2 if rew_base % 16 == 0 else 0)
        o += 2 * _up(EPW * rew_row * 8, 16)
        g.update(EPW=EPW, wv_fast=fast, wv_lds=o,
                 wv_split_ok=L in (16, 64) and window in (3, 5, 7),
                 wave_ok=o <= 64 * 1024 and pitch < 256 and rows * pitch < 65536)
    return types.SimpleNamespace(**g)


def split_fold_lds(L):
    return 1024 * 8 + 32 * 64 * 2 if L > 16 else 256 * 8 + 32 * 64


SPLIT_DBM_INFO, SPLIT_DBM_EDGE = 2 * 64 * 16, 3 * 64
SPLIT_STAGE_MAX_T, SPLIT_WG_PER_CU, AB_SHORT_T = 64, 4, 32
FEAT_PRIM, FEAT_FULL, FEAT_RUN = 1, 2, 4


def split_lds_of(g, occ):
    return (g.wv_lds + g.EPW * g.map_env_bytes + SPLIT_DBM_INFO + SPLIT_DBM_EDGE
            + 2 * 64 * (g.wlen // 2 if occ else g.wlen) + split_fold_lds(g.L))


def _b(v):
    return "true" if v else "false"


def dispatch(g, E, entry, T, outs, out_aligned=True, act="gen", act_aligned=True):
    """pick_wave() and launch() for one call: `entry` observe / step / rollout, `outs` the non-NULL outputs,
    `out_aligned` every runner output pointer 16-byte aligned, `act` "gen" or the buffer's
    dtype, `act_aligned` its pointer 16-byte aligned.  Returns kernel, action_path and the
    intermediate decisions."""
    roll = entry == "rollout"
    outs = frozenset(outs) & frozenset(OBS_KEYS) if entry == "observe" else frozenset(outs)
    T = T if roll else 1
    assert T * E * g.N * max(8, 2 * g.window * g.window) < 2 ** 31 and T * E * g.H * g.W < 2 ** 31, \
        "fits32 false is out of scope"
    has = outs.__contains__
    primal = has("obs_primal") or has("primal_vec")
    d = dict(path="generic", fullw=False, runner=False, split=False, short_t=roll and T <= AB_SHORT_T,
             staged=False, split_lds=0, lds=g.gen_lds, action_path=0)
    if g.wave_ok and not primal and not (has("obs_window") and has("obs_window_occ")):
        fullw = g.N == g.L and E % g.EPW == 0
        occ = has("obs_window_occ")
        win_out = has("obs_window") or occ
        runner = roll and all(has(k) for k in RUNNER_KEYS) and win_out and not has("obs_full")
        split_lds = split_lds_of(g, occ)
        split = (runner and fullw and g.L in (16, 64) and g.wv_split_ok and split_lds <= 64 * 1024
                 and out_aligned)
        WIN = g.window if win_out else 0
        short_t = roll and T <= AB_SHORT_T
        args = None
        if WIN in (0, 3, 5, 7):                        # pick_wave_kernel / pick_wave_win
            if occ:
                if WIN > 0 and roll and runner and split:
                    args = (WIN, True, True, True, g.L, True, True, 8 if short_t else 0)
            elif roll and runner:
                if WIN > 0 and split:
                    args = (WIN, True, True, True, g.L, True, False, 8 if short_t else 0)
                elif not fullw:
                    args = (WIN, True, False, True, 0, False, False, 0)
                else:
                    args = (WIN, True, True, True, g.L if g.L in (16, 64) else 0, False, False, 0)
            elif roll:
                args = (WIN, True, fullw, False, 0, False, False, 0)
            else:
                args = (WIN, False, fullw, False, 16 if fullw and g.L == 16 else 0, False, False, 0)
        if args is not None:
            stage_lds = split_lds + 16 + 64 * T
            resident = lambda lds: min(SPLIT_WG_PER_CU, 160 * 1024 // lds)  # noqa: E731
            staged = (split and act == "int8" and act_aligned and 1 <= T <= SPLIT_STAGE_MAX_T
                      and stage_lds <= 64 * 1024 and resident(stage_lds) == resident(split_lds))
            d.update(path="wave", fullw=fullw, runner=runner, split=split, staged=staged,
                     split_lds=split_lds, lds=stage_lds if staged else split_lds if split else g.wv_lds,
                     action_path=2 if staged else 1 if split and act != "gen" else 0,
                     kernel=("mapf_wave_kernel", ",".join(_b(v) if isinstance(v, bool) else str(v)
                                                           for v in args)))
            return d
    feat = FEAT_FULL | FEAT_PRIM if primal else FEAT_FULL if has("obs_full") else 0
    if (roll and feat == 0 and all(has(k) for k in RUNNER_KEYS)
            and (has("obs_window") or has("obs_window_occ")) and not has("reward_f32")):
        feat = FEAT_RUN
    d["runner"] = feat == FEAT_RUN
    d["kernel"] = ("mapf_rollout_kernel" if roll else "mapf_step_kernel",
                   "%s,%d,%d" % ("unsignedchar" if g.es == 1 else "unsignedshort", g.APL, feat))
    return d


def kernel_args(printed):
    """(name, template arguments without spaces) of a mapfx_last_kernel string."""
    m = re.search(r"(mapf_(?:wave|step|rollout)_kernel)<([^>]*)>", printed)
    return (m.group(1), m.group(2).replace(" ", "")) if m else None


def find_nosplit_shape(L):
    """The smallest-area map with H != W, neither a multiple of 8, on which an L = N runner
    rollout keeps the wave path but its split needs more than 64 KB of LDS, at windows 3, 5
    and 7 alike."""
    best = None
    for H in range(9, 200):
        for W in (H + 3, H - 2):
            if H % 8 == 0 or W % 8 == 0:
                continue
            gs = [geometry(H, W, L, w) for w in (3, 5, 7)]
            if all(g.wave_ok and split_lds_of(g, True) > 64 * 1024 for g in gs) \
                    and (best is None or H * W < best[0] * best[1]):
                best = (H, W)
        if best:
            return best
    raise AssertionError("no such shape")


def find_fold8_shape(N):
    """The smallest H x (H + 3) map on which a generic rollout of N > 128 agents (one env per
    block, L = 256) folds its rewards deferred (fold_R = 8): the ring fits without costing a
    resident block."""
    for H in range(9, 300):
        g = geometry(H, H + 3, N, 5)
        if g is not None and g.EPB == 1 and g.fold_R == 8:
            return (H, H + 3)
    raise AssertionError("no such shape")


# the input domain ALL_KERNELS is enumerated over: every lane group and cell width, maps that
# take the fast builder, the fallback, no wave path (pitch >= 256) and too much LDS for the
# split, every window class, every output selection that changes a decision
DOMAIN = dict(
    N=(1, 2, 3, 4, 8, 16, 32, 33, 64, 65, 127, 128, 129, 256, 257, 512, 513, 769, 1024),
    HW=((6, 7), (5, 65), (3, 250), find_nosplit_shape(16), find_nosplit_shape(64)),
    window=(1, 3, 4, 5, 7, 9),
    obs=(("full",), ("window",), ("window_occ",), ("window", "window_occ"), ("full", "window"),
         ("primal", "window"), ("full", "primal")),
    launch=(("observe", None), ("step", None), ("rollout", None), ("rollout", "runner"),
            ("rollout", "no-window")),
    T=(1, 33), partial_wave=(False, True), out_aligned=(True, False))


def mode_of(obs):
    m = 0
    for k in obs:
        m |= OBS_MODES[k]
    return m


def batch_keys(obs):
    return STEP_KEYS + tuple(k for kind in obs for k in KIND_KEYS[kind])


def launch_outs(obs, entry, select=None):
    """The non-NULL outputs of a launch through MapfGridBatch: step() and observe() pass the
    batch's own buffers, rollout() the trajectory's; `select` None: all of them, "runner":
    the runner output set (no f32 reward, no full map), "no-window": all but the windows,
    or an explicit tuple."""
    keys = batch_keys(obs) + (TRAJ_KEYS if entry == "rollout" else ())
    if select == "runner":
        keys = tuple(k for k in keys if k in RUNNER_KEYS or k in ("obs_window", "obs_window_occ"))
    elif select == "no-window":
        keys = tuple(k for k in keys if k not in ("obs_window", "obs_window_occ"))
    elif select is not None:
        assert set(select) <= set(keys), (select, keys)
        keys = tuple(select)
    if entry == "observe":
        keys = tuple(k for k in keys if k in OBS_KEYS)
    return keys


@functools.lru_cache(maxsize=None)
def _enumerate():
    seen = set()
    D = DOMAIN
    for N, (H, W), win, obs in itertools.product(D["N"], D["HW"], D["window"], D["obs"]):
        g = geometry(H, W, N, win, 10, mode_of(obs))
        if g is None:
            continue
        for (entry, sel), T, part, al in itertools.product(D["launch"], D["T"], D["partial_wave"],
                                                           D["out_aligned"]):
            E = 4 * 64 + (1 if part else 0)
            seen.add(dispatch(g, E, entry, T, launch_outs(obs, entry, sel), al)["kernel"])
    return frozenset(seen)


ALL_KERNELS = _enumerate()
WAVE_KERNELS = frozenset(k for k in ALL_KERNELS if k[0] == "mapf_wave_kernel")
GENERIC_KERNELS = ALL_KERNELS - WAVE_KERNELS
# what csrc/mapfx.hip instantiates (pick_wave_win, pick_kernel_c) -- written out, to name
# the instances no input reaches
COMPILED_WAVE = frozenset(
    ("mapf_wave_kernel", "%d,%s" % (w, a)) for w in (0, 3, 5, 7) for a in
    ["false,true,false,16,false,false,0", "false,true,false,0,false,false,0",
     "false,false,false,0,false,false,0", "true,true,false,0,false,false,0",
     "true,false,false,0,false,false,0", "true,false,true,0,false,false,0",
     "true,true,true,16,false,false,0", "true,true,true,64,false,false,0",
     "true,true,true,0,false,false,0"]
    + (["true,true,true,%d,true,%s,%d" % (ll, o, ab) for ll in (16, 64) for o in ("false", "true")
        for ab in (8, 0)] if w else []))
COMPILED_GENERIC = frozenset(
    [("mapf_step_kernel", "%s,%d,%d" % (c, a, f)) for c in ("unsignedchar", "unsignedshort")
     for a in (1, 2, 4) for f in (0, 2, 3)]
    + [("mapf_rollout_kernel", "%s,%d,%d" % (c, a, f)) for c in ("unsignedchar", "unsignedshort")
       for a in (1, 2, 4) for f in (0, 2, 3, 4)])
UNREACHABLE = (COMPILED_WAVE | COMPILED_GENERIC) - ALL_KERNELS


# --------------------------------------------------------------------------- cases
Case = namedtuple("Case", "name H W N E entry T window psize obs select act act_off misalign "
                          "shared track autoreset rewards env_offset t0 seed dense")


def _c(name, H, W, N, E, entry, T, window=5, psize=10, obs=("window",), select=None, act="int8",
       act_off=0, misalign=None, shared=False, track=True, autoreset=False,
       rewards=DEFAULT_REWARDS, env_offset=0, t0=0, seed=0, dense=0):
    """act: "gen" (rollouts: the device generator) or the buffer's dtype; act_off: the byte
    offset of the action buffer inside a 16-byte aligned allocation; misalign: a trajectory
    output whose pointer is moved one byte; dense = d: every unscripted agent starts inside one
    block of d + 1 rows and d columns, several to a cell (stacked swaps: edge counts of 4 and more)."""
    return Case(name, H, W, N, E, entry, T, window, psize, tuple(obs), select, act,
                act_off if act == "int8" else 0, misalign, shared, track, autoreset, tuple(rewards),
                env_offset, t0, seed, dense)


DEAD_TAIL_T = (6, 9, 15, 18, 40)


def limit_of(c):
    """episode_limit.  Per-step launches and autoreset rollouts: two steps short of the
    episode (T >= 5), so it ends, and then goes on finished or starts again.  A rollout
    without autoreset ends every env AT its last step (limit = T: each step of the launch,
    the last action block included, moves live agents) unless T is one of DEAD_TAIL_T, where
    the last two steps run on finished envs."""
    if c.entry == "rollout" and not c.autoreset and c.T not in DEAD_TAIL_T:
        return c.T
    return c.T - 2 if c.T >= 5 else 3 if c.T == 4 else 2


def case_geometry(c):
    return geometry(c.H, c.W, c.N, c.window, c.psize, mode_of(c.obs), c.rewards)


def case_launches(c):
    """[(entry, dispatch result)] of the distinct launches a case makes: reset()'s observe
    launch, then its entry point's."""
    g = case_geometry(c)
    out = [("observe", dispatch(g, c.E, "observe", 1, launch_outs(c.obs, "observe")))]
    if c.entry != "observe":
        out.append((c.entry, dispatch(g, c.E, c.entry, c.T, launch_outs(c.obs, c.entry, c.select),
                                      c.misalign is None, c.act, c.act_off % 16 == 0)))
    return out


def expected_kernel(c, entry=None):
    """The instance of a case's `entry` launch (default: its own entry point)."""
    return dict(case_launches(c))[entry or c.entry]["kernel"]


def expected_action_path(c):
    return dict(case_launches(c))[c.entry]["action_path"]


SPLIT_T = (1, 2, 15, 16, 32, 33, 40)
GENERIC_T = (1, 3, 4, 5, 13)


def _cases():
    out = []
    add = lambda *a, **k: out.append(_c(*a, **k))  # noqa: E731
    # ---- wave kernel, observe / step: <WIN,false,FULLW,false,LL>.  Lane groups 1..64, full
    # and partial; E with a partial last wave where the instance allows one (fullw needs
    # E % EPW == 0); W <= 64 (fast builder) and W >= 65 (fallback); WIN 0 = no window output
    lanes = ((1, 6, 7, 131), (2, 7, 5, 67), (3, 5, 9, 37), (4, 9, 6, 32), (8, 7, 11, 19), (16, 5, 65, 12),
             (32, 11, 13, 6), (33, 13, 10, 5), (64, 3, 70, 5))
    for k, (N, H, W, E) in enumerate(lanes):
        win = (3, 5, 7)[k % 3]
        add("wave-step-n%d" % N, H, W, N, E, "step", 6, window=win, obs=("window", "full") if k % 2 else ("window",),
            act=("int8", "int32", "int64")[k % 3], shared=k % 2 == 1, track=k % 4 != 3,
            rewards=ODD_REWARDS if k % 2 else DEFAULT_REWARDS)
    for win in (0, 3, 5, 7):
        obs = ("full",) if win == 0 else ("window", "full")
        w = win or 5
        # <WIN,false,true,false,16>, <WIN,false,true,false,0> (L = 8 full), <WIN,false,false,false,0>
        add("wave-step-w%d-l16" % win, 7, 9 + win, 16, 8, "step", 4, window=w, obs=obs, act="int64")
        add("wave-obs-w%d-l16" % win, 9 + win, 7, 16, 8, "observe", 3, window=w, obs=obs, shared=True)
        add("wave-step-w%d-l8" % win, 6, 67, 8, 16, "step", 4, window=w, obs=obs, act="int32",
            rewards=ODD_REWARDS)
        add("wave-step-w%d-part" % win, 11, 6, 13, 9, "step", 4, window=w, obs=obs)
        add("wave-obs-w%d-part" % win, 5, 66, 16, 9, "observe", 3, window=w, obs=obs)
        # ---- non-runner rollouts <WIN,true,FULLW,false,0>: every output (the full map keeps
        # the launch off the runner instances), generator and buffers
        add("wave-roll-w%d-full" % win, 7, 10, 4, 32, "rollout", 9, window=w, obs=obs, act="gen",
            env_offset=1000, t0=3, seed=99, autoreset=win == 5)
        add("wave-roll-w%d-fb" % win, 5, 65, 16, 8, "rollout", 7, window=w, obs=obs, act="int8", act_off=3)
        add("wave-roll-w%d-part" % win, 10, 7, 5, 21, "rollout", 7, window=w, obs=obs, act="int32",
            shared=True, rewards=ODD_REWARDS, autoreset=win == 3)
    # ---- the full map on a width that is a multiple of 4 (its rows leave as whole words, the
    # row of a word found with m_W4, not m_W), non-square, both builders, W / 4 = 1
    add("wave-full-w12", 7, 12, 16, 9, "step", 4, obs=("window", "full"), act="int32")
    add("wave-full-w4", 9, 4, 3, 70, "step", 4, window=3, obs=("full", "window"), shared=True)
    add("wave-full-w68-roll", 5, 68, 8, 16, "rollout", 6, obs=("full",), act="int8", act_off=2)
    add("wave-full-w20-obs", 6, 20, 33, 6, "observe", 3, window=7, obs=("full", "window"))
    # ---- runner rollouts that do not split: <WIN,true,false,true,0> (partial), <..,true,true,{16,64,0}>
    big16, big64 = find_nosplit_shape(16), find_nosplit_shape(64)
    for k, win in enumerate((3, 5, 7)):
        add("run-w%d-part" % win, 9, 6, 12, 11, "rollout", 9, window=win, select="runner", act="int8",
            act_off=5, autoreset=k == 0)
        add("run-w%d-part-fb" % win, 5, 66, 16, 7, "rollout", 6, window=win, select="runner", act="int64")
        add("run-w%d-l8" % win, 6, 7, 8, 16, "rollout", 9, window=win, select="runner", act="gen", seed=5,
            t0=2, env_offset=77)
        add("run-w%d-l32-fb" % win, 3, 69, 32, 6, "rollout", 6, window=win, select="runner", act="int32",
            rewards=ODD_REWARDS)
        # L = 16 / 64 with every lane group full, kept off the split by a `node` pointer one
        # byte off, and by a map whose split LDS passes 64 KB while the wave layout fits
        add("run-w%d-l16-misal" % win, 7, 10, 16, 8, "rollout", 9, window=win, misalign="node",
            act="int8", shared=True)
        add("run-w%d-l64-misal" % win, 5, 67, 64, 5, "rollout", 7, window=win, misalign="node", act="int8",
            act_off=8, autoreset=True)
        add("run-w%d-l16-lds" % win, big16[0], big16[1], 16, 8, "rollout", 5, window=win, act="int32")
        add("run-w%d-l64-lds" % win, big64[0], big64[1], 64, 5, "rollout", 5, window=win, act="gen", seed=3)
    # ---- the split: <WIN,true,true,true,LL,true,OCC,ABT>, T on both sides of the ABT
    # boundary (32 | 33) and of the preloaded "T >= 16" bit (15 | 16), the pipeline's fill and
    # drain (1, 2); per pair the fast builder and the fallback (W >= 65: the M0 -> M1 copy),
    # the three action paths (staged; a buffer off 16 bytes, int32, int64: register blocks;
    # the generator), autoreset, both reward pairs, shared maps, untracked steps
    shapes = {16: ((7, 10), (5, 65), (10, 7), (6, 66)), 64: ((9, 11), (3, 70), (11, 9), (5, 67))}
    acts = (("int8", 0), ("int8", 1), ("gen", 0), ("int32", 0), ("int8", 0), ("int64", 0), ("int8", 8))
    i = 0
    for win in (3, 5, 7):
        for LL in (16, 64):
            for occ in (False, True):
                for j, T in enumerate(SPLIT_T):
                    H, W = shapes[LL][(i + j) % 4]
                    act, off = acts[(i + j) % 7]
                    add("split-w%d-l%d-%s-T%d" % (win, LL, "occ" if occ else "win", T), H, W, LL,
                        12 if LL == 16 else 5, "rollout", T, window=win,
                        obs=("window_occ",) if occ else ("window",), act=act, act_off=off,
                        autoreset=(i + j) % 3 == 1, rewards=ODD_REWARDS if (i + j) % 2 else DEFAULT_REWARDS,
                        shared=(i + j) % 5 == 0, track=(i + j) % 4 != 2, seed=11 + i, t0=j,
                        env_offset=100 * j)
                i += 1
    # T = 17: the short launches' third 8-step action block holds one step -- register blocks
    # only (a staged or generated launch fetches no block)
    for k, (win, LL, occ) in enumerate(itertools.product((3, 5, 7), (16, 64), (False, True))):
        H, W = shapes[LL][(k + 1) % 4]
        act, off = (("int8", 1), ("int32", 0), ("int64", 0), ("int8", 8))[k % 4]
        add("split-w%d-l%d-%s-T17" % (win, LL, "occ" if occ else "win"), H, W, LL, 12 if LL == 16 else 5,
            "rollout", 17, window=win, obs=("window_occ",) if occ else ("window",), act=act, act_off=off,
            autoreset=k % 3 == 2, rewards=ODD_REWARDS if k % 2 else DEFAULT_REWARDS)
    # every action path at both lane groups on one shape each (the dtype rotation above
    # decides the rest): the staged buffer, and the same bytes one byte in
    for LL, (H, W) in ((16, (6, 66)), (64, (3, 70))):
        for off in (0, 1):
            add("split-l%d-act-off%d" % (LL, off), H, W, LL, 8 if LL == 16 else 5, "rollout", 20,
                act="int8", act_off=off, autoreset=off == 1)
    # ---- generic kernel, one-byte cells (N <= 127: L <= 128, APL 1) -- FEAT 0 / FULL /
    # FULL|PRIM / RUN.  N <= 64 lands here through a window the wave path refuses (1, 4, 9),
    # the occupancy window on a step, both window formats at once, PRIMAL outputs, or a
    # pitch >= 256; N = 65 and 127 always
    add("gen8-w1-n3", 6, 9, 3, 70, "step", 5, window=1, act="int64")
    add("gen8-w4-n16", 9, 6, 16, 21, "step", 5, window=4, obs=("window", "full"), act="int32")
    add("gen8-w9-n33", 7, 12, 33, 9, "step", 5, window=9, shared=True, rewards=ODD_REWARDS)
    add("gen8-occ-step-n16", 7, 10, 16, 20, "step", 5, obs=("window_occ",))
    add("gen8-both-n8", 10, 7, 8, 35, "step", 5, window=3, obs=("window", "window_occ"), track=False)
    add("gen8-pitch256-n16", 3, 250, 16, 21, "step", 5, obs=("window", "full"), act="int32")
    add("gen8-pitch256-n64-roll", 3, 250, 64, 5, "rollout", 7, select="runner", act="int8", act_off=1)
    add("gen8-primal-n12", 9, 13, 12, 23, "step", 5, psize=10, obs=("primal", "window"))
    add("gen8-primal-odd-n5", 11, 6, 5, 53, "observe", 3, psize=7, window=7, obs=("primal", "full"))
    add("gen8-n65-step", 7, 9, 65, 5, "step", 5, obs=("window",))
    add("gen8-n127-full", 9, 14, 127, 5, "step", 5, obs=("full", "window_occ"), act="int64",
        rewards=ODD_REWARDS)
    add("gen8-n127-obs", 14, 9, 127, 5, "observe", 3, window=3)
    add("gen8-full-w12", 9, 12, 70, 5, "step", 4, obs=("full", "window"))         # full rows as words
    add("gen8-full-w20-roll", 6, 20, 100, 5, "rollout", 6, obs=("full",), act="int32", autoreset=True)
    add("gen8-full-w4-w9", 11, 4, 5, 40, "step", 4, window=9, obs=("full", "window"))
    for T in GENERIC_T:       # the generic rollout's 4-step action blocks, every dtype
        k = GENERIC_T.index(T)
        add("gen8-n65-roll-T%d" % T, 9, 7, 65, 7, "rollout", T, obs=("window_occ",),
            act=("int8", "int32", "int64", "int8", "int8")[k], act_off=(0, 0, 0, 1, 2)[k],
            autoreset=T == 13)
    add("gen8-n100-full-roll", 6, 11, 100, 6, "rollout", 9, obs=("full", "window"), act="gen", seed=8,
        t0=5, env_offset=31)
    add("gen8-n12-primal-roll", 13, 9, 12, 23, "rollout", 9, psize=5, obs=("primal",), act="int8",
        act_off=7, autoreset=True)
    add("gen8-w9-n64-run", 7, 13, 64, 6, "rollout", 10, window=9, select="runner", act="int32",
        rewards=ODD_REWARDS)
    # one env per block at L = 64 (the map's LDS): the deferred fold (fold_R = 8), past 8 and 16 steps
    add("gen8-l64-epb1-run", 150, 163, 64, 5, "rollout", 19, window=9, select="runner", act="int8",
        act_off=1, rewards=ODD_REWARDS)
    add("gen8-l128-epb1", 131, 190, 100, 5, "rollout", 18, obs=("window_occ",), act="gen", seed=2)
    # ---- generic kernel, two-byte cells: APL 1 (N = 128, 129, 256), 2 (257, 512), 4 (513,
    # 769 = APL 3 rounded up, 1024).  One env per block: every rollout folds deferred
    # (fold_R = 8) unless the ring would cost a resident block (fold_R = 0)
    wide = ((128, 9, 14, 5), (129, 13, 10, 5), (256, 5, 66, 5), (257, 10, 13, 5), (512, 13, 18, 5),
            (513, 14, 19, 5), (769, 19, 14, 5), (1024, 21, 26, 5))
    for k, (N, H, W, E) in enumerate(wide):
        add("gen16-n%d-step" % N, H, W, N, E, "step", 4, window=(5, 3, 7)[k % 3],
            obs=(("window",), ("window_occ", "full"), ("window", "window_occ"))[k % 3],
            act=("int8", "int32", "int64")[k % 3], shared=k % 2 == 0,
            rewards=ODD_REWARDS if k % 2 else DEFAULT_REWARDS, track=k % 4 != 1)
        add("gen16-n%d-run" % N, W, H, N, E, "rollout", (9, 18, 5)[k % 3], window=(3, 5, 7)[k % 3],
            obs=("window_occ",) if k % 2 else ("window",), select="runner",
            act=("int8", "gen", "int32", "int64")[k % 4], act_off=k % 3, seed=k, t0=k,
            autoreset=k % 3 == 0, rewards=DEFAULT_REWARDS if k % 2 else ODD_REWARDS)
    for k, N in enumerate((200, 300, 700)):          # FEAT 0 / FULL / FULL|PRIM at APL 1, 2, 4
        H, W = ((12, 17), (17, 12), (15, 18))[k]
        add("gen16-n%d-full-step" % N, H, W, N, 5, "step", 4, obs=("full", "window"), act="int32")
        add("gen16-n%d-primal-step" % N, W, H, N, 5, "observe", 2, psize=(10, 11, 3)[k],
            obs=("primal", "window_occ"))
        add("gen16-n%d-roll" % N, H, W, N, 5, "rollout", 9, obs=("window_occ",), act="int8",
            act_off=(0, 1, 3)[k], rewards=ODD_REWARDS)
        add("gen16-n%d-full-roll" % N, W, H, N, 5, "rollout", 6, obs=("full",), act="gen", seed=4 + k)
        add("gen16-n%d-primal-roll" % N, H, W, N, 5, "rollout", 5, psize=(3, 10, 11)[k], obs=("primal", "window"),
            act="int64", autoreset=True)
    # the deferred fold at L = 256 takes a map large enough for the ring not to cost a resident
    # block; every small map above keeps the per-step fold (fold_R = 0) with finite rewards
    # (dense starts: stacked swaps with edge counts >= 4, the rows the fold adds without its table)
    for k, N in enumerate((256, 600)):
        H, W = find_fold8_shape(N)
        add("gen16-n%d-fold8-dense" % N, H, W, N, 5, "rollout", 11, obs=("window_occ",), select="runner",
            act=("int8", "int64")[k], dense=6, rewards=(DEFAULT_REWARDS, ODD_REWARDS)[k])
    add("gen8-l64-epb1-dense", 150, 163, 64, 5, "rollout", 10, window=9, select="runner", act="int32", dense=2)
    for k, N in enumerate((256, 300, 600)):
        H, W = find_fold8_shape(N)
        add("gen16-n%d-fold8" % N, (H, W)[k % 2], (W, H)[k % 2], N, 5, "rollout", (19, 10, 18)[k],
            obs=("window_occ",) if k else ("window",), select=None if k == 1 else "runner",
            act=("int8", "int32", "gen")[k], act_off=k == 0, seed=6, t0=1, env_offset=9,
            rewards=ODD_REWARDS if k != 1 else DEFAULT_REWARDS, autoreset=k == 2)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def case_id(c):
    return "%s-%dx%d-N%d-E%d-T%d" % (c.name, c.H, c.W, c.N, c.E, c.T)


# --------------------------------------------------------------------------- instances
def pack_bits(grids):
    """[V, H, W] (nonzero = obstacle) -> [V, mapfx_map_stride] bitmaps, bit r * W + c LSB first."""
    V, H, W = grids.shape
    out = np.zeros((V, corc.stride(H, W)), np.uint8)
    for v in range(V):
        pb = np.packbits((grids[v] != 0).reshape(-1), bitorder="little")
        out[v, :pb.size] = pb
    return out


@functools.lru_cache(maxsize=None)
def grid_of(H, W, variant):
    """~12 % obstacles, the four corners free, at least one obstacle with a free neighbour."""
    rng = np.random.default_rng([H, W, variant, 11])
    g = (rng.random((H, W)) < 0.12).astype(np.int8)
    for r, c in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        g[r, c] = 0
    g[H // 2, W // 2] = g[H // 2, W // 2 + 1] = 1      # two obstacles, the first with a free neighbour
    g[H // 2, W // 2 - 1] = 0
    g.setflags(write=False)
    return g


ROLES = ("top", "bottom", "left", "right", "obstacle", "on-obstacle", "stacked",
         "corner-tl", "corner-tr", "corner-bl", "corner-br")


def role_slots(N):
    """(env, agent) of the roles: env 3 onwards, N per env."""
    return [(3 + k // N, k % N) for k in range(len(ROLES))]


def min_envs(N):
    return role_slots(N)[-1][0] + 2      # + one env for the action outside 0..4


def _free(g):
    return [(int(r), int(c)) for r, c in np.argwhere(g == 0)]


def _nbrs(g, p):
    H, W = g.shape
    return [(a, (p[0] + dr, p[1] + dc)) for a, (dr, dc) in enumerate(DELTAS[:4])
            if 0 <= p[0] + dr < H and 0 <= p[1] + dc < W]


def _role(rng, g, role, stood_on):
    """(start, {step: action}) of a role; "stacked" (start None) takes its left neighbour's
    start once every other start is set (N = 1 has nobody to stack on); `stood_on`: the
    obstacle the env's "on-obstacle" agent starts on -- enterable while it stands there
    (quirk 1), so the "obstacle" bump aims at another one."""
    H, W = g.shape
    free = _free(g)
    pick = lambda cells: cells[int(rng.integers(len(cells)))]  # noqa: E731
    if role in ("top", "bottom", "left", "right"):
        a = ("top", "bottom", "left", "right").index(role)
        line = [p for p in free if (p[0] == 0, p[0] == H - 1, p[1] == 0, p[1] == W - 1)[a]]
        return pick(line), {0: a}
    if role == "obstacle":
        opts = [(p, a) for p in free for a, q in _nbrs(g, p) if g[q] != 0 and q != stood_on]
        p, a = pick(opts)
        return p, {0: a}
    if role == "on-obstacle":
        return stood_on, {0: 4}
    if role == "stacked":
        return None, {0: 4}
    r, c = {"tl": (0, 0), "tr": (0, W - 1), "bl": (H - 1, 0), "br": (H - 1, W - 1)}[role[-2:]]
    return (r, c), {0: 0 if r == 0 else 1, 1: 2 if c == 0 else 3}


BAD = {"int8": (5, -1, 127), "int32": (-2 ** 31, 5, -1), "int64": (2 ** 32 + 2, -1, 5)}
SNAP_STATE = ("pos", "done", "t", "steps")


def _observe(ob, c):
    o = ob.observe(window=c.window, psize=c.psize, full=True, win=True, primal="primal" in c.obs)
    w = o["obs_window"]
    o["obs_window_occ"] = (w[:, :, 1] - w[:, :, 0]).astype(w.dtype)
    return o


def _snapshot(ob, c, stepped=None):
    s = {k: getattr(ob, k).copy() for k in SNAP_STATE}
    s.update(_observe(ob, c))
    if stepped is not None:
        s.update(reward=stepped["reward"], reward_f32=stepped["reward"].astype(np.float32),
                 node=stepped["node"], edge=stepped["edge"], traj_pos=s["pos"], traj_done=s["done"],
                 traj_t=s["t"])
    return s


def make_oracle(c, b):
    return corc.OracleBatch(b["bits"], b["init_pos"], b["goals"], c.H, c.W, limit=limit_of(c),
                            step_reward=c.rewards[0], collide_reward=c.rewards[1],
                            env_offset=c.env_offset, nthreads=2)


def autoreset(ob, term):
    """mapf_gridworld.py:70-83 for the envs whose episode ended."""
    m = term.astype(bool)
    ob.pos[m] = ob.init_pos[m]
    ob.done[m] = 0
    ob.t[m] = 0
    ob.steps[m] = 0


def episode(c, b, actions, start=None, refuse=False, count=None):
    """The oracle's episode of the instance `b` (bits, init_pos, goals of `build`) under
    `actions` [T, E, N]: the loop `build` itself runs, and what tests/graph_replay_cases.py
    runs for further episodes of a built case.  Returns (snaps, final, bad): snaps[0] after
    reset() and snaps[k + 1] after step k (before an autoreset), final = the state after the
    last step's autoreset, bad = (step, env, agent) of the refused action or None.
    start: [E, N, 2] positions the episode begins from in place of init_pos, as
    set_positions leaves them after a reset (done, t and steps zero; an autoreset still
    returns an env to init_pos).  refuse: write an action outside 0..4 into `actions`
    (then modified in place) at step min(1, T - 1) for the last live env behind the roles.
    count = (bumps [T, 5], stats): filled with what the coverage test counts."""
    N, E, T, H, W = c.N, c.E, c.T, c.H, c.W
    assert actions.shape == (T, E, N), (actions.shape, (T, E, N))
    variant = (lambda e: 0) if c.shared else (lambda e: e % VARIANTS)
    limit = limit_of(c)
    ob = make_oracle(c, b)
    if start is not None:
        ob.pos[...] = start
    snaps = [_snapshot(ob, c)]
    bumps, stats = count if count is not None else (None, None)
    tb = min(1, T - 1)
    bad = None
    for t in range(T):
        if t == tb and refuse:
            cand = [e for e in range(role_slots(N)[-1][0] + 1, E) if not ob.done[e].all()]
            assert cand, "no live env for the refused action"
            be = cand[-1]
            ba = (0, N // 2, N - 1)[(N + E) % 3]
            actions[t, be, ba] = BAD[c.act][(N + T) % 3]
            bad = (t, be, ba)
        if count is not None:
            stats["past_done"] += int(ob.done.all(1).sum())
            if t == T - 1:
                stats["live_last"] = int((~ob.done.all(1)).sum()) - (1 if bad and bad[0] == t else 0)
        for e in range(E if count is not None else 0):
            g = grid_of(H, W, variant(e))
            if bad and bad[:2] == (t, e):
                continue
            cnt = np.zeros((H, W), np.int64)
            np.add.at(cnt, (ob.pos[e, :, 0], ob.pos[e, :, 1]), 1)
            for i in range(N):
                a = int(actions[t, e, i])
                if ob.done[e, i] or a == 4:
                    continue
                r, col = ob.pos[e, i] + DELTAS[a]
                if not (0 <= r < H and 0 <= col < W):
                    bumps[t, a] += 1
                elif g[r, col] != 0 and cnt[r, col] == 0:
                    bumps[t, 4] += 1
        a = actions[t]      # 2^32 + 2 must not wrap into 0..4 on its way to the oracle's int32
        stepped = ob.step(np.where((a < 0) | (a > 4), 7, a).astype(np.int32))
        assert stepped["bad"] == (1 if bad and bad[0] == t else 0)
        s = _snapshot(ob, c, stepped)
        snaps.append(s)
        if count is not None:
            stats["node"] = max(stats["node"], int(stepped["node"].sum(1).max()))
            stats["edge"] = max(stats["edge"], int(stepped["edge"].max()))
            newly = s["term"].astype(bool) & ~snaps[-2]["term"].astype(bool) if t else s["term"].astype(bool)
            stats["done_below"] += int((newly & (ob.t < limit)).sum())
            stats["done_at"] += int((newly & (ob.t >= limit)).sum())
        if c.autoreset:
            if count is not None:
                stats["resets"] += int(s["term"].sum())
            autoreset(ob, s["term"])
    final = {k: getattr(ob, k).copy() for k in SNAP_STATE}
    for v in [x for s in snaps for x in s.values()] + list(final.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return snaps, final, bad


@functools.lru_cache(maxsize=None)
def build(c):
    """A case's maps, instance, actions and the oracle's episode, built once per process and
    read-only: grids [1 | E, H, W], bits, init_pos / goals [E, N, 2], actions [T, E, N] int64
    (the generator's for act = "gen"), bad = (step, env) of the refused action or None,
    snaps[0] after reset() and snaps[k + 1] after step k (before an autoreset), final = the
    state after the last step's autoreset, and what the coverage test counts: per step the
    env collisions by kind (bumps [T, 5]: four borders, obstacle), node and edge maxima,
    terminations below and at the limit, resets, the envs still live at the last step."""
    N, E, T, H, W = c.N, c.E, c.T, c.H, c.W
    assert T >= 1 and E >= min_envs(N), (c, min_envs(N))
    rng = np.random.default_rng([H, W, N, E, T, c.window, len(c.name), c.seed])
    variant = (lambda e: 0) if c.shared else (lambda e: e % VARIANTS)
    nv = 1 if c.shared else E
    grids = np.stack([grid_of(H, W, variant(e)) for e in range(nv)])
    actions = rng.integers(0, 5, size=(T, E, N)).astype(np.int64)
    init = np.zeros((E, N, 2), np.int32)
    goals = np.zeros((E, N, 2), np.int32)
    scripts = {}
    slots = dict(zip(role_slots(N), ROLES))
    for e in range(E):
        g = grid_of(H, W, variant(e))
        free = _free(g)
        idx = rng.permutation(len(free))[:N] if N <= len(free) else rng.integers(len(free), size=N)
        init[e] = np.array(free, np.int32)[idx]
        if c.dense:
            block = [p for p in free if abs(p[0] - H // 2) <= c.dense // 2 and 2 <= p[1] - W // 2 < 2 + c.dense]
            init[e] = np.array(block, np.int32)[rng.integers(len(block), size=N)]
        goals[e] = np.array(free, np.int32)[rng.integers(len(free), size=N)]
        if e == 0 and N >= 2:
            spots = [x for x in free if sum(g[q] == 0 for _, q in _nbrs(g, x)) >= 3]
            X = spots[int(rng.integers(len(spots)))]
            around = [(a, q) for a, q in _nbrs(g, X) if g[q] == 0]
            (aY, Y), (aA, A), (aB, B) = (around[k] for k in rng.permutation(len(around))[:3])
            first = 0
            away = [p for p in free if p not in (X, Y, A, B)]      # no gadget agent is done early
            goals[e, :3] = np.array(away, np.int32)[rng.integers(len(away), size=min(N, 3))]
            if N >= 3:
                init[e, 0] = Y
                scripts[(e, 0)] = {0: 4, 1: aY ^ 1}
                first = 1
            for k, (cell, a) in enumerate(((A, aA), (B, aB))):   # a ^ 1: towards X; aY: X -> Y
                init[e, first + k] = cell
                scripts[(e, first + k)] = {0: a ^ 1, 1: aY}
        elif e == 1:
            for i in range(N):
                opts = []
                while not opts:
                    s = free[int(rng.integers(len(free)))]
                    opts = [(a, q) for a, q in _nbrs(g, s) if g[q] == 0]
                a, q = opts[int(rng.integers(len(opts)))]
                init[e, i], goals[e, i] = s, q
                scripts[(e, i)] = {0: 4, 1: a}
        else:
            walls = [(int(r), int(col)) for r, col in np.argwhere(g != 0) if (r, col) != (H // 2, W // 2)]
            stood_on = walls[int(rng.integers(len(walls)))]
            for i in range(N):
                if (e, i) in slots:
                    s, script = _role(rng, g, slots[(e, i)], stood_on)
                    if s is not None:
                        init[e, i] = s
                    scripts[(e, i)] = script
            for i in range(N):
                if slots.get((e, i)) == "stacked":
                    init[e, i] = init[e, (i - 1) % N]
    for (e, i), script in scripts.items():
        for t, a in script.items():
            if t < T:
                actions[t, e, i] = a
    b = {"grids": grids, "bits": pack_bits(grids), "init_pos": init, "goals": goals}
    if c.act == "gen":
        lib = corc.lib()
        actions = np.array([[[lib.orc_action(c.seed, c.env_offset + e, c.t0 + t, i) for i in range(N)]
                             for e in range(E)] for t in range(T)], np.int64)
    bumps = np.zeros((T, 5), np.int64)
    stats = dict(node=0, edge=0, done_below=0, done_at=0, resets=0, past_done=0, live_last=0)
    snaps, final, bad = episode(c, b, actions, refuse=c.act != "gen", count=(bumps, stats))
    b.update(actions=actions, bad=bad, snaps=snaps, bumps=bumps, stats=stats, final=final)
    for v in list(b.values()) + [x for s in snaps for x in s.values()] + list(b["final"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return b


# --------------------------------------------------------------------------- comparer
FIELDS = ("pos", "done", "t", "steps", "reward", "reward_f32", "node", "edge", "avail", "term",
          "obs_full", "obs_window", "obs_window_occ", "obs_window_occ_planes", "obs_primal",
          "primal_vec", "traj_pos", "traj_done", "traj_t")
Diff = namedtuple("Diff", "call field env index got want")


def window_planes(occ):
    """[..., w, w] occupancy window -> [..., 2, w, w] {obstacle, agents} planes: what
    mapfx.batch.window_planes computes on the device."""
    return np.stack(((occ == -1).astype(occ.dtype), np.maximum(occ, 0)), axis=-3)


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    if a.dtype == np.float32:
        return a.view(np.uint32).astype(np.int64)
    return a if a.dtype == np.uint64 else a.astype(np.int64)


def compare(got, want, call=None):
    """None when every array of `got` (name -> numpy array: a batch's state arrays, a step's
    outputs, a trajectory slot) equals the oracle snapshot `want` bit for bit, else the first
    difference in FIELDS order as a Diff (index = the flat position inside the env's
    element).  Rewards as fp64 / fp32 bit patterns; obs_window_occ raw and decoded
    (obs_window_occ_planes, from the caller's own decoder, against the oracle's planes; when
    absent it is decoded here)."""
    unknown = set(got) - set(FIELDS)
    assert not unknown, unknown
    got = dict(got)
    if "obs_window_occ" in got and "obs_window_occ_planes" not in got:
        got["obs_window_occ_planes"] = window_planes(np.asarray(got["obs_window_occ"]))
    E = len(want["t"])
    for f in FIELDS:
        if f not in got:
            continue
        w = want["obs_window" if f == "obs_window_occ_planes" else f]
        g, w = _bits(got[f]).reshape(E, -1), _bits(w).reshape(E, -1)
        assert g.shape == w.shape, (f, g.shape, w.shape)
        bad = g != w
        if bad.any():
            e, j = (int(v) for v in np.argwhere(bad)[0])
            return Diff(call, f, e, j, int(g[e, j]), int(w[e, j]))
    return None
