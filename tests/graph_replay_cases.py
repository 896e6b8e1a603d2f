"""The selection and the episodes of the graph-replay tests (tests/test_graph_replay_cases.py on
the CPU, tests/test_gpu_graph_replay.py on the device).  TEST INFRASTRUCTURE ONLY; no test
lives here, and nothing here imports mapfx or torch.

The eager tests launch every kernel instance on the default stream.  The graph-replay tests
capture the same wrapper calls into a HIP graph and replay it with other inputs written in
place, which shows what a default-stream launch cannot: a launch that ignores its `stream`
argument (it runs at capture time and is missing from the graph) and anything fixed at
capture time that should be read at replay time ("Graphs and streams").

Selection.  `CLASSES` names, per family, the launch classes the replay must reach, each as a
predicate over the case tables' own `expected_kernel` / `expected_action_path` / `family`;
`SELECTED` takes the first cases of each table that fill every class (`need` cases per
class, a case counting for every class it belongs to).  No case name is written out here.

Episodes.  `episodes(family, case)` gives three episodes A, B, C of the case's one instance:
  A  the table's scripted episode (`build`), its refused action included;
  B, C  seeded random actions, all valid, through the same oracle and the same code path
     (`episode` of the case module): corc.OracleBatch, partial_step_cases.Ref,
     primal_step_cases.RecordedWorld.
A MAPF rollout on the device generator cannot vary its actions -- seed and t0 are fixed by
the call -- so its three episodes start from three sets of positions instead (`start`:
set_positions outside the graph, no reset() inside it).
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import mapf_step_cases as msc
import partial_step_cases as psc
import primal_step_cases as qsc

FAMILIES = ("mapf", "partial", "primal")
TABLES = {"mapf": msc.CASES, "partial": psc.CASES, "primal": qsc.CASES}
MAX_E, MAX_T = 131, 40      # no selected case is a workload: the tables' own small shapes


# --------------------------------------------------------------------------- classes
def _own(c):
    return dict(msc.case_launches(c))[c.entry]


def _wave(c, entry=None):
    d = _own(c)
    return d["path"] == "wave" and (entry is None or c.entry == entry)


def _split(c):
    return _wave(c, "rollout") and _own(c)["split"]


def _cells(c):
    """Bytes per cell of a generic launch, 0 for a wave launch."""
    d = _own(c)
    return 0 if d["path"] == "wave" else (1 if d["kernel"][1].startswith("unsignedchar") else 2)


def _apl(c):
    return int(_own(c)["kernel"][1].split(",")[1])


def _fold8(c):
    return c.entry == "rollout" and _cells(c) != 0 and msc.case_geometry(c).fold_R == 8


def _primal_ls(c):
    """log2 of the lanes per world of a primal_act_kernel case (None: the seq kernel)."""
    if "primal_act_kernel" not in c.kernel:
        return None
    return int(c.kernel.split("<")[1].split(",")[1])


Class = namedtuple("Class", "family name need pred")
CLASSES = (
    Class("mapf", "wave step, full lane group", 2, lambda c: _wave(c, "step") and _own(c)["fullw"]),
    Class("mapf", "wave step, partial lane group", 2, lambda c: _wave(c, "step") and not _own(c)["fullw"]),
    Class("mapf", "wave observe", 2, lambda c: _wave(c, "observe")),
    Class("mapf", "wave rollout, not runner, device generator, env_offset and t0 non-zero", 1,
          lambda c: _wave(c, "rollout") and not _own(c)["runner"] and c.act == "gen"
          and c.env_offset != 0 and c.t0 != 0),
    Class("mapf", "runner rollout, not split", 2,
          lambda c: _wave(c, "rollout") and _own(c)["runner"] and not _own(c)["split"]),
    Class("mapf", "split rollout, action path 2 (staged int8), 16 lanes", 1,
          lambda c: _split(c) and msc.expected_action_path(c) == 2 and c.N == 16),
    Class("mapf", "split rollout, action path 2 (staged int8), 64 lanes", 1,
          lambda c: _split(c) and msc.expected_action_path(c) == 2 and c.N == 64),
    Class("mapf", "split rollout, action path 1, int8 off alignment", 1,
          lambda c: _split(c) and msc.expected_action_path(c) == 1 and c.act == "int8"),
    Class("mapf", "split rollout, action path 1, int32 or int64", 2,
          lambda c: _split(c) and msc.expected_action_path(c) == 1 and c.act in ("int32", "int64")),
    Class("mapf", "split rollout, action path 0 (generator), 16 lanes", 1,
          lambda c: _split(c) and msc.expected_action_path(c) == 0 and c.N == 16),
    Class("mapf", "split rollout, action path 0 (generator), 64 lanes", 1,
          lambda c: _split(c) and msc.expected_action_path(c) == 0 and c.N == 64),
    Class("mapf", "split rollout with autoreset", 1, lambda c: _split(c) and c.autoreset),
    Class("mapf", "gen8 step", 2, lambda c: c.entry == "step" and _cells(c) == 1),
    Class("mapf", "gen8 rollout", 2, lambda c: c.entry == "rollout" and _cells(c) == 1 and not _fold8(c)),
    Class("mapf", "gen16 step, APL > 1", 1, lambda c: c.entry == "step" and _cells(c) == 2 and _apl(c) > 1),
    Class("mapf", "fold8 rollout", 1, _fold8),
    Class("mapf", "shared map", 1, lambda c: c.shared),
    Class("mapf", "per-env maps", 1, lambda c: not c.shared),
    Class("partial", "fast, u8 tables, sqrt table", 1,
          lambda c: psc.family(c) == "fast" and psc.table_bytes(c.H, c.W) == 1
          and psc.expected_geometry(c)["sqrt_table"] and c.T != 8),
    Class("partial", "fast, int16 tables", 1,
          lambda c: psc.family(c) == "fast" and psc.table_bytes(c.H, c.W) == 2 and c.T != 8),
    Class("partial", "fast, int32 block map (EPW 1)", 1,
          lambda c: psc.family(c) == "fast" and psc.table_bytes(c.H, c.W) == 4
          and psc.expected_geometry(c)["EPW"] == 1),
    Class("partial", "generic instance", 2, lambda c: psc.family(c) == "generic" and c.T != 8),
    Class("partial", "partial_wg_kernel, APL 1", 1,
          lambda c: psc.expected_step_kernel(c)[0] == "partial_wg_kernel"
          and psc.expected_step_kernel(c)[1].endswith(",1") and c.T != 8),
    Class("partial", "partial_wg_kernel, APL > 1", 1,
          lambda c: psc.expected_step_kernel(c)[0] == "partial_wg_kernel"
          and not psc.expected_step_kernel(c)[1].endswith(",1")),
    Class("partial", "partial_bfs_kernel", 1, lambda c: psc.expected_bfs_kernel(c)[0] == "partial_bfs_kernel"),
    Class("partial", "partial_bfs_big_kernel", 1,
          lambda c: psc.expected_bfs_kernel(c)[0] == "partial_bfs_big_kernel"),
    Class("partial", "partial_bfs_huge_kernel", 1,
          lambda c: psc.expected_bfs_kernel(c)[0] == "partial_bfs_huge_kernel"),
    Class("partial", "masked reset (the T = 8 cases of the action and reset tests)", 3, lambda c: c.T == 8),
    Class("primal", "primal_seq_kernel", 1, lambda c: _primal_ls(c) is None and not c.diag),
    Class("primal", "primal_act_kernel, 16 lanes per world", 1, lambda c: _primal_ls(c) == 4 and not c.diag),
    Class("primal", "primal_act_kernel, 64 lanes per world", 1, lambda c: _primal_ls(c) == 6 and not c.diag),
    Class("primal", "diagonal movement", 1, lambda c: c.diag and _primal_ls(c) is not None),
)


def eligible(family, c):
    """Inside the limits of the device runs (E <= 131, T <= 40; a PRIMAL case: every world
    its own).  MAPF: at least two agents -- a lone agent has no node or edge collision and
    its finished env's reward is 0.0 whatever it is told, so its episodes cannot differ in
    any of the three at a last step past the limit."""
    if family == "primal":
        return c.E <= MAX_E and c.pool == 0
    return c.E <= MAX_E and c.T <= MAX_T and (family != "mapf" or c.N >= 2)


@functools.lru_cache(maxsize=None)
def selected():
    """[(family, case)] in class order: per class the first eligible cases of the table that
    bring it to `need`, a case already taken for another class counting."""
    out = []
    for cl in CLASSES:
        have = sum(1 for f, c in out if f == cl.family and cl.pred(c))
        for c in TABLES[cl.family]:
            if have >= cl.need:
                break
            if eligible(cl.family, c) and cl.pred(c) and (cl.family, c) not in out:
                out.append((cl.family, c))
                have += 1
    return tuple(out)


SELECTED = selected()


def of_family(family):
    return [c for f, c in SELECTED if f == family]


def members(cl):
    return [c for f, c in SELECTED if f == cl.family and cl.pred(c)]


def case_id(family, c):
    mod = {"mapf": msc, "partial": psc, "primal": qsc}[family]
    return "%s-%s" % (family, mod.case_id(c))


# --------------------------------------------------------------------------- episodes
NAMES = ("A", "B", "C")
# an episode: what is written into the static buffers (actions; PRIMAL: ids too; start:
# positions set outside the graph, or None), and what the oracle answers (snaps in call
# order; MAPF: final, bad)
Episode = namedtuple("Episode", "name actions ids start snaps final bad")


TRIES = 16


def _rng(family, c, name, what=0):
    return np.random.default_rng([FAMILIES.index(family), TABLES[family].index(c), ord(name), what])


def _distinct(family, c, eps, make):
    """make(try) -> an episode; the first try (0, 1, ...: the draw's seed) that differs from
    every episode of `eps` as tests/test_graph_replay_cases.py asks: in pos and in one of
    reward / node / edge, after step 0 and after the last step.  The small cases that end
    two steps before their last (E = 3 to 5 envs, all finished) need a second or third."""
    for k in range(TRIES):
        ep = make(k)
        if all(separates(differing(family, c, ep, other, at)) for other in eps for at in (0, -1)):
            return ep
    raise AssertionError("no distinct episode for %s in %d tries" % (case_id(family, c), TRIES))


def separates(names):
    return bool({"pos", "traj_pos"} & set(names)) and bool({"reward", "node", "edge"} & set(names))


def _frozen(a):
    a.setflags(write=False)
    return a


def _mapf_start(c, b, rng):
    """[E, N, 2] positions on free cells of each env's own map, several agents to a cell
    allowed (legal state: the table's stacked role starts so)."""
    out = np.zeros((c.E, c.N, 2), np.int32)
    for e in range(c.E):
        free = np.argwhere(b["grids"][0 if c.shared else e] == 0).astype(np.int32)
        out[e] = free[rng.integers(len(free), size=c.N)]
    return out


@functools.lru_cache(maxsize=None)
def mapf_episodes(c):
    b = msc.build(c)
    gen = c.act == "gen"
    eps = [Episode("A", b["actions"], None, b["init_pos"] if gen else None, b["snaps"], b["final"], b["bad"])]

    def make(name, k):
        rng = _rng("mapf", c, name, k)
        if gen:
            acts, start = np.array(b["actions"]), _frozen(_mapf_start(c, b, rng))
        else:
            acts, start = rng.integers(0, 5, size=(c.T, c.E, c.N)).astype(np.int64), None
        snaps, final, bad = msc.episode(c, b, acts, start=start)
        assert bad is None
        return Episode(name, _frozen(acts), None, start, snaps, final, None)

    for name in NAMES[1:]:
        eps.append(_distinct("mapf", c, eps, functools.partial(make, name)))
    return tuple(eps)


def reset_masks(c):
    """The masks of the [T / 2 steps, reset(env_mask), T / 2 steps] graph, one per episode:
    all ones, the irregular mask of the eager masked-reset test, all zeros."""
    irregular = np.zeros(c.E, np.uint8)
    irregular[[0, 1, c.E - 1]] = 1
    irregular[5::7] = 1
    assert 0 < irregular.sum() < c.E
    return {"A": np.ones(c.E, np.uint8), "B": _frozen(irregular), "C": np.zeros(c.E, np.uint8)}


def has_masked_reset(c):
    return c.T == 8


@functools.lru_cache(maxsize=None)
def partial_episodes(c):
    """A, B, C of a MARL_PARTIAL case; a masked-reset case (T = 8) carries reset(env_mask)
    between steps T / 2 - 1 and T / 2 in every episode (`reset_masks`), its snapshot
    inserted there: snaps = [reset, T / 2 steps, masked reset, T / 2 steps]."""
    b = psc.build(c)
    masks = reset_masks(c) if has_masked_reset(c) else None
    eps = []

    def make(name, k):
        acts = np.array(b["actions"]) if name == "A" else \
            _rng("partial", c, name, k).integers(0, 5, size=(c.T, c.E, c.N))
        if masks is None and name == "A":
            snaps = b["snaps"]
        else:
            snaps = psc.episode(c, b, acts, resets=None if masks is None else {c.T // 2: masks[name]})
        return Episode(name, _frozen(acts), None, None, snaps, None, None)

    eps.append(make("A", 0))
    for name in NAMES[1:]:
        eps.append(_distinct("partial", c, eps, functools.partial(make, name)))
    return tuple(eps)


@functools.lru_cache(maxsize=None)
def primal_episodes(c):
    """A, B, C of a PRIMAL case: snaps is ONE dict, every output of every call with a
    leading [E, K] (what primal_step_cases.compare takes), and pos / past after the launch."""
    b = qsc.build(c)
    eps = [Episode("A", b["actions"], b["ids"], None, b, None, None)]

    def make(name, k):
        rng = _rng("primal", c, name, k)
        ids = rng.integers(1, c.N + 1, size=(c.E, c.K)).astype(np.int32)
        acts = rng.integers(0, 9 if c.diag else 5, size=(c.E, c.K)).astype(np.int32)
        return Episode(name, _frozen(acts), _frozen(ids), None, qsc.episode(c, b, (ids, acts)), None, None)

    for name in NAMES[1:]:
        eps.append(_distinct("primal", c, eps, functools.partial(make, name)))
    return tuple(eps)


def episodes(family, c):
    return {"mapf": mapf_episodes, "partial": partial_episodes, "primal": primal_episodes}[family](c)


# ---- the carried-state form: [T steps] without the reset, replayed twice = one 2T episode
def carry_case(family):
    """The case of a family's [T steps] graph: the first selected MAPF wave step case with
    every lane group full / the first selected fast MARL_PARTIAL case."""
    if family == "mapf":
        return next(c for c in of_family("mapf") if _wave(c, "step") and _own(c)["fullw"])
    return next(c for c in of_family("partial") if psc.family(c) == "fast" and not has_masked_reset(c))


@functools.lru_cache(maxsize=None)
def carry_episode(family):
    """(case, limit, episode): 2T steps of seeded valid actions on the case's instance with
    episode_limit raised to `limit` (MAPF: limit_of at 2T steps = 2T - 2; MARL_PARTIAL:
    2T - 1), so that the episode ends inside the SECOND replay."""
    c = carry_case(family)
    T2 = 2 * c.T
    acts = _rng(family, c, "A", 2).integers(0, 5, size=(T2, c.E, c.N)).astype(np.int64)
    if family == "mapf":
        c2 = c._replace(T=T2)
        limit = msc.limit_of(c2)
        snaps, final, _ = msc.episode(c2, msc.build(c), acts)
    else:
        limit = T2 - 1
        snaps, final = psc.episode(c, psc.build(c), acts, limit=limit), None
    return c, limit, Episode("2T", _frozen(acts), None, None, snaps, final, None)


# --------------------------------------------------------------------------- what differs
def mapf_step_arrays(c, snap):
    """The arrays of one MAPF step snapshot that the case's launch writes, in the device's
    shapes: what `compare` is given."""
    keys = msc.launch_outs(c.obs, c.entry, c.select) if c.entry != "observe" else msc.launch_outs(c.obs, "step")
    got = {k: snap[k] for k in keys}
    if c.entry != "rollout":
        got.update({k: snap[k] for k in ("pos", "done", "t")})
        if c.track:
            got["steps"] = snap["steps"]
    return got


def differing(family, c, ea, eb, k):
    """The names of the arrays that differ between two episodes after step k (k = -1: the
    last; PRIMAL: call k of every world)."""
    if family == "primal":
        K = ea.snaps["done"].shape[1]
        k = k % K
        names = [f for f in qsc.FIELDS if not np.array_equal(ea.snaps[f][:, k], eb.snaps[f][:, k])]
        if not np.array_equal(ea.snaps["pos_at"][:, k], eb.snaps["pos_at"][:, k]):
            names.append("pos")
        return names
    sa, sb = ea.snaps[k if k < 0 else k + 1], eb.snaps[k if k < 0 else k + 1]
    fields = msc.FIELDS if family == "mapf" else psc.FIELDS
    return [f for f in fields if f in sa and not np.array_equal(sa[f], sb[f])]
