"""The split rollout's protocol model and checker (tests/split_protocol.py) on the host: the
documented schedule is conflict-free and fresh for every launch length, and each known
way of getting it wrong -- the shipped barrier-T + 1 race first of all -- is flagged for
exactly the lengths at which it is wrong.  No device, no timing."""
import os
import re

import pytest

import split_protocol as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_T = range(1, 131)


def _check(T, staged, **kw):
    return sp.check(sp.model(T, staged, **kw), sp.barriers(T), T)


def _both(T):
    return (False, True) if T <= sp.STAGE_MAX_T else (False,)


def test_numbers_mirror_the_header():
    """RESOURCES / KINDS / SITES are the enums of the probe section of csrc/internal.h."""
    with open(os.path.join(REPO, "mapf-marl_amd", "csrc", "internal.h")) as f:
        text = f.read()
    probe = text[text.index("#ifdef MAPFX_SPLIT_PROBE"):]
    for prefix, names in (("MAPFX_PR_", sp.RESOURCES), ("MAPFX_PK_", sp.KINDS), ("MAPFX_PS_", sp.SITES)):
        found = [m for m in re.findall(r"\b%s([A-Z_0-9]+)\b" % prefix, probe)]
        found = list(dict.fromkeys(found))
        if prefix == "MAPFX_PS_":
            assert found[-1] == "COUNT"
            found = found[:-1]
        assert tuple(found) == tuple(names), prefix
    assert int(re.search(r"#define MAPFX_SPLIT_PROBE_CAP (\d+)", probe).group(1)) == sp.PROBE_CAP
    assert int(re.search(r"#define MAPFX_SPLIT_PROBE_STAGE_FLAGS (\d+)", probe).group(1)) == sp.STAGE_FLAGS
    assert set(sp.STEP_SITES) | set(sp.STORE_SITES) == set(sp.SITES)


def test_probe_library_is_no_product_path():
    """Nothing in the package or the benchmark names the probe library, the shipped
    library's build id does not depend on the probe flag, and all probe code in the kernel
    source sits under the flag."""
    import __graft_entry__ as g
    for root, _, files in os.walk(os.path.join(REPO, "mapf-marl_amd", "mapfx")):
        for name in files:
            if name.endswith(".py"):
                with open(os.path.join(root, name)) as f:
                    assert "mapfx_probe" not in f.read(), name
    with open(os.path.join(REPO, "bench.py")) as f:
        assert "mapfx_probe" not in f.read()
    assert os.path.basename(g.LIB) == "libmapfx.so" and g.PROBE_LIB != g.LIB
    assert g.PROBE_FLAG not in g.HIPCC_FLAGS
    assert g.build_id() != g.build_id((g.PROBE_FLAG,))
    with open(os.path.join(REPO, "mapf-marl_amd", "csrc", "mapfx.hip")) as f:
        depth, flagged = [], False
        for line in f:
            t = line.strip()
            if t.startswith(("#ifdef", "#ifndef", "#if ")):
                depth.append("MAPFX_SPLIT_PROBE" in t)
            elif t.startswith("#endif"):
                depth.pop()
            elif ("split_probe" in t or "g_probe" in t) and not t.startswith("//"):
                assert any(depth), line
                flagged = True
        assert flagged and not depth


def test_model_is_clean_for_every_length():
    for T in ALL_T:
        for staged in _both(T):
            assert _check(T, staged) == [], (T, staged)
            # an autoreset re-count at every step changes nothing about that
            assert _check(T, staged, recounts=range(1, T)) == [], (T, staged)


def test_model_fits_the_probe_buffers():
    for T in ALL_T:
        for staged in _both(T):
            recs = sp.model(T, staged, recounts=range(1, T))
            for wave in range(3):
                assert sum(r.wave == wave for r in recs) <= sp.PROBE_CAP, (T, staged, wave)


def test_model_shape():
    """Spot values of the table: who touches what in which interval at T = 20."""
    recs = sp.model(20, True)
    def at(**kw):
        return [r for r in recs if all(getattr(r, k) == v for k, v in kw.items())]
    assert [(r.wave, r.interval, r.slot, r.kind) for r in at(res="MAP", tag=7)] == \
        [(0, 7, 1, "RMW"), (2, 8, 1, "R")]
    assert [(r.wave, r.interval, r.slot) for r in at(res="EDGE", tag=7)] == [(0, 8, 1), (2, 9, 1)]
    assert [(r.wave, r.interval, r.slot) for r in at(res="EDGE", tag=19)] == [(0, 19, 2), (2, 20, 2)]
    assert [(r.wave, r.interval, r.kind) for r in at(res="CODE", tag=18)] == [(1, 20, "W"), (2, 21, "R")]
    assert [(r.wave, r.interval, r.kind) for r in at(res="CODE", tag=3)] == [(2, 5, "W"), (2, 17, "R")]
    assert {r.interval for r in at(kind="SHARE")} == {-1}
    assert [r.slot for r in at(site="STAGE_NEXT")] == list(range(1, 20)) + [19]
    assert sorted(r.slot for r in at(site="STAGE_COMMIT", wave=1, kind="W")) == [16, 17, 18, 19]


@pytest.mark.parametrize("staged", [False, True])
def test_mutation_last_fold_in_interval_T(staged):
    """The race this project shipped: the launch's last fold in the interval in which the
    other store wave still writes code T - 2.  Flagged whenever the last batch holds that
    code -- T >= 2 and (T - 1) % 16 != 0 -- as a CODE conflict on row (T - 2) & 31 between the
    two store waves; clean otherwise (T = 17, 33: the batch is the folding wave's own code)."""
    for T in ALL_T:
        if staged and T > sp.STAGE_MAX_T:
            continue
        f = _check(T, staged, mutate="early_last_fold")
        if T >= 2 and (T - 1) % 16 != 0:
            conflicts = [x for x in f if x.rule == "conflict"]
            assert [(x.res, x.slot, x.interval, x.waves) for x in conflicts] == \
                [("CODE", (T - 2) & 31, T, (1, 2))], (T, f)
            # (the same read is also not fresh: its write is not ordered before it)
            assert all((x.res, x.slot) == ("CODE", (T - 2) & 31) for x in f), (T, f)
        else:
            assert f == [], (T, f)
    assert _check(17, staged, mutate="early_last_fold") == []
    assert _check(33, staged, mutate="early_last_fold") == []


@pytest.mark.parametrize("staged", [False, True])
def test_mutation_no_third_edge_slot(staged):
    """The last step's edge count in slot (T - 1) & 1: the step wave writes it while
    b(T - 3) reads that slot."""
    for T in ALL_T:
        if staged and T > sp.STAGE_MAX_T:
            continue
        f = _check(T, staged, mutate="no_third_edge_slot")
        hit = [x for x in f if x.rule == "conflict" and x.res == "EDGE" and x.slot == (T - 1) & 1 and
               x.interval == T - 1 and x.waves == (0, 1 + ((T - 3) & 1))]
        assert (len(hit) == 1) == (T >= 3), (T, f)
        assert all(x.res == "EDGE" for x in f), (T, f)
        if T < 3:
            assert f == [], (T, f)


@pytest.mark.parametrize("mutate,res,first_T", [("single_info_slot", "INFO", 2), ("map_early", "MAP", 3)])
def test_mutation_names_its_resource(mutate, res, first_T):
    for T in ALL_T:
        f = _check(T, False, mutate=mutate)
        assert all(x.res == res for x in f), (T, f)
        assert any(x.rule == "conflict" for x in f) == (T >= first_T), (T, f)


def test_mutation_code_ring_of_16_rows():
    """16 rows are one too few only where b(T - 1) writes row (T - 1) & 15 while b(T - 2)
    folds rows T - 17 .. T - 2 next to it: T % 16 == 1."""
    for T in ALL_T:
        f = _check(T, False, mutate="code_ring_16")
        assert all(x.res == "CODE" for x in f), (T, f)
        assert any(x.rule == "conflict" and x.slot == (T - 1) & 15 and x.interval == T for x in f) == \
            (T >= 17 and T % 16 == 1), (T, f)


def test_barrier_count_rule():
    recs = sp.model(5, True)
    f = sp.check(recs, (7, 6, 7), 5)
    assert [(x.rule, x.waves) for x in f] == [("barriers", (1,))]


def test_freshness_rule():
    R = sp.Rec
    w = R(0, 0, 0, "INFO_W", "INFO", 0, 0, "W")
    w2 = R(0, 1, 2, "INFO_W", "INFO", 0, 2, "W")
    r = R(1, 0, 3, "INFO_R", "INFO", 0, 0, "R")
    assert [x.rule for x in sp.check([w, w2, r])] == ["stale"]
    assert [x.rule for x in sp.check([w2, r])] == ["no write"]
    assert sp.check([w, r]) == []
    # a write of the same wave earlier in the interval is ordered before the read
    own = R(1, 0, 3, "IMG_W", "IMG", 0, 4, "W")
    assert sp.check([own, R(1, 1, 3, "IMG_R", "IMG", 0, 4, "R")]) == []
    assert [x.rule for x in sp.check([R(1, 0, 3, "IMG_R", "IMG", 0, 4, "R"), own._replace(seq=1)])] == ["no write"]


def test_compare_and_decode():
    exp = sp.model(3, True)
    assert sp.compare(exp, exp) == []
    assert sp.compare(exp[:-1], exp) != []
    moved = [r._replace(interval=r.interval + 1) if r.site == "EDGE_LAST" else r for r in exp]
    assert len(sp.compare(moved, exp)) == 2
    # round trip through the probe's packed words
    sites, ress, kinds = (list(x) for x in (sp.SITES, sp.RESOURCES, sp.KINDS))
    n = [0, 0, 0]
    rec = [[[0, 0] for _ in range(sp.PROBE_CAP)] for _ in range(3)]
    for r in exp:
        rec[r.wave][n[r.wave]] = [r.seq | (r.interval + 1) << 16,
                                  sites.index(r.site) | ress.index(r.res) << 8 | kinds.index(r.kind) << 12 |
                                  r.slot << 16 | (r.tag + 1) << 24]
        n[r.wave] += 1
    assert sorted(sp.decode(n, rec)) == sorted(exp)
