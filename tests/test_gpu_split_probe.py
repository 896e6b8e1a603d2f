"""The split rollout's three-wave LDS protocol, checked on the device without relying on
timing luck (the resource / interval table).

libmapfx_probe.so is mapfx.hip compiled with -DMAPFX_SPLIT_PROBE: in one traced workgroup
every wave logs which shared LDS resource it touches in which barrier interval and which
step's data it expects.  tests/split_protocol.py holds the documented schedule as a model
and a checker for conflicts and stale reads.

1. the kernel's log equals the model and the checker finds nothing in it, for every launch
   length at which the schedule takes another path, while the same launch's outputs equal
   the oracle;
2. negative control: with the launch's last fold put back into interval T (the race this
   project once shipped) the checker reports the CODE conflict at T = 20, on every run, and
   nothing at T = 17, where that batch holds only the folding wave's own code;
3. a supplement: with one wave delayed at one annotated site -- by about one and about four
   step-wave barrier intervals (~2,000 and ~8,000 cycles; perturbation sizes, nothing is
   asserted about time) -- every launch still equals the oracle.

The probe library is chosen when mapfx is imported, so every launch runs in a fresh child
process (tests/split_probe_child.py), one at a time.  A child that ends by signal or
timeout fails its test and every probe case after it is skipped: nothing more is started
on a device that may have faulted.

Shapes as in tests/test_gpu_rollout_action_staging.py: 12x12 maps, 20 % obstacles, runner
output set, int8 actions in a 16-byte-aligned buffer."""
import json
import os
import subprocess
import sys

import pytest
import torch

import split_protocol as sp
from test_gpu_rollout_action_staging import STAGE_MAX_T, _split_lds

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_LIB = os.path.join(REPO, "mapf-marl_amd", "mapfx", "libmapfx_probe.so")
CHILD = os.path.join(REPO, "tests", "split_probe_child.py")
S = 12

TRACE_T = [1, 2, 3, 15, 16, 17, 20, 31, 32, 33, 48, 64, 65, 96]  # <= 64: staged, past it register blocks
DELAY_T = [1, 2, 3, 15, 16, 17, 20, 32, 33, 64, 65]

_STOP = {"why": None}  # set when a child died: the remaining probe cases are skipped


def _kernel(N, win, occ, T):
    return "mapf_wave_kernel<%d, true, true, true, %d, true, %s, %d>" % (
        win, N, "true" if occ else "false", 8 if T <= 32 else 0)


def _path(N, win, occ, T):
    """2 staged, 1 register blocks: launch()'s rule (T <= 64 and the extra 16 + 64 T bytes of
    LDS leave the resident workgroups per CU as they are)."""
    lds = _split_lds(S, N, win) - (2 * 64 * win * win if occ else 0)
    staged = lds + 16 + 64 * T
    ok = T <= STAGE_MAX_T and staged <= 64 * 1024 and min(4, 160 * 1024 // staged) == min(4, 160 * 1024 // lds)
    return 2 if ok else 1


def _run_child(job, tmp_path, timeout):
    if _STOP["why"]:
        pytest.skip("an earlier probe child %s: no further probe launches" % _STOP["why"])
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    assert os.path.exists(PROBE_LIB), "%s not built: build() makes it next to libmapfx.so" % PROBE_LIB
    job_path, out_path = str(tmp_path / "job.json"), str(tmp_path / "result.json")
    with open(job_path, "w") as f:
        json.dump(job, f)
    env = dict(os.environ, MAPFX_LIB=PROBE_LIB)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [CHILD, job_path, out_path]
    try:
        p = subprocess.run(cmd, env=env, timeout=timeout, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:
        _STOP["why"] = "ran into its %d s timeout" % timeout
        pytest.fail("probe child timed out after %d s\n%s" % (timeout, e.stdout))
    if p.returncode < 0:
        _STOP["why"] = "ended by signal %d" % -p.returncode
    assert p.returncode == 0, "probe child exit %d\n%s" % (p.returncode, p.stdout[-4000:])
    with open(out_path) as f:
        res = json.load(f)
    assert res.get("done")
    return res


# name -> N, E, window, occupancy records, autoreset, traced workgroup
TRACE_CASES = {
    "n16-e4": dict(N=16, E=4, win=5, block=0),
    "n16-e4-autoreset": dict(N=16, E=4, win=5, block=0, autoreset=True, limit=6),
    "n16-e36": dict(N=16, E=36, win=5, block=0),
    "n16-e36-last-block": dict(N=16, E=36, win=5, block=8),
    "n16-e36-last-block-autoreset": dict(N=16, E=36, win=5, block=8, autoreset=True, limit=6),
    "n16-e36-occ": dict(N=16, E=36, win=5, block=0, occ=True),
    "n64-e3-w3": dict(N=64, E=3, win=3, block=0),
}


def _records(r):
    return [sp.Rec(*x) for x in r["records"]]


@pytest.mark.parametrize("name", sorted(TRACE_CASES))
def test_trace_equals_model(name, tmp_path):
    c = dict(TRACE_CASES[name], name=name, Ts=TRACE_T)
    res = _run_child({"mode": "trace", "cases": [c]}, tmp_path, timeout=120 + 2 * len(TRACE_T))
    resets = 0
    for T in TRACE_T:
        r = res["cases"]["%s/T%d" % (name, T)]
        assert r["error"] is None, (T, r["error"])  # (the launch's outputs against the oracle)
        occ = c.get("occ", False)
        assert _kernel(c["N"], c["win"], occ, T) in r["kernel"], (T, r["kernel"])
        path = _path(c["N"], c["win"], occ, T)
        assert r["path"] == path and path == (2 if T <= STAGE_MAX_T else 1), (T, r["path"])
        assert r["overflow"] == 0 and max(r["n"]) <= sp.PROBE_CAP, (T, r["n"])
        recs = _records(r)
        assert sp.check(recs, r["barriers"], T) == [], T
        assert sp.compare(recs, sp.model(T, path == 2, recounts=r["recounts"])) == [], T
        resets += len(r["recounts"])
    if c.get("autoreset"):
        assert resets >= 20  # re-counts did happen inside the launches


def test_negative_control_early_last_fold(tmp_path):
    """The last fold in interval T: flagged from the trace alone at T = 20, clean at T = 17.
    Whether the rewards came out wrong is a matter of timing and is not asserted."""
    c = dict(N=16, E=4, win=5, block=0, early=True, name="early", Ts=[20, 17])
    res = _run_child({"mode": "trace", "cases": [c]}, tmp_path, timeout=120)
    for T in (20, 17):
        r = res["cases"]["early/T%d" % T]
        assert r["error"] is None, (T, r["error"])
        assert _kernel(16, 5, False, T) in r["kernel"] and r["path"] == 2, (T, r["kernel"], r["path"])
        assert r["overflow"] == 0
        recs = _records(r)
        assert sp.compare(recs, sp.model(T, True, mutate="early_last_fold")) == [], T
        f = sp.check(recs, r["barriers"], T)
        conflicts = [(x.res, x.slot, x.interval, x.waves) for x in f if x.rule == "conflict"]
        if T == 20:
            assert conflicts == [("CODE", (T - 2) & 31, T, (1, 2))], f
        else:
            assert f == [], f


@pytest.mark.parametrize("T", DELAY_T)
def test_delayed_parity(T, tmp_path):
    shapes = [dict(N=16, E=4, win=5), dict(N=16, E=36, win=5)]
    if T == 20:
        shapes.append(dict(N=64, E=3, win=3))
    per_shape = 2 * (len(sp.STEP_SITES) + 2 * len(sp.STORE_SITES))  # two delay lengths
    res = _run_child({"mode": "delay", "T": T, "shapes": shapes}, tmp_path,
                     timeout=120 + len(shapes) * per_shape // 4)
    assert res["error"] is None, res["error"]
    assert res["launches"] == len(shapes) * per_shape
    assert res["mismatches"] == []
    for N, E, kern, path in res["kernels"]:
        win = 3 if N == 64 else 5
        assert _kernel(N, win, False, T) in kern and path == _path(N, win, False, T), (N, E, kern, path)
