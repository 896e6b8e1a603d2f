"""Child process of tests/test_gpu_split_probe.py: runs split-rollout launches on the probe
build of the library (MAPFX_LIB = libmapfx_probe.so, chosen before mapfx is imported) and
writes what it saw to a JSON file; the parent asserts on that file.

    python split_probe_child.py JOB.json RESULT.json

JOB: {"mode": "trace", "cases": [{"name", "N", "E", "win", "occ", "autoreset", "limit",
      "block", "early", "Ts"}]} or {"mode": "delay", "T": .., "shapes": [{"N", "E", "win"}]}.
The result is rewritten after every case, so a child that dies leaves what it finished."""
import ctypes
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (HERE, REPO, os.path.join(REPO, "mapf-marl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import split_protocol as sp  # noqa: E402
import test_gpu_rollout_action_staging as st  # noqa: E402  (shapes, actions, _check_vs_oracle)
import mapfx  # noqa: E402
from mapfx import _abi  # noqa: E402

S = st.S
AR_LIMIT = 6          # autoreset cases: every env resets several times inside a launch
DELAY_LENS = (1, 4)   # sleeps of ~2000 cycles: about one step-wave barrier interval, about four


class ProbeCfg(ctypes.Structure):  # csrc/internal.h mapfx_split_probe_cfg
    _fields_ = [(k, ctypes.c_int32) for k in ("block", "delay_role", "delay_site", "delay_len",
                                              "early_last_fold")]


class ProbeTrace(ctypes.Structure):  # csrc/internal.h mapfx_split_probe_trace
    _fields_ = [("n", ctypes.c_uint32 * 3), ("barriers", ctypes.c_uint32 * 3),
                ("overflow", ctypes.c_uint32), ("pad", ctypes.c_uint32),
                ("rec", ctypes.c_uint32 * 2 * sp.PROBE_CAP * 3)]


def configure(block=-1, role=-1, site=-1, length=0, early=0):
    cfg = ProbeCfg(block, role, site, length, early)
    _abi.check(_abi.lib.mapfx_split_probe_config(ctypes.byref(cfg)), "mapfx_split_probe_config")


def read_trace():
    tr = ProbeTrace()
    _abi.check(_abi.lib.mapfx_split_probe_read(ctypes.byref(tr)), "mapfx_split_probe_read")
    return tr


def outs(occ):
    return tuple("obs_window_occ" if (occ and k == "obs_window") else k for k in st.OUTS)


def launch(c, T, inst, acts):
    """A fresh batch and one rollout of T steps; (batch, traj, kernel name, action path)."""
    limit = c.get("limit", 2000)
    b = st._batch(mapfx, inst, win=c["win"], limit=limit, occ=c.get("occ", False))
    traj = b.rollout(T, actions=acts, autoreset=c.get("autoreset", False), outputs=outs(c.get("occ", False)))
    return b, traj, _abi.last_kernel(), _abi.last_action_path()


def run_trace(job, save):
    res = {"cases": {}}
    for c in job["cases"]:
        inst = st._inst(c["E"], n=c["N"], seed=41 if c["N"] == 16 else 43)
        assert (c["E"] * c["N"] // 64) % 8 != 0  # the workgroups keep their order: block b, envs 64 / N * b ..
        for T in c["Ts"]:
            r = {"error": None}
            res["cases"]["%s/T%d" % (c["name"], T)] = r
            try:
                acts_np = st._actions(T, c["E"], n=c["N"], seed=21)
                acts = torch.from_numpy(acts_np).cuda()
                assert acts.data_ptr() % 16 == 0
                configure(block=c["block"], early=1 if c.get("early") else 0)
                b, traj, r["kernel"], r["path"] = launch(c, T, inst, acts)
                tr = read_trace()
                configure()
                r["n"], r["barriers"], r["overflow"] = list(tr.n), list(tr.barriers), int(tr.overflow)
                r["records"] = [list(x) for x in sp.decode(tr.n, tr.rec)]
                if not c.get("early"):  # (the early fold may or may not read a stale code: not asserted)
                    st._check_vs_oracle(b, traj, acts_np, inst, win=c["win"], limit=c.get("limit", 2000),
                                        autoreset=c.get("autoreset", False), occ=c.get("occ", False))
                    b.check_err()
                # the steps that start with a re-count: an env of the traced workgroup ended the step before
                epw = 64 // c["N"]
                term = st._np(traj["term"])[:, c["block"] * epw:(c["block"] + 1) * epw]
                r["recounts"] = [k + 1 for k in range(T - 1) if c.get("autoreset") and term[k].any()]
            except Exception:
                r["error"] = traceback.format_exc()
            save(res)
    return res


def snapshot(b, traj):
    torch.cuda.synchronize()
    d = {k: st._np(v).copy() for k, v in traj.items() if isinstance(v, torch.Tensor)}
    for k in ("pos", "done", "t"):
        d["final_" + k] = st._np(getattr(b, k)).copy()
    return d


def run_delay(job, save):
    """Every (role, site, length) delay at T steps on every shape against the oracle: the
    undelayed launch is checked against the oracle step by step (once per shape and
    autoreset setting), and every delayed launch must equal it bit for bit."""
    T = job["T"]
    res = {"launches": 0, "mismatches": [], "kernels": [], "error": None}
    try:
        for c in job["shapes"]:
            inst = st._inst(c["E"], n=c["N"], seed=41 if c["N"] == 16 else 43)
            acts_np = st._actions(T, c["E"], n=c["N"], seed=22)
            acts = torch.from_numpy(acts_np).cuda()
            assert acts.data_ptr() % 16 == 0
            refs = {}
            for ar in (False, True):
                cc = dict(c, autoreset=ar, limit=AR_LIMIT if ar else 2000)
                configure()
                b, traj, kern, path = launch(cc, T, inst, acts)
                st._check_vs_oracle(b, traj, acts_np, inst, win=c["win"], limit=cc["limit"], autoreset=ar)
                b.check_err()
                refs[ar] = (cc, snapshot(b, traj))
                res["kernels"].append([c["N"], c["E"], kern, path])
            for role in (0, 1, 2):
                for site in (sp.STEP_SITES if role == 0 else sp.STORE_SITES):
                    cc, ref = refs[site == "MAP_RESET"]  # (the re-count runs only with autoreset)
                    for length in DELAY_LENS:
                        configure(role=role, site=sp.SITES.index(site), length=length)
                        b, traj, kern, path = launch(cc, T, inst, acts)
                        got = snapshot(b, traj)
                        res["launches"] += 1
                        res["kernels"].append([c["N"], c["E"], kern, path])
                        for k in ref:
                            x, y = got[k], ref[k]
                            if x.dtype == np.float64:
                                x, y = st._u64(x), st._u64(y)
                            if not np.array_equal(x, y):
                                res["mismatches"].append([c["N"], c["E"], role, site, length, k])
            configure()
            save(res)
    except Exception:
        res["error"] = traceback.format_exc()
    return res


def main():
    job_path, out_path = sys.argv[1:3]
    with open(job_path) as f:
        job = json.load(f)
    assert os.path.basename(_abi.LIB_PATH) == "libmapfx_probe.so", _abi.LIB_PATH

    def save(res):
        with open(out_path + ".tmp", "w") as f:
            json.dump(res, f)
        os.replace(out_path + ".tmp", out_path)

    res = run_trace(job, save) if job["mode"] == "trace" else run_delay(job, save)
    res["done"] = True
    save(res)


if __name__ == "__main__":
    main()
