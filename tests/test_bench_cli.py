"""bench.py's command line: a plain run times the steps only, --full adds the other
measurements, --dump-outputs writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("kernel_ms_per_launch", "roofline", "per_step", "cpu_baseline")


def _bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + list(argv),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dump_outputs_budget_and_dtypes(tmp_path, monkeypatch):
    """Arrays over the budget are cut to the same seeded sample in every run; 8-byte
    elements leave as float64, everything else as float32."""
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 5 << 20)
    rs = np.random.RandomState(0)
    arrays = {"big": rs.randint(0, 100, size=(1 << 21,)).astype(np.int16),
              "r": rs.standard_normal(1000), "m": np.arange(35, dtype=np.uint8).reshape(5, 7)}
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, arrays)
    bench.dump_outputs(b, arrays)
    got = {k: np.load(os.path.join(a, k + ".npy")) for k in arrays}
    assert got["r"].dtype == np.float64 and np.array_equal(got["r"], arrays["r"])
    assert got["m"].dtype == np.float32 and np.array_equal(got["m"], arrays["m"])
    assert got["big"].dtype == np.float32 and got["big"].size < arrays["big"].size
    assert sum(x.nbytes for x in got.values()) <= 5 << 20
    assert np.isin(got["big"], arrays["big"]).all()
    for k in arrays:
        assert np.array_equal(got[k], np.load(os.path.join(b, k + ".npy")))


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last(tmp_path):
    """--steps K is the number of timed steps; the plain line carries ms_per_step and none
    of the --full measurements; the dump is the last of the warmup + K steps."""
    d = str(tmp_path / "out")
    line = _bench("--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", d)
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert abs(line["ms_per_step"] * 3 - line["timing"]["wall_ms"]) < 1e-3
    assert line["timing"]["launches"] == 1
    assert not [k for k in FULL_ONLY if k in line]
    E, N = 4096, 16
    shapes = {"reward": (E,), "term": (E,), "node": (E, N), "edge": (E, N), "avail": (E, N),
              "obs_window": (E, N, 2, 5, 5), "traj_pos": (E, N, 2), "traj_done": (E, N),
              "traj_t": (E,)}
    assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in shapes)
    total = 0
    for k, shape in shapes.items():
        x = np.load(os.path.join(d, k + ".npy"))
        assert x.shape == shape and x.dtype == (np.float64 if k == "reward" else np.float32)
        assert np.isfinite(x).all()
        total += x.nbytes
    assert total <= 64 << 20
    # warmup runs whole launches of the timed shape (3 steps), then the 3 timed steps
    assert (np.load(os.path.join(d, "traj_t.npy")) == 6).all()
    assert (np.load(os.path.join(d, "reward.npy")) < 0).any()


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements():
    line = _bench("--gpus", "1", "--steps", "3", "--warmup", "2", "--full",
                  "--per-step-steps", "4", "--cpu-seconds", "0.05")
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert not [k for k in FULL_ONLY if k not in line]
    assert line["kernel_ms_per_launch"] > 0 and line["roofline"]["achieved"] > 0
    assert line["per_step"]["kernel_ms"] > 0 and line["cpu_baseline"]["value"] > 0
