"""bench.py end to end on the GPU, every workload and mode for two steps: the contract line (one JSON object on stdout with
the driver's keys, `roofline` under --full, the workload named in `config`), so that a change that breaks a secondary workload
shows up in the suite and not at the next capture; a plain run's line and its --dump-outputs files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
        "dtype", "data", "config", "roofline")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "2", "--warmup", "1", *args],
                       capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]          # ONE line on stdout
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("args,dtype,points", [((), "f32", 400000),
                                               (("--mode", "infer"), "f32", 400000),
                                               (("--workload", "vaihingen"), "f32", 12000),
                                               (("--workload", "vaihingen_wl"), "f32", 6000),
                                               (("--workload", "dales_deform"), "bf16", 400000),
                                               (("--prefetch", "0", "--contrast", "0"), "f32", 400000),
                                               (("--nearest-upsample", "1"), "f32", 400000)])
def test_bench_line_of_every_workload(args, dtype, points):
    d = _bench("--full", "--no-cpu-baseline", *args)
    for k in KEYS:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "points/s" and d["data"] == "synthetic"
    assert d["dtype"] == dtype and d["config"]["points_per_step_per_gpu"] == points
    assert d["value"] > 0 and abs(d["value"] - points / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and 0 < rf["frac"] < 1.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert d["config"]["library_launches_per_step"] > 50
    assert "cpu_baseline" not in d                   # (--no-cpu-baseline)
    assert ("OPT-IN nearest-only" in d["config"]["workload"]) == ("--nearest-upsample" in args)


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("args,names", [((), {"loss", "logits", "parameters"}),
                                        (("--mode", "infer"), {"logits"}),
                                        (("--workload", "vaihingen_wl"), {"loss", "logits", "class_logits", "cam", "parameters"})])
def test_plain_run_times_the_headline_and_dumps_the_last_step(tmp_path, args, names):
    """without --full the line holds the headline only (no HIP-event figures, no CPU baseline); --dump-outputs writes the
    last timed step's arrays as float32, 64 MB at most"""
    d = _bench("--dump-outputs", str(tmp_path), *args)
    for k in KEYS[:-1]:
        assert k in d, k
    assert "roofline" not in d and "kernels_ms" not in d and "cpu_baseline" not in d
    assert d["steps"] == 2 and abs(d["value"] - d["config"]["points_per_step_per_gpu"] / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(n + ".npy" for n in names)
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in files) <= 64 * 1000 * 1000
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in files}
    for a in got.values():
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all()
    assert got["logits"].shape[0] == d["config"]["points_per_step_per_gpu"]
    if "loss" in got:
        assert got["loss"].item() == np.float32(d["config"]["final_loss"])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_dumped_outputs_repeat_from_run_to_run(tmp_path):
    """the same arguments give the same inputs: two runs' outputs agree up to the order of floating-point sums"""
    runs = [tmp_path / "a", tmp_path / "b"]
    for r in runs:
        _bench("--workload", "vaihingen", "--dump-outputs", str(r))
    for name in ("loss", "logits", "parameters"):
        a, b = (np.load(r / (name + ".npy")) for r in runs)
        assert a.shape == b.shape, name
        assert np.abs(a - b).max() <= 1e-4 * max(np.abs(a).max(), 1e-6), name
