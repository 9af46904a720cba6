"""bench.py without a GPU: its own launcher's argument / environment handling of `--gpus N` without torchrun, and the
size cap and fixed sample of --dump-outputs."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                            "WEASAL_DIST_BACKEND")}


def test_more_ranks_than_gpus_is_refused_for_rccl():
    """RCCL needs one GPU per rank: with fewer visible GPUs the launcher says so and starts nothing"""
    res = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "64", "--steps", "1", "--warmup", "0"],
                         env=_env(), capture_output=True, text=True, timeout=300)
    assert res.returncode == 2
    assert "one GPU per rank" in res.stderr


def test_child_failure_is_the_launchers_exit_code():
    """the ranks need a GPU; on a box without one every child fails and the launcher must not report success"""
    import torch
    if torch.cuda.is_available():
        return
    env = _env()
    env["WEASAL_DIST_BACKEND"] = "gloo"
    res = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                          "--no-cpu-baseline", "--workload", "vaihingen"], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode != 0
    assert "needs a GPU" in res.stderr


def test_gpus_flag_must_match_the_launchers_world_size():
    env = _env()
    env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    res = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                         env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "WORLD_SIZE=1" in res.stderr


def test_steps_must_be_positive():
    res = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0"], env=_env(), capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 2 and "--steps" in res.stderr


def test_dump_outputs_caps_the_bytes_with_a_fixed_sample(tmp_path):
    import numpy as np
    import torch
    import bench
    big = torch.arange(6_000_000, dtype=torch.float64)       # (integers exact in float32)
    arrays = {"loss": torch.tensor(1.5), "big": big, "small": torch.ones(3, 4, dtype=torch.bfloat16)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "loss.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 1000 * 1000
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype == np.float32 for a in got.values())
    assert float(got["loss"]) == 1.5 and got["small"].shape == (3, 4) and (got["small"] == 1).all()
    s = got["big"]
    assert s.size == bench.DUMP_BYTES // (4 * 3) and (np.diff(s) > 0).all() and s[-1] < 6_000_000    # ascending distinct elements
    assert np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))                                        # the same sample every time
