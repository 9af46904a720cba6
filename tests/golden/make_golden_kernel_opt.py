"""Generates tests/golden/g20_kernel_opt.npz (run once in the build container, on the CPU; the reference cannot travel): the
reference's OWN kernels/kernel_points.py:kernel_point_optimization_debug (:257-404, verbose = 0: no figure is opened)
under np.random.seed, for the runs of RUNS below.  Only settings and recorded results are stored, per run r:
  r_seed, r_num_points, r_num_kernels, r_fixed      the call (radius 1.0, dimension 3, ratio 0.66: the defaults load_kernels uses)
  r_points [num_kernels, num_points, 3]             float64
  r_norms  [steps, num_kernels]                     the full gradient-norm trace
  r_steps                                           its length
  r_rng_sha                                         sha256 of np.random's state (key, pos) after the call
Asserted here, at generation time: a second run under the same seed gives the same bits, and weasal_amd.kernel_points.
kernel_point_optimization reproduces the record bit for bit.
Usage: python tests/golden/make_golden_kernel_opt.py"""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402,F401  (import aids; puts the reference on sys.path)
import numpy as np                # noqa: E402
import matplotlib                 # noqa: E402
matplotlib.use("Agg")
from kernels import kernel_points as ref   # noqa: E402
from weasal_amd import kernel_points as kpm  # noqa: E402

# (name, seed, num_points, num_kernels, fixed)
RUNS = [("k9c", 901, 9, 3, "center"), ("k13c", 1301, 13, 2, "center"), ("k9n", 902, 9, 2, "none")]


def rng_digest():
    st = np.random.get_state()
    h = hashlib.sha256(np.ascontiguousarray(st[1]).tobytes())
    h.update(np.int64(st[2]).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def main():
    out = {"runs": np.array([r[0] for r in RUNS])}
    for name, seed, k, nk, fixed in RUNS:
        np.random.seed(seed)
        pts, norms = ref.kernel_point_optimization_debug(1.0, k, num_kernels=nk, dimension=3, fixed=fixed, verbose=0)
        sha = rng_digest()
        np.random.seed(seed)
        pts2, norms2 = ref.kernel_point_optimization_debug(1.0, k, num_kernels=nk, dimension=3, fixed=fixed, verbose=0)
        assert np.array_equal(pts, pts2) and np.array_equal(norms, norms2) and np.array_equal(sha, rng_digest())
        np.random.seed(seed)
        own, own_norms = kpm.kernel_point_optimization(1.0, k, num_kernels=nk, dimension=3, fixed=fixed)
        assert np.array_equal(own, pts) and np.array_equal(own_norms, norms) and np.array_equal(sha, rng_digest())
        assert pts.dtype == np.float64 and pts.shape == (nk, k, 3) and norms.shape[0] < 10000
        out[name + "_seed"], out[name + "_num_points"], out[name + "_num_kernels"] = np.int64(seed), np.int64(k), np.int64(nk)
        out[name + "_fixed"] = np.array(fixed)
        out[name + "_points"], out[name + "_norms"] = pts, norms
        out[name + "_steps"], out[name + "_rng_sha"] = np.int64(norms.shape[0]), sha
        print(name, "steps", norms.shape[0], "last norms", norms[-1])
    path = os.path.join(HERE, "g20_kernel_opt.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
