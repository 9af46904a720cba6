"""CPU: the kernel-point optimiser (weasal_amd.kernel_points.kernel_point_optimization / make_disposition) against the
seeded runs of the reference's optimiser recorded in g20_kernel_opt.npz, and the 9- and 13-point tables packaged from it."""
import hashlib
import os

import numpy as np
import pytest

from conftest import golden
from weasal_amd import kernel_points as kpm


def rng_digest():
    st = np.random.get_state()
    h = hashlib.sha256(np.ascontiguousarray(st[1]).tobytes())
    h.update(np.int64(st[2]).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


@pytest.fixture(scope="module")
def g20():
    return golden("g20_kernel_opt.npz")


@pytest.mark.parametrize("run", ["k9c", "k13c", "k9n"])
def test_optimiser_reproduces_the_recorded_runs(g20, run):
    """Same float64 numpy operations in the same order as the recorded routine: bit equality of the points, of the
    whole gradient-norm trace, of the step count, and of np.random's state after the call."""
    g = g20
    k, nk, fixed = int(g[run + "_num_points"]), int(g[run + "_num_kernels"]), str(g[run + "_fixed"])
    np.random.seed(int(g[run + "_seed"]))
    pts, norms = kpm.kernel_point_optimization(1.0, k, num_kernels=nk, dimension=3, fixed=fixed)
    sha = rng_digest()
    assert pts.dtype == np.float64 and pts.shape == (nk, k, 3) and norms.dtype == np.float64
    assert norms.shape == (int(g[run + "_steps"]), nk)
    assert np.array_equal(norms, g[run + "_norms"])
    assert np.array_equal(pts, g[run + "_points"])
    assert np.array_equal(sha, g[run + "_rng_sha"])


def test_radius_scales_the_result(g20):
    np.random.seed(int(g20["k13c_seed"]))
    pts, _ = kpm.kernel_point_optimization(2.5, 13, num_kernels=2)
    assert np.array_equal(pts, g20["k13c_points"] * 2.5)


@pytest.mark.parametrize("k", [9, 13])
def test_packaged_tables_are_the_generator_output(k):
    path = os.path.join(os.path.dirname(kpm.__file__), "data", "k_%03d_center_3D.txt" % k)
    table = np.loadtxt(path, dtype=np.float64)          # text with 17 significant digits: every float64 exactly
    assert table.dtype == np.float64 and table.shape == (k, 3)
    before = rng_digest().copy()
    assert np.array_equal(kpm.make_disposition(k), table)          # the module's seed
    assert np.array_equal(kpm.make_disposition(k, "center", kpm.DISPOSITION_SEED), table)
    assert np.array_equal(rng_digest(), before)                    # the caller's random stream is left alone
    assert np.array_equal(kpm._disposition(k, 3, "center"), table)


@pytest.mark.parametrize("k", [9, 13])
def test_packaged_tables_shape(k):
    """First point at the origin; the other K - 1 on a shell of mean radius 0.66.  The optimiser normalises the mean
    radius over all 100 candidates, and a candidate stops once its gradient norms change by < 1e-5 per step, not at
    a zero gradient: with the well's curvature of 10 a residual gradient of 1e-2 is a radial offset of 1e-3, the
    tolerance here.  The points of one table lie on one shell to the same tolerance."""
    table = kpm._disposition(k, 3, "center")
    assert np.array_equal(table[0], np.zeros(3))
    r = np.linalg.norm(table[1:], axis=1)
    assert abs(r.mean() - 0.66) < 1e-3
    assert np.abs(r - r.mean()).max() < 1e-3
    # distinct points: the repulsion keeps every pair apart by more than a third of the shell radius
    d = np.linalg.norm(table[:, None] - table[None], axis=-1) + 9.0 * np.eye(k)
    assert d.min() > 0.22


def test_thirteen_points_are_an_icosahedron():
    """12 shell points: each has 5 nearest neighbours at the icosahedron's edge, 1.0515 r."""
    table = kpm._disposition(13, 3, "center")[1:]
    d = np.linalg.norm(table[:, None] - table[None], axis=-1) + 9.0 * np.eye(12)
    edge = 0.66 / np.sin(2 * np.pi / 5)
    assert np.all((np.abs(d - edge) < 2e-3).sum(axis=1) == 5)


@pytest.mark.parametrize("k", [9, 13])
def test_load_kernels_random_stream(k):
    """load_kernels draws one rand() for the angle, then normal(size=(K, 3)); nothing else."""
    np.random.seed(77)
    got = kpm.load_kernels(0.5, k, 3, "center")
    after = rng_digest().copy()
    np.random.seed(77)
    theta = np.random.rand() * 2 * np.pi
    noise = np.random.normal(scale=0.01, size=(k, 3))
    assert np.array_equal(rng_digest(), after)
    c, s = np.cos(theta), np.sin(theta)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float32)
    want = np.matmul(0.5 * (kpm._disposition(k, 3, "center") + noise), R).astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_unbuilt_requests_still_raise():
    with pytest.raises(NotImplementedError):
        kpm.kernel_point_optimization(1.0, 9, fixed="verticals")
    with pytest.raises(NotImplementedError):
        kpm.kernel_point_optimization(1.0, 9, dimension=2)
    with pytest.raises(NotImplementedError):
        kpm.kernel_point_optimization(1.0, 31)
    with pytest.raises(NotImplementedError):
        kpm.make_disposition(31)
    for args in [(1.0, 9, 3, "verticals"), (1.0, 31, 3, "center"), (1.0, 20, 3, "center"), (1.0, 9, 3, "none")]:
        with pytest.raises(NotImplementedError):
            kpm.load_kernels(*args)
