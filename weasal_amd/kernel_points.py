"""Kernel-point dispositions (host side of KPConv.init_KP).

Mirrors the interface of the reference's kernels/kernel_points.py for the part the hot path
uses: ``load_kernels`` (kernel_points.py:407-488) and ``create_3D_rotations`` (:43-74).  The
cached 15-point 'center' disposition the reference ships as kernels/dispositions/
k_015_center_3D.ply is packaged as a data table (weasal_amd/data/k_015_center_3D.npy, 15x3
float64).  The reference writes every other disposition on first use with its gradient optimiser
(:257-404, 100 candidates, :433-444); ``kernel_point_optimization`` / ``make_disposition`` restate
that arithmetic, and the 9- and 13-point 'center' tables packaged next to the 15-point one
(k_009_center_3D.txt, k_013_center_3D.txt: text, every value exact) are ``make_disposition`` under DISPOSITION_SEED.
``load_kernels`` never runs the optimiser: asking for a disposition that is not packaged raises.
The Lloyd generator (:77-254, K > 30), 'verticals' and 2-D kernels are not restated.
"""
import os

import numpy as np

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def create_3D_rotations(axis, angle):
    """Rotation matrices from unit axes [N,3] and angles [N] (Rodrigues form), float64 in ->
    [N,3,3].  Same element formulas as the reference (kernel_points.py:43-74) so that seeded
    rotations are bit-identical."""
    axis = np.asarray(axis)
    angle = np.asarray(angle)
    c = np.cos(angle)
    omc = 1 - c
    s = np.sin(angle)
    ax, ay, az = axis[:, 0], axis[:, 1], axis[:, 2]
    xy = omc * ax * ay
    xz = omc * ax * az
    yz = omc * ay * az
    rows = [c + omc * (ax * ax), xy - s * az, xz + s * ay,
            xy + s * az, c + omc * (ay * ay), yz - s * ax,
            xz - s * ay, yz + s * ax, c + omc * (az * az)]
    return np.reshape(np.stack(rows, axis=1), (-1, 3, 3))


# np.random.seed of the packaged k_009 / k_013 tables (make_disposition; data/k_0xx_center_3D.txt)
DISPOSITION_SEED = 20240915
_CANDIDATES = 100
_MAX_STEPS = 10000


def kernel_point_optimization(radius, num_points, num_kernels=1, dimension=3, fixed="center", ratio=0.66):
    """`num_kernels` dispositions of `num_points` points each by gradient descent on a repulsive
    potential between the points plus a quadratic well, all kernels in one array (the arithmetic
    contract of the reference's kernel_point_optimization_debug, kernel_points.py:257-404: the same
    float64 numpy operations in the same order, np.random consumed in the same order, so a seeded
    run has the reference's bits).  fixed: 'center' pins point 0 at the origin, 'none' pins nothing.
    Returns (points [num_kernels, num_points, dimension] * radius, gradient_norms [steps, num_kernels]:
    the largest gradient norm of each kernel at every step)."""
    if dimension != 3:
        raise NotImplementedError("only 3-D kernels are supported")
    if fixed not in ("center", "none"):
        raise NotImplementedError("fixed must be 'center' or 'none' (got %r)" % (fixed,))
    if num_points > 30:
        raise NotImplementedError("more than 30 kernel points take the reference's Lloyd generator, which is not restated")
    radius0, diameter0 = 1, 2
    moving_factor, decay = 1e-2, 0.9995
    thresh = 1e-5
    clip = 0.05 * radius0
    total = num_kernels * num_points

    # start: uniform in the cube, rejected down to the ball d2 < 0.5; draws of total - 1 rows, so at least two
    pts = np.random.rand(total - 1, dimension) * diameter0 - radius0
    while pts.shape[0] < total:
        new = np.random.rand(total - 1, dimension) * diameter0 - radius0
        pts = np.vstack((pts, new))
        d2 = np.sum(np.power(pts, 2), axis=1)
        pts = pts[d2 < 0.5 * radius0 * radius0, :]
    pts = pts[:total, :].reshape((num_kernels, num_points, -1))
    center = fixed == "center"
    if center:
        pts[:, 0, :] *= 0

    saved = np.zeros((_MAX_STEPS, num_kernels))
    old_norms = np.zeros((num_kernels, num_points))
    first = 1 if center else 0           # first point that moves
    step = -1
    while step < _MAX_STEPS:
        step += 1
        # gradient of the pair potential 1/d summed over the other points, plus the well 5 |x|^2
        a = np.expand_dims(pts, axis=2)
        b = np.expand_dims(pts, axis=1)
        interd2 = np.sum(np.power(a - b, 2), axis=-1)
        inter = (a - b) / (np.power(np.expand_dims(interd2, -1), 3 / 2) + 1e-6)
        inter = np.sum(inter, axis=1)
        grads = inter + 10 * pts
        norms = np.sqrt(np.sum(np.power(grads, 2), axis=-1))
        saved[step, :] = np.max(norms, axis=1)
        # stop once no moving point's gradient norm changed by 1e-5
        if np.max(np.abs(old_norms[:, first:] - norms[:, first:])) < thresh:
            break
        old_norms = norms
        # move along the gradient by at most `clip`
        dists = np.minimum(moving_factor * norms, clip)
        if center:
            dists[:, 0] = 0
        pts -= np.expand_dims(dists, -1) * grads / np.expand_dims(norms + 1e-6, -1)
        moving_factor *= decay
    if step < _MAX_STEPS:
        saved = saved[:step + 1, :]
    # mean radius of the points past the first -> ratio (also with fixed='none', as the reference does)
    r = np.sqrt(np.sum(np.power(pts, 2), axis=-1))
    pts *= ratio / np.mean(r[:, 1:])
    return pts * radius, saved


def make_disposition(num_kpoints, fixed="center", seed=DISPOSITION_SEED):
    """The unit-radius table load_kernels reads: of 100 candidates optimised together, the one whose
    last gradient norm is smallest (kernel_points.py:433-444).  Seeds and restores np.random."""
    state = np.random.get_state()
    try:
        np.random.seed(seed)
        points, norms = kernel_point_optimization(1.0, num_kpoints, num_kernels=_CANDIDATES, dimension=3, fixed=fixed)
    finally:
        np.random.set_state(state)
    return points[np.argmin(norms[-1, :]), :, :]


def _disposition(num_kpoints, dimension, fixed):
    name = "k_{:03d}_{:s}_{:d}D.npy".format(num_kpoints, fixed, dimension)
    path = os.path.join(_DATA, name)
    text = path[:-4] + ".txt"           # the tables of make_disposition: 17 significant digits per value, exact float64
    if not os.path.exists(path) and os.path.exists(text):
        return np.loadtxt(text, dtype=np.float64).reshape(num_kpoints, dimension)
    if not os.path.exists(path):
        raise NotImplementedError(
            "kernel disposition %s is not packaged (the reference would run its Lloyd / gradient "
            "optimiser, kernels/kernel_points.py:77-404, which is outside the hot path)" % name)
    return np.load(path)


def load_kernels(radius, num_kpoints, dimension, fixed, lloyd=False):
    """Kernel points for one KPConv: disposition + N(0, 0.01) noise, scaled by `radius`, rotated
    about z by a random angle.  Consumes np.random in the reference's order (one rand() for the
    angle, then normal(size=(K,dim))) so that a seeded run reproduces the reference's values."""
    kernel_points = _disposition(num_kpoints, dimension, fixed)
    if dimension != 3 or fixed == "vertical":
        raise NotImplementedError("only 3-D kernels with fixed in {'center','none'} are supported")
    theta = np.random.rand() * 2 * np.pi
    c, s = np.cos(theta), np.sin(theta)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float32)
    kernel_points = kernel_points + np.random.normal(scale=0.01, size=kernel_points.shape)
    kernel_points = radius * kernel_points
    kernel_points = np.matmul(kernel_points, R)
    return kernel_points.astype(np.float32)
