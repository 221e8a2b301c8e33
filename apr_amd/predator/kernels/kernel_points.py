"""Kernel-point dispositions (Predator_APR/kernels/kernel_points.py:246-470 `kernel_point_optimization_debug`,
`load_kernels`).

The reference reads the optimised disposition of (num_kpoints, fixed) from `kernels/dispositions/k_{K:03d}_{fixed}_3D.ply`
in the working directory -- it ships the 15-point 'center' file and MAKES every other one on first use by a descent on
repulsive potentials --, applies a RANDOM z-rotation and N(0, 0.01) noise from the global NumPy RNG, and scales by the
radius; the result is stored in the module as the non-trainable parameter `kernel_points` (so trained checkpoints carry
their own).

Here the 15x3 'center' table ships as data (`k_015_center_3D.npy`, extracted from that .ply) and `kernel_point_optimization`
restates the descent: the same NumPy draws in the same order, the same constants and the same global stop rule, so under the
same `np.random.seed` the points equal the reference's first run in a fresh working directory.

Where a made disposition lives, and what that means for seeded runs
-------------------------------------------------------------------
A made disposition is kept in a module-level memo keyed by (K, fixed); with `APR_KP_DISPOSITION_DIR` set it is also
written to that directory as `k_{K:03d}_{fixed}_3D.npy` and later processes read it from there (the stand-in for the
reference's .ply files; nothing is ever written into the package or the working directory).  The generator's draws are
consumed ONLY when a disposition is actually made: the first `load_kernels(.., K, .., fixed)` of a process without a
directory (or of the first process with one) advances the global RNG by the generator's draws plus the rotation and the
noise, every later call by the rotation and the noise alone -- the reference's first run without a file and its later runs
with one.  A seeded run that must reproduce another has to start from the same state: both with the disposition at hand
(memo or directory) or both without.  `(15, 'center')` never draws more than the rotation and the noise.
"""
import os

import numpy as np

_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "k_015_center_3D.npy")
_FIXED = ('none', 'center', 'verticals')
_MEMO = {}      # (K, fixed) -> float64 [K, 3] disposition at radius 1
DISPOSITION_DIR_ENV = "APR_KP_DISPOSITION_DIR"


def kernel_point_optimization(radius, num_points, num_kernels=1, dimension=3, fixed='center', ratio=0.66):
    """`num_kernels` dispositions of `num_points` kernel points by descent on the potential sum_ij 1 / |x_i - x_j| +
    5 sum_i |x_i|^2 (kernel_points.py:246-385) -> (points [num_kernels, num_points, dimension] scaled to `radius`,
    saved_gradient_norms [10000, num_kernels]: row i holds every kernel's largest gradient norm at iteration i; the rows
    after the stop stay 0).  fixed: 'center' pins point 0 at the origin, 'verticals' points 0, 1, 2 at the origin and at
    +-2/3 on the last axis (1 and 2 may still slide along it), 'none' nothing.  All kernels stop together: when the largest
    change of a gradient norm over ALL kernels (over the moving points for 'center' / 'verticals') falls under 1e-5."""
    n_iter, thresh, clip, decay = 10000, 1e-5, 0.05, 0.9995
    step = 1e-2
    total = num_kernels * num_points
    # rejection sampling of the ball of radius sqrt(0.5) in the cube [-1, 1]^d; the first batch is NOT filtered on its own
    pts = np.random.rand(total - 1, dimension) * 2 - 1
    while pts.shape[0] < total:
        pts = np.vstack((pts, np.random.rand(total - 1, dimension) * 2 - 1))
        pts = pts[np.sum(np.power(pts, 2), axis=1) < 0.5, :]
    pts = pts[:total, :].reshape((num_kernels, num_points, -1))
    if fixed == 'center':
        pts[:, 0, :] *= 0
    if fixed == 'verticals':
        pts[:, :3, :] *= 0
        pts[:, 1, -1] += 2 / 3
        pts[:, 2, -1] -= 2 / 3
    first_moving = {'center': 1, 'verticals': 3}.get(fixed, 0)
    saved = np.zeros((n_iter, num_kernels))
    old_norms = np.zeros((num_kernels, num_points))
    for it in range(n_iter):
        diff = np.expand_dims(pts, axis=2) - np.expand_dims(pts, axis=1)              # [nk, K, K, d]: x_i - x_j
        d2 = np.sum(np.power(diff, 2), axis=-1)
        grad = np.sum(diff / (np.power(np.expand_dims(d2, -1), 3 / 2) + 1e-6), axis=1) + 10 * pts
        if fixed == 'verticals':
            grad[:, 1:3, :-1] = 0
        norms = np.sqrt(np.sum(np.power(grad, 2), axis=-1))
        saved[it, :] = np.max(norms, axis=1)
        if np.max(np.abs(old_norms[:, first_moving:] - norms[:, first_moving:])) < thresh:
            break
        old_norms = norms
        dist = np.minimum(step * norms, clip)
        if fixed in ('center', 'verticals'):
            dist[:, 0] = 0
        pts -= np.expand_dims(dist, -1) * grad / np.expand_dims(norms + 1e-6, -1)
        step *= decay
    r = np.sqrt(np.sum(np.power(pts, 2), axis=-1))
    pts *= ratio / np.mean(r[:, 1:])
    return pts * radius, saved


def set_disposition(num_kpoints, fixed, points):
    """Supply the disposition of (num_kpoints, fixed) -- float [num_kpoints, 3] at radius 1 -- instead of having it made: it
    goes into the memo, `load_kernels` then draws the rotation and the noise alone.  For dispositions kept elsewhere (a file
    written by another tool) and for benchmarks and tests that do not care which disposition they run on.  (15, 'center') is
    the shipped table and cannot be replaced."""
    pts = np.array(points, np.float64)
    if fixed not in _FIXED or (num_kpoints == 15 and fixed == 'center') or pts.shape != (num_kpoints, 3) \
            or not np.isfinite(pts).all():
        raise ValueError("set_disposition: need finite [%d, 3] points for a fixed of %r other than (15, 'center')"
                         % (num_kpoints, _FIXED))
    _MEMO[(int(num_kpoints), fixed)] = pts


def _disposition(num_kpoints, fixed):
    """float64 [K, 3] at radius 1: the shipped table, the memo, the directory, or a fresh descent (in that order)"""
    if num_kpoints == 15 and fixed == 'center':
        return np.load(_TABLE)
    key = (num_kpoints, fixed)
    if key in _MEMO:
        return _MEMO[key].copy()
    folder = os.environ.get(DISPOSITION_DIR_ENV)
    path = os.path.join(folder, 'k_{:03d}_{:s}_3D.npy'.format(num_kpoints, fixed)) if folder else None
    if path and os.path.exists(path):
        pts = np.asarray(np.load(path), np.float64)
        if pts.shape != (num_kpoints, 3):
            raise ValueError("%s: expected a [%d, 3] disposition, got %s" % (path, num_kpoints, pts.shape))
    else:
        cand, grad_norms = kernel_point_optimization(1.0, num_kpoints, num_kernels=100, dimension=3, fixed=fixed)
        # the reference's choice (kernel_points.py:422): the LAST row, which is all zeros whenever the descent stopped before
        # iteration 9999 -- then candidate 0
        pts = cand[np.argmin(grad_norms[-1, :]), :, :]
        if path:
            os.makedirs(folder, exist_ok=True)
            tmp = path + ".tmp%d" % os.getpid()
            with open(tmp, "wb") as f:
                np.save(f, pts)
            os.replace(tmp, path)
    _MEMO[key] = pts.copy()
    return pts


def load_kernels(radius, num_kpoints, dimension, fixed, lloyd=False):
    if dimension != 3:
        raise NotImplementedError("kernel points: only 3-d dispositions (p_dim = 3) are built, got dimension %r" % (dimension,))
    if fixed not in _FIXED:
        raise ValueError("kernel points: fixed must be 'none', 'center' or 'verticals', got %r" % (fixed,))
    if lloyd or num_kpoints > 30:
        raise NotImplementedError("kernel points: the Lloyd dispositions (lloyd=True, more than 30 kernel points) are not "
                                  "built, got %d" % num_kpoints)
    if num_kpoints < 2 or (fixed == 'verticals' and num_kpoints < 4):
        raise ValueError("kernel points: %r needs at least %d kernel points, got %d"
                         % (fixed, 4 if fixed == 'verticals' else 2, num_kpoints))
    kernel_points = _disposition(int(num_kpoints), fixed)
    # (the reference tests fixed != 'vertical', singular: 'verticals' takes the z-rotation as well)
    theta = np.random.rand() * 2 * np.pi
    c, s = np.cos(theta), np.sin(theta)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float32)
    kernel_points = kernel_points + np.random.normal(scale=0.01, size=kernel_points.shape)
    kernel_points = radius * kernel_points
    kernel_points = np.matmul(kernel_points, R)
    return kernel_points.astype(np.float32)
