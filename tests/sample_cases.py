"""A small synthetic pair with complement frames for the training-sample tests: two key scans of one scene and, per key
scan, 2k scans taken 6 m apart behind and ahead of it (far enough for the crop to the key frame's radius to drop rows), with
the exact poses that move them into their key frame."""
import functools

import numpy as np

from apr_amd import synth


def _pose(x, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    W = np.eye(4)
    W[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    W[:3, 3] = [x, 0.0, 0.0]
    return W


@functools.lru_cache(None)
def scene_pair(seed=3, k=1, n_beams=16, n_azimuth=500):
    """-> dict(xyz_0, xyz_1, cmpl_0, cmpl_1 (2k scans each, behind first), M_0, M_1 (float64 [4,4] each), tsfm) with
    xyz_1 ~= xyz_0 @ R.T + t for tsfm = [R t]."""
    rng = np.random.default_rng(seed)
    scene = synth.make_scene(seed)
    scan = lambda W: synth.raycast(scene, W[:3, 3], np.arctan2(W[1, 0], W[0, 0]), rng, n_beams, n_azimuth)
    W0, W1 = _pose(0.0, 0.0), _pose(7.0, 0.08)
    out = dict(xyz_0=scan(W0), xyz_1=scan(W1), tsfm=np.linalg.inv(W1) @ W0)
    for name, W in (("0", W0), ("1", W1)):
        yaw = np.arctan2(W[1, 0], W[0, 0])
        steps = [-6.0 * (j + 1) for j in range(k)] + [6.0 * (j + 1) for j in range(k)]
        Wc = [_pose(W[0, 3] + d, yaw + 0.003 * d) for d in steps]
        out["cmpl_" + name] = [scan(w) for w in Wc]
        out["M_" + name] = [np.linalg.inv(W) @ w for w in Wc]
    return out
