"""Float64 NumPy restatement of `apr_fcgf_test_pair`'s record (include/apr_hip.h), operation by operation where the header
states the order, and a float32 restatement of the `dists` row.  Shared by tests/test_fcgf_tester_cpu.py and
tests/test_fcgf_test_pair_gpu.py."""
import struct

import numpy as np

HIT_LEVELS = [k * 0.1 for k in range(1, 11)]      # the Python doubles the tables of test_apr.py:200-213 compare with
CHUNK = 1 << 20


def pack_raw(T, it=4242, inliers=37, err2=1.2345, total_valid=777):
    """The raw RANSAC result as the library leaves it: double T[12], long long it, int inliers, int pad, double err2, then
    long long total_valid -> uint8 [136]."""
    raw = struct.pack("<12dqiidq", *np.asarray(T, np.float64)[:3].reshape(12), it, inliers, 0, err2, total_valid)
    return np.frombuffer(raw, np.uint8).copy()


def _rows(idx, n):
    idx = np.asarray(idx, np.int64)
    bad = (idx < 0) | (idx >= n)
    return np.where(bad, 0, idx), int(bad.sum())


def find_corr_rows(n0, n1, sel0, sel1, nn):
    """-> (source rows, target rows, entries out of range): xyz0[sel0] <-> xyz1[sel1[nn]], an entry out of range reads row 0."""
    m0 = n0 if sel0 is None else len(sel0)
    m1 = n1 if sel1 is None else len(sel1)
    a, bad_a = (np.arange(m0), 0) if sel0 is None else _rows(sel0, n0)
    b, bad_b = _rows(nn, m1)
    bad_c = 0
    if sel1 is not None:
        b, bad_c = _rows(np.asarray(sel1, np.int64)[b], n1)
    return a, b, bad_a + bad_b + bad_c


def dists_f32(xyz0, xyz1, a, b, T_gt32):
    """evaluate_nn_dist in float32 NumPy, every operation rounded, in the order of csrc/inlier_dist.h."""
    f = np.float32
    p, t = xyz0[a].astype(f), xyz1[b].astype(f)
    R, tr = T_gt32[:3, :3].astype(f), T_gt32[:3, 3].astype(f)
    q = [((R[k, 0] * p[:, 0] + R[k, 1] * p[:, 1]) + R[k, 2] * p[:, 2]) + tr[k] for k in range(3)]
    dx, dy, dz = q[0] - t[:, 0], q[1] - t[:, 1], q[2] - t[:, 2]
    s = (dx * dx + dy * dy) + dz * dz
    assert s.dtype == f
    return np.sqrt(s + f(1e-6))


def _dist64(p, t, T):
    return np.linalg.norm(p.astype(np.float64) @ T[:3, :3].T + T[:3, 3] - t.astype(np.float64), axis=1)


def restate(xyz0, xyz1, sel0, sel1, nn, r0, r1, corr, T_gt32, T_raw, total_valid, max_iter, rte_thresh=2, rre_thresh_deg=5):
    """-> dict of the record's figures.  T_raw: the float64 pose of the raw result; T_gt32: float32 [4,4]."""
    E = np.asarray(T_raw, np.float64).astype(np.float32).astype(np.float64)      # T_ransac, widened
    E[3] = [0, 0, 0, 1]
    G = np.asarray(T_gt32, np.float32).astype(np.float64)
    tr = 0.0
    for i in range(3):
        row = 0.0
        for k in range(3):
            row = row + float(E[i, k]) * float(G[i, k])
        tr = tr + row
    arg = (tr - 1.0) / 2.0
    with np.errstate(invalid="ignore"):
        rre = float(np.arccos(arg))
    e2 = g2 = 0.0
    for i in range(3):
        d = float(E[i, 3]) - float(G[i, 3])
        e2, g2 = e2 + d * d, g2 + float(G[i, 3]) * float(G[i, 3])
    rte = float(np.sqrt(e2))
    ok = float(rte < rte_thresh and rre == rre and rre < np.pi / 180 * rre_thresh_deg)
    a, b, bad = find_corr_rows(len(xyz0), len(xyz1), sel0, sel1, nn)
    d_nn = np.sqrt(_dist64(xyz0[a], xyz1[b], G) ** 2 + 1e-6)
    j, bad_corr = _rows(corr, len(r1))
    return dict(rte=rte, arg=arg, rre=rre, ok=ok, dist=float(np.sqrt(g2)), m0=len(a), k0=len(r0), k1=len(r1), bad=bad + bad_corr,
                T=E, overflow=float(total_valid > CHUNK and max_iter > CHUNK), d_est=_dist64(r0, r1[j], E),
                d_gt=_dist64(r0, r1[j], G), d_nn=d_nn, hits=[int((d_nn < t).sum()) for t in HIT_LEVELS],
                d32=dists_f32(xyz0, xyz1, a, b, np.asarray(T_gt32, np.float32)))
