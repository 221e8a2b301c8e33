"""A float64 NumPy restatement of DESIGN section 19, the yardstick of csrc/posegraph.hip: open3d's
`get_information_matrix_from_point_clouds` and `global_optimization(GlobalOptimizationLevenbergMarquardt(),
GlobalOptimizationConvergenceCriteria(), option)`, and the reference's `full_registration` / `multiway_registration`
(FCGF_APR/lib/complement_data_loader.py:408-516) over `icp_oracle.icp`.  open3d itself is not installed, so this is a
restatement of the contract, not a recording of open3d's output; tests/test_posegraph_cpu.py holds it to an independent
scipy minimum of the equivalent Geman-McClure objective.
"""
import math

import numpy as np

from tests import icp_oracle as O

MAX_ITERATION, MAX_ITERATION_LM, MIN = 100, 20, 1e-6
PRUNE, PREFERENCE = 0.25, 1.0


# ---- information matrix ----
def information_sums(xyz):
    """The ten sums over matched target rows [K,3] (float32 values, products in float64), each by math.fsum (exact)."""
    q = np.asarray(xyz, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    terms = [np.ones(len(q)), x, y, z, x * x, y * y, z * z, x * y, x * z, y * z]
    return np.array([math.fsum(t) for t in terms]), np.array([math.fsum(np.abs(t)) for t in terms])


def information_from_sums(s):
    n, x, y, z, xx, yy, zz, xy, xz, yz = [float(v) for v in s]
    L = np.zeros((6, 6))
    L[:3, :3] = [[yy + zz, -xy, -xz], [-xy, xx + zz, -yz], [-xz, -yz, xx + yy]]
    L[3:, 3:] = n * np.eye(3)
    L[:3, 3:] = [[0, -z, y], [z, 0, -x], [-y, x, 0]]
    L[3:, :3] = L[:3, 3:].T
    return L


def information_rowwise(xyz):
    """sum G^T G built row by row from g1, g2, g3."""
    L = np.zeros((6, 6))
    for x, y, z in np.asarray(xyz, dtype=np.float64).reshape(-1, 3):
        G = np.array([[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]], dtype=np.float64)
        L += G.T @ G
    return L


def information_matrix(src, tgt, max_dist, T, tree=None):
    """-> (Lambda [6,6], corr int64 [n], sums [10], abs sums [10]) with apr_icp_batch's float32 association."""
    from scipy.spatial import cKDTree
    src, tgt = np.ascontiguousarray(src, dtype=np.float32), np.ascontiguousarray(tgt, dtype=np.float32)
    tree = cKDTree(tgt.astype(np.float64)) if tree is None else tree
    ev = O.evaluate(np.asarray(T, dtype=np.float64), src, tgt, tree, max_dist, True)
    s, sa = information_sums(tgt[ev["corr"][ev["corr"] >= 0]])
    return information_from_sums(s), ev["corr"], s, sa


# ---- pose <-> vector ----
def vec(M):
    sy = math.hypot(M[0, 0], M[1, 0])
    if sy >= 1e-6:
        a, b, g = math.atan2(M[2, 1], M[2, 2]), math.atan2(-M[2, 0], sy), math.atan2(M[1, 0], M[0, 0])
    else:
        a, b, g = math.atan2(-M[1, 2], M[1, 1]), math.atan2(-M[2, 0], sy), 0.0
    return np.array([a, b, g, M[0, 3], M[1, 3], M[2, 3]])


def mat(v):
    ca, sa, cb, sb, cg, sg = math.cos(v[0]), math.sin(v[0]), math.cos(v[1]), math.sin(v[1]), math.cos(v[2]), math.sin(v[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    M = np.eye(4)
    M[:3, :3] = Rz @ Ry @ Rx
    M[:3, 3] = v[3:6]
    return M


def _generators():
    out = []
    for a, b in ((1, 2), (2, 0), (0, 1)):          # unit skew matrices about x, y, z: O_0 has (1,2) = -1, (2,1) = +1
        Om = np.zeros((4, 4))
        Om[a, b], Om[b, a] = -1.0, 1.0
        out.append(Om)
    for d in range(3):
        Om = np.zeros((4, 4))
        Om[d, 3] = 1.0
        out.append(Om)
    return out


GENERATORS = _generators()


def lin(M):
    return np.array([(M[2, 1] - M[1, 2]) / 2, (M[0, 2] - M[2, 0]) / 2, (M[1, 0] - M[0, 1]) / 2, M[0, 3], M[1, 3], M[2, 3]])


class Edge:
    def __init__(self, source, target, T, info, uncertain):
        assert source < target
        self.s, self.t, self.uncertain = int(source), int(target), bool(uncertain)
        self.T = np.array(T, dtype=np.float64).reshape(4, 4)
        self.info = np.array(info, dtype=np.float64).reshape(6, 6)
        self.Ti = np.linalg.inv(self.T)


def edge_error(e, P):
    return vec(e.Ti @ np.linalg.inv(P[e.t]) @ P[e.s])


def edge_jacobian(e, P):
    X = e.Ti @ np.linalg.inv(P[e.t])
    Js = np.stack([lin(X @ Om @ P[e.s]) for Om in GENERATORS], 1)
    return Js


def odometry_chain(n, edges):
    """P_0 = I; odo <- T_(j,j+1) odo; P_(j+1) = odo^-1 (:426-438)."""
    odo, P = np.eye(4), [np.eye(4)]
    for j in range(n - 1):
        e = next(e for e in edges if e.s == j and e.t == j + 1)
        odo = e.T @ odo
        P.append(np.linalg.inv(odo))
    return P


def _mu(edges, mcd, preference=PREFERENCE):
    return preference * mcd * mcd * float(np.mean([e.info[5, 5] for e in edges])) if edges else 0.0


def _residual(errs, edges, conf, mu):
    tot = 0.0
    for e, er, l in zip(edges, errs, conf):
        r = float(er @ e.info @ er)
        tot += l * r + mu * (math.sqrt(l) - 1.0) ** 2 if e.uncertain else r
    return tot


def _system(P, edges, conf):
    N = 6 * len(P)
    H, b = np.zeros((N, N)), np.zeros(N)
    for e, l in zip(edges, conf):
        l = l if e.uncertain else 1.0
        er, Js = edge_error(e, P), edge_jacobian(e, P)
        Jt = -Js
        s, t = slice(6 * e.s, 6 * e.s + 6), slice(6 * e.t, 6 * e.t + 6)
        H[s, s] += l * Js.T @ e.info @ Js
        H[s, t] += l * Js.T @ e.info @ Jt
        H[t, s] += l * Jt.T @ e.info @ Js
        H[t, t] += l * Jt.T @ e.info @ Jt
        b[s] -= l * Js.T @ e.info @ er
        b[t] -= l * Jt.T @ e.info @ er
    return H, b


def _positive_definite(A):
    """The status-3 rule of DESIGN section 19.2: a Cholesky factorisation whose pivots are all positive and finite."""
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return False
    return bool(np.isfinite(L.diagonal()).all() and (L.diagonal() > 0.0).all())


def _optimize(P, edges, conf, mu, trace):
    """One LM optimisation with mu > 0.  -> (poses, confidences, outer iterations, failed).  `failed`: H + lambda I was not
    positive definite (status 3); the poses and confidences are those of the last accepted step.
    `trace` (dict) receives `steps`, one dict per inner pass, and `decisions`, one (name, outer iteration, inner count, lhs,
    rhs) per comparison the contract makes: max_b (lhs < rhs stops), delta (lhs < rhs stops), rho (lhs > rhs accepts),
    decrease and residual (lhs < rhs stops)."""
    steps, dec = trace.setdefault("steps", []), trace.setdefault("decisions", [])
    P, conf = [p.copy() for p in P], list(conf)
    errs = [edge_error(e, P) for e in edges]
    cur = _residual(errs, edges, conf, mu)
    H, b = _system(P, edges, conf)
    lam, ni = 1e-5 * H.diagonal().max(), 2.0
    dec.append(("max_b", -1, 0, float(b.max()), MIN))
    stop = b.max() < MIN
    failed = False
    # The factorisation reads the LOWER triangle of H + lambda I.  With every Lambda symmetric H is
    # symmetric up to rounding and the full matrix goes to the solver, as it always did; an unsymmetric Lambda makes
    # A_e = Js^T Lambda Js, and with it H, unsymmetric by more than rounding, and then the lower triangle is mirrored first.
    mirror = any(not np.array_equal(e.info, e.info.T) for e in edges)
    it = 0
    while it < MAX_ITERATION and not stop:
        count, rho = 0, 0.0
        while True:
            step = dict(outer=it, count=count, lam_before=lam, lam_after=lam, cur=cur, new=None, den=None, rho=None,
                        accepted=False, failed=False)
            steps.append(step)
            A = H + lam * np.eye(len(b))
            if mirror:
                A = np.tril(A) + np.tril(A, -1).T
            if not _positive_definite(A):
                failed = stop = step["failed"] = True
                w = np.linalg.eigvalsh(A, UPLO="L")                # the lower triangle, as the factorisation reads it
                step["eigenvalues"] = (float(w.min()), float(w.max()))
            else:
                d = np.linalg.solve(A, b)
                x = np.concatenate([vec(p) for p in P])
                dec.append(("delta", it, count, float(np.linalg.norm(d)), MIN * (float(np.linalg.norm(x)) + MIN)))
                stop = stop or np.linalg.norm(d) < MIN * (np.linalg.norm(x) + MIN)
            if not stop:
                Pn = [mat(d[6 * i:6 * i + 6]) @ P[i] for i in range(len(P))]
                errs_n = [edge_error(e, Pn) for e in edges]
                new = _residual(errs_n, edges, conf, mu)
                den = d @ (lam * d + b)
                rho = (cur - new) / (den + 1e-3)
                dec.append(("rho", it, count, float(rho), 0.0))
                step.update(new=new, den=float(den), rho=float(rho), accepted=bool(rho > 0))
                if rho > 0:
                    dec.append(("decrease", it, count, cur - new, MIN * cur))
                    dec.append(("residual", it, count, new, MIN))
                    stop = stop or (cur - new < MIN * cur) or (new < MIN)
                    P = Pn
                    lam *= max(1.0 / 3.0, min(1.0 - (2.0 * rho - 1.0) ** 3, 2.0 / 3.0))
                    ni = 2.0
                    cur = new
                    conf = [(mu / (mu + float(er @ e.info @ er))) ** 2 if e.uncertain else l
                            for e, er, l in zip(edges, errs_n, conf)]
                    errs = errs_n
                    H, b = _system(P, edges, conf)
                    dec.append(("max_b", it, count, float(b.max()), MIN))
                    stop = stop or b.max() < MIN
                else:
                    lam *= ni
                    ni *= 2.0
                step["lam_after"] = lam
            count += 1
            stop = stop or count > MAX_ITERATION_LM
            if rho > 0 or stop:
                break
        it += 1
    return P, conf, it, failed


def optimize_once(P, edges, conf, mcd, preference=PREFERENCE, trace=None):
    """One LM optimisation.  -> (poses, confidences, outer iterations), or None when mu = 0."""
    mu = _mu(edges, mcd, preference)
    if not (mu > 0.0):
        return None
    return _optimize(P, edges, conf, mu, {} if trace is None else trace)[:3]


def global_optimization(n, edges, mcd, init=None, edge_prune_threshold=PRUNE, preference_loop_closure=PREFERENCE):
    """-> dict(poses [n] of [4,4], confidence [ne] after the first pass, kept bool [ne], iterations (2), status, trace).
    trace: dict(passes = the traces of the passes that ran (see _optimize), prune = (confidence, threshold) of every
    uncertain edge after the first pass).  Status 3: the pass stops at the solve that failed and
    counts that outer iteration; after the first pass the confidences and flags are still those of its last accepted step."""
    P0 = [np.array(p, dtype=np.float64) for p in init] if init is not None else odometry_chain(n, edges)
    trace = dict(passes=[], prune=[])
    out = dict(poses=P0, confidence=np.ones(len(edges)), kept=np.ones(len(edges), dtype=bool), iterations=(0, 0), status=0,
               trace=trace)
    mu1 = _mu(edges, mcd, preference_loop_closure)
    if not (mu1 > 0.0):
        out["status"] = 1
        return out
    trace["passes"].append({})
    P1, conf1, it1, failed = _optimize(P0, edges, [1.0] * len(edges), mu1, trace["passes"][0])
    conf1 = np.array([c if e.uncertain else 1.0 for e, c in zip(edges, conf1)])
    trace["prune"] = [(float(c), edge_prune_threshold) for e, c in zip(edges, conf1) if e.uncertain]
    kept = np.array([not (e.uncertain and c < edge_prune_threshold) for e, c in zip(edges, conf1)])
    out.update(poses=P1, confidence=conf1, kept=kept, iterations=(it1, 0))
    if failed:
        out["status"] = 3
        return out
    sub = [e for e, k in zip(edges, kept) if k]
    mu2 = _mu(sub, mcd, preference_loop_closure)
    if not (mu2 > 0.0):
        out["status"] = 2
        return out
    trace["passes"].append({})
    P2, _, it2, failed = _optimize(P1, sub, [c for c, k in zip(conf1, kept) if k], mu2, trace["passes"][1])
    out.update(poses=P2, iterations=(it1, it2), status=3 if failed else 0)
    return out


def relative_poses(P):
    """:508-509: P_0^-1 P_i for i >= 1."""
    return [np.linalg.inv(P[0]) @ P[i] for i in range(1, len(P))]


# ---- synthetic graphs with the edges given directly ----
def cloud_information(n_points, seed):
    rng = np.random.default_rng(seed)
    pts = (rng.uniform(-1.0, 1.0, size=(n_points, 3)) * np.array([30.0, 30.0, 2.0])).astype(np.float32)
    return information_from_sums(information_sums(pts)[0])


def synthetic_graph(n, seed, planted=True, noise=(0.004, 0.02)):
    """A complete graph on n nodes along a drive (about 1 m and 1 degree per node).  Edge (s, t): T = G_t^-1 G_s disturbed by
    `noise` (metres, degrees), Lambda of a few thousand points.  `planted` (n >= 4): loop edge (0, n - 1) is off by 1.5 m
    and 12 degrees.  -> (edges, G ground-truth poses, index of the planted edge or None)."""
    rng = np.random.default_rng(seed)
    G = [np.eye(4)]
    for i in range(1, n):
        G.append(G[-1] @ O.perturbation(1.0 + 0.1 * rng.uniform(), 1.0 + rng.uniform(), seed * 100 + i))
    edges, bad = [], None
    for s in range(n):
        for t in range(s + 1, n):
            T = np.linalg.inv(G[t]) @ G[s]
            T = O.perturbation(noise[0] * rng.uniform(0.5, 1.0), noise[1] * rng.uniform(0.5, 1.0), seed * 1000 + 10 * s + t) @ T
            if planted and n >= 4 and (s, t) == (0, n - 1):
                T = O.perturbation(1.5, 12.0, seed + 7) @ T
                bad = len(edges)
            edges.append(Edge(s, t, T, cloud_information(3000 + 500 * ((s + t) % 3), seed * 50 + s * 8 + t), t != s + 1))
    return edges, G, bad


GRAPH_SIZES = (2, 4, 6, 8)
MCD_FINE = 0.075


def graph_batch():
    """The graphs of the GPU test: n = 2, 4, 6, 8, the n >= 4 ones with a planted bad loop edge."""
    return [synthetic_graph(n, 10 + n, planted=True) for n in GRAPH_SIZES]


# ---- the reference's multiway registration over the ICP restatement ----
def pairwise_init(pos_source, pos_target, velo2cam):
    """:410-411."""
    return (velo2cam @ pos_source.T @ np.linalg.inv(pos_target.T) @ np.linalg.inv(velo2cam)).T


def full_registration(clouds, inits, max_dist=0.2, max_dist_fine=MCD_FINE, max_iteration=200, trees=None):
    """:423-463 on already reduced clouds; inits[(s, t)] = M_st.  -> (poses, edges, global_optimization's dict)."""
    from scipy.spatial import cKDTree
    n = len(clouds)
    edges = []
    for s in range(n):
        for t in range(s + 1, n):
            tree = trees[t] if trees is not None else cKDTree(clouds[t].astype(np.float64))
            reg = O.icp(clouds[s], clouds[t], inits[(s, t)], max_dist, max_iteration, fp32_round=True, tree=tree)
            L, _, _, _ = information_matrix(clouds[s], clouds[t], max_dist_fine, reg["T"], tree=tree)
            edges.append(Edge(s, t, reg["T"], L, t != s + 1))
    res = global_optimization(n, edges, max_dist_fine)
    return res["poses"], edges, res


def multiway_registration(xyz_curr, xyz_cmpls, inits_left, inits_right, k, icp_voxel_size=0.05, max_dist=0.2,
                          max_dist_fine=MCD_FINE, max_iteration=200):
    """:494-509 without the caches.  -> (the 2k poses P_0^-1 P_i, left then right; the two result dicts)."""
    from scipy.spatial import cKDTree
    red = [x[O.voxel_first_rows(x, icp_voxel_size)] for x in [xyz_curr] + list(xyz_cmpls)]
    trees = [cKDTree(r.astype(np.float64)) for r in red]
    out, infos = [], []
    for side, inits in ((0, inits_left), (1, inits_right)):
        ids = [0] + [1 + side * k + i for i in range(k)]
        P, _, res = full_registration([red[i] for i in ids], inits, max_dist, max_dist_fine, max_iteration,
                                      trees=[trees[i] for i in ids])
        out += relative_poses(P)
        infos.append(res)
    return out, infos


# ---- the end-to-end case of tests/test_multiway_gpu.py ----
CASE_K = 2
CASE_XS = (0.0, -1.0, -2.0, 1.0, 2.0)        # key frame, left side (behind), right side (ahead), metres along the drive


def inits_from_key_poses(Ms):
    """apg.inits_from_key_poses: M_st = M_t^-1 M_s with M_0 = I."""
    Ms = [np.eye(4)] + [np.asarray(M, dtype=np.float64) for M in Ms]
    return {(s, t): np.linalg.inv(Ms[t]) @ Ms[s] for s in range(len(Ms)) for t in range(s + 1, len(Ms))}


def multiway_case(n_beams=16, n_azimuth=500, seed=3):
    """1 + 2k scans of synth.make_scene(seed) (16 beams x 500 azimuths: a few thousand rows after the 5 cm reduction), the
    ground-truth poses into the key frame, and the odometry poses: the truth disturbed by 0.08 m and 0.25 degrees.
    -> (frames [1 + 2k] float32, truth [2k], odometry [2k])."""
    from apr_amd import synth
    scene = synth.make_scene(seed)
    rng = np.random.default_rng(seed)
    frames = [synth.raycast(scene, (float(x), 0.0, 0.0), 0.0, rng, n_beams=n_beams, n_azimuth=n_azimuth) for x in CASE_XS]
    truth = []
    for x in CASE_XS[1:]:
        T = np.eye(4)
        T[0, 3] = float(x) - CASE_XS[0]
        truth.append(T)
    odometry = [O.perturbation(0.08, 0.25, 40 + i) @ T for i, T in enumerate(truth)]
    return frames, truth, odometry
