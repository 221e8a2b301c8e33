"""The float64 restatement of DESIGN section 19 (tests/posegraph_oracle.py) held to checks of its own, without a GPU: the
closed form of the information matrix against sum G^T G row by row, the LM result against an independent
scipy.optimize.least_squares minimum of the equivalent Geman-McClure objective, the confidence margin the GPU test relies
on, and the two formulas around the optimiser against lines of the reference (tests/golden/multiway_ref.npz)."""
import functools
import os

import numpy as np
import pytest

from tests import icp_oracle as O
from tests import posegraph_oracle as PG

BAR_M, BAR_DEG = 1e-3, 1e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multiway_ref.npz")


def test_information_closed_form_equals_the_row_wise_sum():
    rng = np.random.default_rng(0)
    for n in (0, 1, 7, 500):
        pts = (rng.uniform(-1, 1, size=(n, 3)) * np.array([40.0, 40.0, 3.0])).astype(np.float32)
        closed = PG.information_from_sums(PG.information_sums(pts)[0])
        rowwise = PG.information_rowwise(pts)
        scale = max(1.0, float(np.abs(rowwise).max()))
        assert np.abs(closed - rowwise).max() <= 1e-12 * scale, n
        assert np.array_equal(closed, closed.T)
    assert np.array_equal(PG.information_from_sums(np.zeros(10)), np.zeros((6, 6)))


def test_vec_and_mat_are_inverse_and_the_jacobian_is_the_derivative():
    rng = np.random.default_rng(1)
    for _ in range(5):
        v = rng.uniform(-1, 1, size=6) * np.array([0.5, 0.5, 0.5, 3, 3, 3])
        assert np.abs(PG.vec(PG.mat(v)) - v).max() < 1e-12
    edges, G, _ = PG.synthetic_graph(4, 3, planted=False)
    P = PG.odometry_chain(4, edges)
    e = edges[1]
    Js = PG.edge_jacobian(e, P)
    # the columns are the derivative of the LINEARISED error lin(T_e^-1 P_t^-1 exp(h O_i) P_s): compare by finite differences
    for i in range(6):
        h = 1e-6
        d = np.zeros(6)
        d[i] = h
        Pp = [p.copy() for p in P]
        Pp[e.s] = PG.mat(d) @ P[e.s]
        num = (PG.lin(e.Ti @ np.linalg.inv(Pp[e.t]) @ Pp[e.s]) - PG.lin(e.Ti @ np.linalg.inv(P[e.t]) @ P[e.s])) / h
        assert np.abs(num - Js[:, i]).max() < 1e-5


@functools.lru_cache(maxsize=None)
def _solved(n, planted):
    edges, G, bad = PG.synthetic_graph(n, 10 + n, planted=planted)
    return edges, G, bad, PG.global_optimization(n, edges, PG.MCD_FINE)


def _scipy_minimum(n, edges, mcd):
    """Geman-McClure: sum_certain r + sum_uncertain mu r / (mu + r), r = e^T Lambda e, node 0 fixed at the identity; started
    from the odometry chain.  As least squares: the residual of an edge is C^T e (Lambda = C C^T), scaled by
    sqrt(mu / (mu + r)) when the edge is uncertain."""
    from scipy.optimize import least_squares
    mu = PG.PREFERENCE * mcd * mcd * float(np.mean([e.info[5, 5] for e in edges]))
    chol = [np.linalg.cholesky(e.info) for e in edges]

    def poses(x):
        return [np.eye(4)] + [PG.mat(x[6 * i:6 * i + 6]) for i in range(n - 1)]

    def fun(x):
        P = poses(x)
        out = []
        for e, C in zip(edges, chol):
            w = C.T @ PG.edge_error(e, P)
            if e.uncertain:
                w = w * np.sqrt(mu / (mu + float(w @ w)))
            out.append(w)
        return np.concatenate(out)

    x0 = np.concatenate([PG.vec(p) for p in PG.odometry_chain(n, edges)[1:]])
    res = least_squares(fun, x0, xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=1.0, method="trf")
    return poses(res.x)


@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("n", PG.GRAPH_SIZES)
def test_lm_agrees_with_scipy_geman_mcclure_minimum(n, planted):
    """The second pass minimises the objective over the kept edges with mu taken over them; scipy gets exactly those."""
    edges, G, bad, res = _solved(n, planted)
    assert res["status"] == 0
    kept = [e for e, k in zip(edges, res["kept"]) if k]
    want = PG.relative_poses(_scipy_minimum(n, kept, PG.MCD_FINE))
    got = PG.relative_poses(res["poses"])
    for i, (a, b) in enumerate(zip(got, want)):
        rte, rre = O.pose_error(a, b)
        print(f"n = {n}, planted {planted}, node {i + 1}: {rte:.2e} m / {rre:.2e} deg, iterations {res['iterations']}")
        assert rte < BAR_M and rre < BAR_DEG
    if planted and n >= 4:
        assert not res["kept"][bad] and res["kept"].sum() == len(edges) - 1
    else:
        assert res["kept"].all()


@pytest.mark.parametrize("n", [m for m in PG.GRAPH_SIZES if m >= 4])
def test_planted_cases_keep_clear_of_the_prune_threshold(n):
    """The GPU test compares kept / pruned flags exactly: no first-pass confidence may lie in [0.15, 0.35]."""
    edges, _, bad, res = _solved(n, True)
    c = res["confidence"]
    print(f"n = {n}: planted {c[bad]:.3e}, smallest other {np.delete(c, bad).min():.4f}")
    assert not ((c >= 0.15) & (c <= 0.35)).any()
    assert c[bad] < 0.15 and np.delete(c, bad).min() > 0.35


def test_two_node_graph_returns_its_edge_and_zero_information_is_refused():
    edges, _, _, res = _solved(2, True)
    assert np.abs(PG.relative_poses(res["poses"])[0] - np.linalg.inv(edges[0].T)).max() < 1e-12
    edges4 = [PG.Edge(e.s, e.t, e.T, np.zeros((6, 6)), e.uncertain) for e in PG.synthetic_graph(4, 14)[0]]
    res = PG.global_optimization(4, edges4, PG.MCD_FINE)
    assert res["status"] == 1
    for a, b in zip(res["poses"], PG.odometry_chain(4, edges4)):
        assert np.array_equal(a, b)


def test_pairwise_init_and_final_product_equal_the_reference_lines():
    g = np.load(GOLDEN)
    for (s, t), want in zip(g["pairs"], g["inits"]):
        assert np.array_equal(PG.pairwise_init(g["pos"][s], g["pos"][t], g["velo2cam"]), want)
    got = PG.relative_poses(list(g["left"])) + PG.relative_poses(list(g["right"]))
    assert np.array_equal(np.stack(got), g["products"])
    # the package's own host functions are the same formulas
    from apr_amd.fcgf.lib import apg
    for (s, t), want in zip(g["pairs"], g["inits"]):
        assert np.array_equal(apg.pairwise_init(g["pos"][s], g["pos"][t], g["velo2cam"]), want)
    side = apg.pairwise_inits(list(g["pos"][:4]), g["velo2cam"])
    assert sorted(side) == [(s, t) for s in range(4) for t in range(s + 1, 4)]
    assert np.array_equal(side[(1, 3)], PG.pairwise_init(g["pos"][1], g["pos"][3], g["velo2cam"]))
    Ms = [PG.pairwise_init(g["pos"][i], g["pos"][0], g["velo2cam"]) for i in (1, 2, 3)]
    for (s, t), M in apg.inits_from_key_poses(Ms).items():
        assert np.abs(M - PG.pairwise_init(g["pos"][s], g["pos"][t], g["velo2cam"])).max() < 1e-12


def test_values_the_kernel_does_not_take_are_refused():
    from apr_amd.fcgf import registration as R
    pg = R.PoseGraph()
    pg.nodes = [R.PoseGraphNode(), R.PoseGraphNode()]
    pg.edges = [R.PoseGraphEdge(0, 1, np.eye(4), np.eye(6), uncertain=False)]
    for kw in (dict(criteria=R.GlobalOptimizationConvergenceCriteria(max_iteration=50)),
               dict(criteria=R.GlobalOptimizationConvergenceCriteria(min_residual=1e-9)),
               dict(method=object()),
               dict(option=R.GlobalOptimizationOption(reference_node=1))):
        with pytest.raises(NotImplementedError):
            R.global_optimization(pg, **kw)
    pg.nodes = [R.PoseGraphNode() for _ in range(9)]
    with pytest.raises(NotImplementedError):
        R.global_optimization(pg)
    with pytest.raises(TypeError):
        R.GlobalOptimizationConvergenceCriteria(max_iterations=5)


def test_full_registration_on_small_clouds():
    """full_registration over icp_oracle.icp: three box clouds a few centimetres apart come back within the pose bar."""
    base = O.box_cloud(1500, 700)
    G = [np.eye(4), O.perturbation(0.06, 0.4, 1), O.perturbation(0.09, 0.7, 2)]
    clouds = [base] + [O.apply_transform(base, np.linalg.inv(g)) for g in G[1:]]
    inits = {(s, t): np.eye(4) for s in range(3) for t in range(s + 1, 3)}
    P, edges, res = PG.full_registration(clouds, inits)
    assert res["status"] == 0 and len(edges) == 3 and [e.uncertain for e in edges] == [False, True, False]
    for got, want in zip(PG.relative_poses(P), G[1:]):
        rte, rre = O.pose_error(got, want)
        assert rte < 5e-3 and rre < 5e-2, (rte, rre)
