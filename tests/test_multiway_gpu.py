"""Multiway registration on the HIP kernels of csrc/posegraph.hip against the float64 restatement (tests/posegraph_oracle.py,
itself held to scipy in tests/test_posegraph_cpu.py): the information matrices of a ragged batch, the pose-graph optimiser on
graphs whose edges are given directly, and apg.multiway_registration end to end."""
import functools

import numpy as np
import pytest
import torch

from tests import icp_oracle as O
from tests import posegraph_oracle as PG

pytestmark = pytest.mark.gpu

BAR_M, BAR_DEG = 1e-3, 1e-3
MAX_DIST = 0.075


# ---- information matrices ----
INFO_TGT_ROWS, INFO_TGT_SEEDS = (6000, 700, 1900), (800, 801, 802)
INFO_SRC_ROWS = (1, 63, 64, 65, 257, 5000)
INFO_TGT_OF_PROBLEM = (2, 1, 0, 1, 2, 0)
INFO_FAR, INFO_EDGE = 1, 3          # problem 1 has no correspondence; problem 3 carries the rim and the tie rows


@functools.lru_cache(maxsize=None)
def _info_case():
    """Three box targets; the source of problem i is a sample of its target's rows with 5 mm noise, moved by the inverse of
    T_i, so that T_i brings every row back to within reach of its own target row.
    Problem 1 is moved 50 m away instead (no correspondence).  Problem 3 has T = I, and three isolated target rows appended
    to its segment (segment 1) at z = 50 m: A = (0, 0, 50), B = (0.0625, 10, 50), C = (0, 10, 50), in that row order.  Its
    last three source rows are (r, 0, 50) with r = float32(0.075): d = r exactly in float32, NOT matched (strict bound);
    (r - 1 ulp, 0, 50): matched to A; (0.03125, 10, 50): exactly 0.03125 from B and from C, matched to B, the smaller row."""
    rng = np.random.default_rng(810)
    tgts = [O.box_cloud(m, s) for m, s in zip(INFO_TGT_ROWS, INFO_TGT_SEEDS)]
    tgts[1] = np.concatenate([tgts[1], np.array([[0, 0, 50], [0.0625, 10, 50], [0, 10, 50]], dtype=np.float32)])
    r = np.float32(MAX_DIST)
    srcs, Ts = [], []
    for i, (n, seg) in enumerate(zip(INFO_SRC_ROWS, INFO_TGT_OF_PROBLEM)):
        T = np.eye(4) if i == INFO_EDGE else O.perturbation(0.3 + 0.1 * i, 2.0 + i, 820 + i)
        rows = rng.choice(INFO_TGT_ROWS[seg], size=n, replace=False)
        s = tgts[seg][rows].astype(np.float64) + rng.normal(0.0, 0.005, size=(n, 3))
        if i == INFO_FAR:
            s += 50.0
        inv = np.linalg.inv(T)
        s = (s @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
        if i == INFO_EDGE:
            s[-3:] = np.array([[r, 0, 50], [np.nextafter(r, np.float32(0)), 0, 50], [0.03125, 10, 50]], dtype=np.float32)
        srcs.append(np.ascontiguousarray(s))
        Ts.append(T)
    want = [PG.information_matrix(s, tgts[seg], MAX_DIST, T) for s, seg, T in zip(srcs, INFO_TGT_OF_PROBLEM, Ts)]
    return tgts, srcs, np.stack(Ts), want


def _info_call(dev, srcs, tgts, top, Ts):
    from apr_amd import ops
    s = torch.from_numpy(np.concatenate(srcs)).to(dev)
    t = torch.from_numpy(np.concatenate(tgts)).to(dev)
    so = np.concatenate([[0], np.cumsum([len(x) for x in srcs])])
    to = np.concatenate([[0], np.cumsum([len(x) for x in tgts])])
    info, sums, corr = ops.information_batch(s, so, t, to, Ts, MAX_DIST, tgt_of_problem=top, want_corr=True, want_sums=True)
    return info.cpu().numpy(), sums.cpu().numpy(), corr.cpu().numpy().astype(np.int64), (s, so, t, to)


def test_information_ragged_batch(dev):
    from apr_amd import ops
    from apr_amd.fcgf import registration
    tgts, srcs, Ts, want = _info_case()
    top = list(INFO_TGT_OF_PROBLEM)
    info, sums, corr, (s, so, t, to) = _info_call(dev, srcs, tgts, top, Ts)
    # the association is apr_icp_batch's evaluation step: corr and n entry for entry
    rec, corr_icp = ops.icp_batch(s, so, t, to, Ts, MAX_DIST, max_iteration=0, tgt_of_problem=top, want_corr=True)
    assert np.array_equal(corr, corr_icp.cpu().numpy())
    assert np.array_equal(sums[:, 0], rec[:, ops.ICP_N_CORR].cpu().numpy())
    for i, (L, c, sw, sa) in enumerate(want):
        ci = corr[so[i]:so[i + 1]]
        assert np.array_equal(ci, c), f"problem {i}"
        n = sw[0]
        assert sums[i, 0] == n
        bound = n * 2.0 ** -52 * sa                      # the worst case of a fixed-order float64 sum of n terms
        err = np.abs(sums[i] - sw)
        print(f"problem {i}: n = {int(n)}, worst sum error / bound {np.max(err[1:] / np.maximum(bound[1:], 1e-300)):.3f}")
        assert (err <= bound).all(), f"problem {i}: {err} > {bound}"
        # the layout: Lambda is the closed form of the kernel's own sums, bit for bit, and the oracle's within the bound
        assert np.array_equal(info[i], PG.information_from_sums(sums[i])), f"problem {i}"
        assert (np.abs(info[i] - L) <= np.abs(PG.information_from_sums(bound))).all(), f"problem {i}"
    assert sums[INFO_FAR, 0] == 0 and (corr[so[INFO_FAR]:so[INFO_FAR + 1]] == -1).all()
    assert np.array_equal(info[INFO_FAR], np.zeros((6, 6))) and np.array_equal(sums[INFO_FAR], np.zeros(10))
    m1 = len(tgts[1])
    assert corr[so[INFO_EDGE + 1] - 3:so[INFO_EDGE + 1]].tolist() == [-1, m1 - 3, m1 - 2]
    # alone = inside the batch, and run to run
    for i in range(len(srcs)):
        a_info, a_sums, a_corr, _ = _info_call(dev, [srcs[i]], [tgts[top[i]]], None, Ts[i:i + 1])
        assert np.array_equal(a_info[0], info[i]) and np.array_equal(a_sums[0], sums[i]), f"problem {i} alone"
        assert np.array_equal(a_corr, corr[so[i]:so[i + 1]])
    info2, sums2, corr2, _ = _info_call(dev, srcs, tgts, top, Ts)
    assert np.array_equal(info2, info) and np.array_equal(sums2, sums) and np.array_equal(corr2, corr)
    # ICP's records as they lie (stride 20) give the same bits as the 4x4 transforms, and so does the open3d-shaped entry
    info3, _, _ = ops.information_batch(s, so, t, to, rec, MAX_DIST, tgt_of_problem=top)
    assert np.array_equal(info3.cpu().numpy(), info)
    one = registration.get_information_matrix_from_point_clouds(srcs[4], tgts[top[4]], MAX_DIST, Ts[4])
    assert one.shape == (6, 6) and one.dtype == np.float64 and np.array_equal(one, info[4])


# ---- the optimiser ----
@functools.lru_cache(maxsize=None)
def _graphs():
    """n = 2, 4, 6, 8 (a planted bad loop edge for n >= 4), and a 4-node graph whose information matrices are all zero.
    -> (graphs [(n, edges)], the oracle's result per graph)."""
    graphs = [(n, edges) for n, (edges, _, _) in zip(PG.GRAPH_SIZES, PG.graph_batch())]
    zero = [PG.Edge(e.s, e.t, e.T, np.zeros((6, 6)), e.uncertain) for e in PG.synthetic_graph(4, 30)[0]]
    graphs.append((4, zero))
    return graphs, [PG.global_optimization(n, edges, PG.MCD_FINE) for n, edges in graphs]


def _optimize(graphs, init=None):
    from apr_amd import ops
    layout = ops.PoseGraphLayout([(n, [(e.s, e.t, e.uncertain) for e in edges]) for n, edges in graphs], need_chain=init is None)
    T = np.stack([e.T for _, edges in graphs for e in edges])
    info = np.stack([e.info for _, edges in graphs for e in edges])
    out = ops.posegraph_optimize(layout, T, info, init, PG.MCD_FINE)
    return [x.cpu().numpy() for x in out], layout


def test_posegraph_batch(dev):
    graphs, want = _graphs()
    (poses, conf, kept, iters, status), layout = _optimize(graphs)
    no, eo = layout.node_off_host, layout.edge_off_host
    print("iterations", iters.tolist(), "oracle", [w["iterations"] for w in want], "status", status.tolist())
    for g, ((n, edges), w) in enumerate(zip(graphs, want)):
        P, c, k = poses[no[g]:no[g + 1]], conf[eo[g]:eo[g + 1]], kept[eo[g]:eo[g + 1]]
        assert status[g] == w["status"], g
        if w["status"] != 0:
            continue
        for i, (a, b) in enumerate(zip(PG.relative_poses(list(P)), PG.relative_poses(w["poses"]))):
            rte, rre = O.pose_error(a, b)
            assert rte < BAR_M and rre < BAR_DEG, (g, i, rte, rre)
        assert np.array_equal(k != 0, w["kept"]), g
        print(f"graph {g}: worst confidence difference {np.abs(c - w['confidence']).max():.2e}")
        assert np.abs(c - w["confidence"]).max() <= 1e-6, g
    # n = 2: the graph returns its edge
    e = graphs[0][1][0]
    assert np.abs(np.linalg.inv(poses[0]) @ poses[1] - np.linalg.inv(e.T)).max() <= 1e-12
    assert kept[0] == 1 and conf[0] == 1.0
    # the planted edges are pruned, nothing else is
    for g, (_, _, bad) in enumerate(PG.graph_batch()):
        k = kept[eo[g]:eo[g + 1]]
        assert k.sum() == len(k) - (bad is not None) and (bad is None or k[bad] == 0)
    # all-zero Lambda: the initial poses (the odometry chain) and a status, no division
    z = len(graphs) - 1
    assert status[z] == 1 and want[z]["status"] == 1 and np.isfinite(poses).all()
    for a, b in zip(poses[no[z]:no[z + 1]], PG.odometry_chain(4, graphs[z][1])):
        assert np.abs(a - b).max() <= 1e-12
    # alone = inside the batch, and run to run
    for g in range(len(graphs)):
        (p1, c1, k1, i1, s1), _ = _optimize([graphs[g]])
        assert np.array_equal(p1, poses[no[g]:no[g + 1]]) and np.array_equal(c1, conf[eo[g]:eo[g + 1]]), g
        assert np.array_equal(k1, kept[eo[g]:eo[g + 1]]) and np.array_equal(i1[0], iters[g]) and s1[0] == status[g], g
    (p2, c2, k2, i2, s2), _ = _optimize(graphs)
    assert np.array_equal(p2, poses) and np.array_equal(c2, conf) and np.array_equal(k2, kept) and np.array_equal(i2, iters)


def test_posegraph_given_initial_poses_and_the_open3d_shaped_entry(dev):
    from apr_amd.fcgf import registration as R
    graphs, want = _graphs()
    n, edges = graphs[1]
    init = np.stack(PG.odometry_chain(n, edges))
    (poses, conf, kept, iters, status), _ = _optimize([graphs[1]], init)
    (poses_c, conf_c, _, _, _), _ = _optimize([graphs[1]])
    for a, b in zip(PG.relative_poses(list(poses)), PG.relative_poses(list(poses_c))):
        rte, rre = O.pose_error(a, b)
        assert rte < 1e-9 and rre < 1e-6          # the chain built in the kernel and the one handed in differ by rounding
    pg = R.PoseGraph()
    pg.nodes = [R.PoseGraphNode(p) for p in init]
    pg.edges = [R.PoseGraphEdge(e.s, e.t, e.T, e.info, uncertain=e.uncertain) for e in edges]
    res = R.global_optimization(pg, R.GlobalOptimizationLevenbergMarquardt(), R.GlobalOptimizationConvergenceCriteria(),
                                R.GlobalOptimizationOption(max_correspondence_distance=PG.MCD_FINE, edge_prune_threshold=0.25,
                                                           reference_node=0))
    assert res["status"] == 0 and res["iterations"] == tuple(iters[0])
    assert np.array_equal(np.stack([nd.pose for nd in pg.nodes]), poses)
    assert len(pg.edges) == int(kept.sum()) == len(edges) - 1
    assert [e.confidence for e in pg.edges] == [c for c, k in zip(conf, kept) if k]
    with pytest.raises(NotImplementedError):
        R.global_optimization(pg, criteria=R.GlobalOptimizationConvergenceCriteria(max_iteration=50))
    with pytest.raises(NotImplementedError):
        R.global_optimization(pg, method=object())


# ---- end to end ----
@functools.lru_cache(maxsize=None)
def _e2e_oracle():
    frames, truth, odo = PG.multiway_case()
    k = PG.CASE_K
    poses, infos = PG.multiway_registration(frames[0], frames[1:], PG.inits_from_key_poses(odo[:k]),
                                            PG.inits_from_key_poses(odo[k:]), k)
    return frames, truth, odo, poses, infos


def test_multiway_registration_end_to_end(dev):
    from apr_amd.fcgf.lib import apg
    frames, truth, odo, want, infos = _e2e_oracle()
    k = PG.CASE_K
    key, cmpls = torch.from_numpy(frames[0]).to(dev), [torch.from_numpy(f).to(dev) for f in frames[1:]]
    poses, graph = apg.multiway_registration(key, cmpls, apg.inits_from_key_poses(odo[:k]), apg.inits_from_key_poses(odo[k:]),
                                             k, return_graph=True)
    assert len(poses) == 2 * k and (graph["status"] == 0).all()
    print("ICP iterations", graph["records"][..., 19].astype(int).tolist(), "LM iterations", graph["iterations"].tolist(),
          "oracle", [r["iterations"] for r in infos])
    for i, (p, w, g, m) in enumerate(zip(poses, want, truth, odo)):
        rte, rre = O.pose_error(p, w)
        (te, re), (t0, r0) = O.pose_error(p, g), O.pose_error(m, g)
        print(f"pose {i}: {rte:.2e} m / {rre:.2e} deg from the oracle; {te:.4f} m / {re:.4f} deg from the truth, odometry "
              f"{t0:.4f} m / {r0:.4f} deg")
        assert rte < BAR_M and rre < BAR_DEG, i
        assert te <= t0 and re <= r0, i
    # the APG built through refine='multiway' is the APG of those poses, bit for bit
    a_xyz, a_sel = apg.aggregate_frames(key, cmpls, poses, 0.3)
    b_xyz, b_sel = apg.aggregate_frames(key, cmpls, odo, 0.3, refine='multiway')
    assert torch.equal(a_xyz, b_xyz) and torch.equal(a_sel, b_sel)
    # one side through full_registration is that side of the batch
    side = apg.full_registration([key[apg.voxel_first_rows([key], 0.05)[0]]] +
                                 [c[s] for c, s in zip(cmpls[:k], apg.voxel_first_rows(cmpls[:k], 0.05))],
                                 apg.inits_from_key_poses(odo[:k]))
    for i in range(k):
        assert np.array_equal(np.linalg.inv(side[0]) @ side[i + 1], poses[i])
