"""Multiway registration on the HIP kernels of csrc/posegraph.hip against the float64 restatement (tests/posegraph_oracle.py,
itself held to scipy in tests/test_posegraph_cpu.py): the information matrices of a ragged batch, the pose-graph optimiser on
graphs whose edges are given directly, and apg.multiway_registration end to end."""
import functools

import numpy as np
import pytest
import torch

from tests import icp_oracle as O
from tests import posegraph_cases as C
from tests import posegraph_oracle as PG

pytestmark = pytest.mark.gpu

BAR_M, BAR_DEG = 1e-3, 1e-3          # end to end only: ICP's float32 association stands between it and the oracle
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


def _assert_info_problem(i, info, sums, corr, want):
    """One problem against the oracle: corr entry for entry, every sum within the worst case of a fixed-order float64 sum of
    n terms, Lambda the closed form of the kernel's own sums bit for bit and the oracle's within that bound."""
    L, c, sw, sa = want
    assert np.array_equal(corr, c), f"problem {i}"
    n = sw[0]
    assert sums[0] == n
    bound = n * 2.0 ** -52 * sa
    err = np.abs(sums - sw)
    print(f"problem {i}: n = {int(n)}, worst sum error / bound {np.max(err[1:] / np.maximum(bound[1:], 1e-300)):.3f}")
    assert (err <= bound).all(), f"problem {i}: {err} > {bound}"
    assert np.array_equal(info, PG.information_from_sums(sums)), f"problem {i}"
    assert (np.abs(info - L) <= np.abs(PG.information_from_sums(bound))).all(), f"problem {i}"


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
    for i, w in enumerate(want):
        _assert_info_problem(i, info[i], sums[i], corr[so[i]:so[i + 1]], w)
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


def test_information_optional_outputs(dev):
    """Without corr and without the sums: the same Lambda bits."""
    from apr_amd import ops
    tgts, srcs, Ts, _ = _info_case()
    top = list(INFO_TGT_OF_PROBLEM)
    info, _, _, (s, so, t, to) = _info_call(dev, srcs, tgts, top, Ts)
    bare, sums, corr = ops.information_batch(s, so, t, to, Ts, MAX_DIST, tgt_of_problem=top, want_corr=False, want_sums=False)
    assert sums is None and corr is None and np.array_equal(bare.cpu().numpy(), info)


PARTIAL_ROWS = (65536, 65537, 131073)        # 256, 257 and 513 partial rows: k_info_reduce's loop goes round 1, 2 and 3 times


@functools.lru_cache(maxsize=None)
def _partial_case():
    rng = np.random.default_rng(830)
    tgt = O.box_cloud(3000, 831)
    srcs = []
    for n in PARTIAL_ROWS:
        rows = rng.integers(0, len(tgt), size=n)
        srcs.append(np.ascontiguousarray((tgt[rows].astype(np.float64) + rng.normal(0.0, 0.005, size=(n, 3))).astype(np.float32)))
    Ts = np.tile(np.eye(4), (len(srcs), 1, 1))
    return tgt, srcs, Ts, [PG.information_matrix(s, tgt, MAX_DIST, np.eye(4)) for s in srcs]


def test_information_more_than_256_partial_rows(dev):
    tgt, srcs, Ts, want = _partial_case()
    assert [-(-n // 256) for n in PARTIAL_ROWS] == [256, 257, 513]
    top = [0, 0, 0]
    info, sums, corr, (s, so, t, to) = _info_call(dev, srcs, [tgt], top, Ts)
    for i, w in enumerate(want):
        assert w[2][0] > 0.9 * PARTIAL_ROWS[i]                     # nearly every row is matched: the sums are long
        _assert_info_problem(i, info[i], sums[i], corr[so[i]:so[i + 1]], w)
    for i in range(len(srcs)):
        a_info, a_sums, a_corr, _ = _info_call(dev, [srcs[i]], [tgt], None, Ts[i:i + 1])
        assert np.array_equal(a_info[0], info[i]) and np.array_equal(a_sums[0], sums[i]), f"problem {i} alone"
        assert np.array_equal(a_corr, corr[so[i]:so[i + 1]])
    info2, sums2, corr2, _ = _info_call(dev, srcs, [tgt], top, Ts)
    assert np.array_equal(info2, info) and np.array_equal(sums2, sums) and np.array_equal(corr2, corr)


@pytest.mark.parametrize("segments", [64, 3])
def test_information_at_the_problem_limit(dev, segments):
    """64 problems of 1 .. 300 rows: on 64 segments with the default mapping, and on 3 segments through tgt_of_problem."""
    rng = np.random.default_rng(840 + segments)
    tgts = [O.box_cloud(150 + 10 * (j % 7), 850 + j) for j in range(segments)]
    top = None if segments == 64 else [int(v) for v in rng.integers(0, segments, size=64)]
    sizes = [1, 300] + [int(v) for v in rng.integers(1, 301, size=62)]
    srcs, Ts = [], []
    for i, n in enumerate(sizes):
        tgt = tgts[i if top is None else top[i]]
        T = O.perturbation(0.2, 1.5, 860 + i)
        sel = tgt[rng.integers(0, len(tgt), size=n)].astype(np.float64) + rng.normal(0.0, 0.005, size=(n, 3))
        inv = np.linalg.inv(T)
        srcs.append(np.ascontiguousarray((sel @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)))
        Ts.append(T)
    Ts = np.stack(Ts)
    info, sums, corr, (s, so, t, to) = _info_call(dev, srcs, tgts, top, Ts)
    for i in (0, 31, 63):
        tgt = tgts[i if top is None else top[i]]
        _assert_info_problem(i, info[i], sums[i], corr[so[i]:so[i + 1]], PG.information_matrix(srcs[i], tgt, MAX_DIST, Ts[i]))
    for i in range(64):
        a_info, a_sums, a_corr, _ = _info_call(dev, [srcs[i]], [tgts[i if top is None else top[i]]], None, Ts[i:i + 1])
        assert np.array_equal(a_info[0], info[i]) and np.array_equal(a_sums[0], sums[i]), f"problem {i} alone"
        assert np.array_equal(a_corr, corr[so[i]:so[i + 1]]), f"problem {i} alone"


@pytest.mark.parametrize("kind", ["65_problems", "65_segments"])
def test_information_beyond_the_problem_limit_is_refused(dev, kind):
    """Argument checks on the host, before any launch (as test_icp_batch_gpu.py::test_batch_limits_are_refused)."""
    from apr_amd import _lib
    tgt, src = O.box_cloud(200, 870), O.box_cloud(200, 870)[:50]
    srcs, tgts, top = {"65_problems": ([src] * 65, [tgt], [0] * 65), "65_segments": ([src] * 3, [tgt] * 65, [0, 64, 1])}[kind]
    with pytest.raises(_lib.AprHipError, match="apr_information_batch"):
        _info_call(dev, srcs, tgts, top, np.tile(np.eye(4), (len(srcs), 1, 1)))


def _info_raw(dev, src, tgt, sentinel=-777.25):
    """apr_information_batch on one problem, T = I, into tensors pre-filled with a sentinel.  -> (rc, info, sums, corr)."""
    import ctypes
    from apr_amd import ops
    s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    so, to = np.array([0, len(src)], dtype=np.int64), np.array([0, len(tgt)], dtype=np.int64)
    T = torch.eye(4, dtype=torch.float64, device=dev).reshape(1, 16)
    info = torch.full((1, 6, 6), sentinel, dtype=torch.float64, device=dev)
    sums = torch.full((1, ops.INFORMATION_SUMS), sentinel, dtype=torch.float64, device=dev)
    corr = torch.full((len(src),), -7, dtype=torch.int32, device=dev)
    lib = ops._lib_()
    sb = int(lib.apr_information_scratch_bytes(len(src), len(tgt), 1))
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
    rc = lib.apr_information_batch(ops.ptr(s), so.ctypes.data_as(ctypes.c_void_p), ops.ptr(t), to.ctypes.data_as(ctypes.c_void_p),
                                   1, None, 1, ops.ptr(T), 16, float(MAX_DIST), ops.ptr(info), ops.ptr(sums), ops.ptr(corr),
                                   ops.ptr(scratch), sb, ops.stream())
    torch.cuda.synchronize()
    return rc, info.cpu().numpy(), sums.cpu().numpy(), corr.cpu().numpy()


def test_information_refused_grid_writes_nothing(dev):
    """A two-row target segment (0, 0, 0), (L, 0, 0) at max_dist = 0.075: the search cell is 1.01 x 0.075 and the grid refuses
    a segment of more than 40960 cells, about 3103 m.  L = 3200 is refused with APR_ERANGE and nothing is written; L = 3000
    is answered, both rows finding themselves; and a good call straight after the refused one is right (the pinned status
    word is reused)."""
    from apr_amd import _lib, ops
    cell = np.float32(MAX_DIST) * np.float32(1.01)
    assert np.float32(3200.0) / cell > 40960 * 1.02 and np.float32(3000.0) / cell < 40960 / 1.02       # in float32, 2 % clear
    far = np.array([[0, 0, 0], [3200.0, 0, 0]], dtype=np.float32)
    near = np.array([[0, 0, 0], [3000.0, 0, 0]], dtype=np.float32)
    rc, info, sums, corr = _info_raw(dev, far, far)
    assert rc == -3                                              # APR_ERANGE
    assert (info == -777.25).all() and (sums == -777.25).all() and (corr == -7).all()
    with pytest.raises(_lib.AprHipError, match=r"error -3: apr_information_batch: search grid refused"):
        ops.check(rc)
    rc, info, sums, corr = _info_raw(dev, near, near)
    want = PG.information_matrix(near, near, MAX_DIST, np.eye(4))
    assert rc == 0 and np.array_equal(want[1], [0, 1])
    _assert_info_problem(0, info[0], sums[0], corr.astype(np.int64), want)
    # through the wrapper: refused, then right
    s, t = torch.from_numpy(far).to(dev), torch.from_numpy(far).to(dev)
    with pytest.raises(_lib.AprHipError, match="search grid refused"):
        ops.information_batch(s, [0, 2], t, [0, 2], np.eye(4)[None], MAX_DIST)
    info2, _, corr2, _ = _info_call(dev, [near], [near], None, np.eye(4)[None])
    assert np.array_equal(info2[0], info[0]) and np.array_equal(corr2, [0, 1])


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
        assert tuple(iters[g]) == tuple(w["iterations"]), (g, iters[g], w["iterations"])
        worst = C.compare(C.result_of(P, c, k, iters[g], status[g]), w, C.BAR)
        print(f"graph {g}: worst difference from the oracle {worst:.2e} (bar {C.BAR:.0e})")
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
