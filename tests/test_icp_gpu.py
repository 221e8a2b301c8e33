"""ICP pose refinement on the HIP kernels (csrc/icp.hip, ops.icp_batch, registration.registration_icp, apg.refine_*) against
the host restatement of open3d's RegistrationICP (tests/icp_oracle.py).  The pose bar is the project's: 1e-3 m / 1e-3 deg
(DESIGN section 2)."""
import functools

import numpy as np
import pytest
import torch

from tests import icp_oracle as O

pytestmark = pytest.mark.gpu

BAR_M, BAR_DEG = 1e-3, 1e-3


def _run(dev, src, tgt, init=None, max_dist=0.2, max_iteration=30, rel_fitness=1e-6, rel_rmse=1e-6):
    from apr_amd import ops
    s, t = torch.from_numpy(np.ascontiguousarray(src)).to(dev), torch.from_numpy(np.ascontiguousarray(tgt)).to(dev)
    init = np.eye(4) if init is None else init
    rec, corr = ops.icp_batch(s, [0, len(s)], t, [0, len(t)], np.asarray(init, dtype=np.float64).reshape(1, 4, 4), max_dist,
                              max_iteration, rel_fitness, rel_rmse, want_corr=True)
    r = rec.cpu().numpy()[0]
    return dict(T=r[:16].reshape(4, 4), fitness=r[16], rmse=r[17], n_corr=int(r[18]), iterations=int(r[19]),
                corr=corr.cpu().numpy().astype(np.int64), rec=rec, corr_dev=corr)


@functools.lru_cache(maxsize=None)
def _case(trans_m, rot_deg):
    from scipy.spatial import cKDTree
    src, tgt = O.icp_case(trans_m, rot_deg)
    return src, tgt, cKDTree(tgt.astype(np.float64))


def test_ops_reject_cpu_tensors():
    from apr_amd import _lib, ops
    x = torch.zeros((4, 3))
    with pytest.raises(_lib.AprHipError):
        ops.icp_batch(x, [0, 4], x, [0, 4], np.eye(4).reshape(1, 4, 4), 0.2)


def test_evaluation_only_matches_the_oracle_exactly(dev):
    """max_iteration = 0: the association itself.  Planted: a tie between two targets (smallest row wins), a duplicate
    target, a target whose float32 d^2 equals max_dist^2 exactly (no correspondence), sources beyond reach, and a bulk of
    2000 noisy pairs under a non-trivial init."""
    rng = np.random.default_rng(1)
    bulk_t = rng.uniform(-20.0, 20.0, size=(2000, 3)).astype(np.float32)
    special_t = np.array([[100.25, 0, 0], [99.75, 0, 0],         # equidistant from (100, 0, 0)
                          [110.0, 0.25, 0], [110.0, 0.25, 0],     # duplicate
                          [120.5, 0, 0],                          # exactly max_dist = 0.5 from (120, 0, 0)
                          [130.0, 0, 0.4375]], dtype=np.float32)
    tgt = np.concatenate([bulk_t[:1000], special_t, bulk_t[1000:]])
    init = O.perturbation(0.1, 2.0, seed=2)
    inv = np.linalg.inv(init)
    special_s = np.array([[100.0, 0, 0], [110.0, 0, 0], [120.0, 0, 0], [130.0, 0, 0], [200.0, 0, 0]], dtype=np.float32)
    bulk_s = (bulk_t + rng.normal(0.0, 0.2, size=bulk_t.shape)).astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]
    src = np.concatenate([special_s, bulk_s.astype(np.float32)])
    for T0, max_dist in ((np.eye(4), 0.5), (init, 0.5), (init, 0.2)):
        want = O.icp(src, tgt, T0, max_dist, 0, fp32_round=True)
        got = _run(dev, src, tgt, T0, max_dist, 0)
        print(f"max_dist {max_dist}: {got['n_corr']} correspondences, rmse {got['rmse']:.9f} / {want['rmse']:.9f}")
        assert np.array_equal(got["corr"], want["corr"])
        assert got["n_corr"] == want["n_corr"] and got["fitness"] == want["fitness"] and got["iterations"] == 0
        assert abs(got["rmse"] - want["rmse"]) <= 1e-6 * want["rmse"]
        assert np.array_equal(got["T"], T0)
        if T0[0, 3] == 0.0:
            assert got["corr"][:5].tolist() == [1000, 1002, -1, 1005, -1]     # tie -> row 1000, d^2 == r^2 -> none
    assert want["n_corr"] > 100


def test_fixed_iteration_count_matches_the_oracle(dev):
    """30 iterations with both thresholds 0 on the full-size frames (6 m apart, 5 cm reduction, 0.15 m / 0.5 deg off).
    Measured on the CPU between the oracle's float32-rounded and all-float64 variants on this very input after 30
    iterations: the same correspondence count (66904 of 94595 in both), no row with a different partner, poses 2.0e-9 m
    apart.  The kernel follows the float32-rounded variant's arithmetic and differs from it only in the last bits of T
    (Horn against SVD, summation order), far less than the variants differ from each other; the cap is 2 rows all the
    same -- the largest difference the two variants showed on any input tried (0.3 m / 1 deg), and a row at a rounding
    knife-edge is 1e-5 of the count."""
    src, tgt, tree = _case(0.15, 0.5)
    want = O.icp(src, tgt, None, 0.2, 30, 0.0, 0.0, fp32_round=True, tree=tree)
    got = _run(dev, src, tgt, None, 0.2, 30, 0.0, 0.0)
    rte, rre = O.pose_error(got["T"], want["T"])
    rows = int((got["corr"] != want["corr"]).sum())
    print(f"pose difference {rte:.2e} m / {rre:.2e} deg, correspondences {got['n_corr']} / {want['n_corr']}, "
          f"{rows} rows differ, rmse {got['rmse']:.9f} / {want['rmse']:.9f}")
    assert got["iterations"] == want["iterations"] == 30
    assert rte < BAR_M and rre < BAR_DEG
    assert abs(got["n_corr"] - want["n_corr"]) <= 2 and rows <= 2


@pytest.mark.parametrize("trans_m,rot_deg", [(0.05, 0.2), (0.15, 0.5)])
def test_converged_run_stops_where_the_oracle_stops(dev, trans_m, rot_deg):
    """The reference's criteria (1e-6 / 1e-6 / 200).  open3d's rule stops only when the correspondence count repeats
    exactly (one point is 1e-5 of fitness), so the iteration count is a sharp test of the whole loop; the oracle's two
    arithmetic variants agree on it for these inputs (tests/test_icp_cpu.py)."""
    src, tgt, tree = _case(trans_m, rot_deg)
    want = O.icp(src, tgt, None, 0.2, 200, fp32_round=True, tree=tree)
    got = _run(dev, src, tgt, None, 0.2, 200)
    rte, rre = O.pose_error(got["T"], want["T"])
    print(f"iterations {got['iterations']} / {want['iterations']}, pose difference {rte:.2e} m / {rre:.2e} deg, "
          f"fitness {got['fitness']:.6f} / {want['fitness']:.6f}, rmse {got['rmse']:.6f} / {want['rmse']:.6f}")
    assert got["iterations"] == want["iterations"]
    assert rte < BAR_M and rre < BAR_DEG


def test_same_bits_run_to_run_and_alone_against_batched(dev):
    from apr_amd import ops
    src, tgt, _ = _case(0.15, 0.5)
    t = torch.from_numpy(tgt).to(dev)
    srcs = [torch.from_numpy(O.apply_transform(src, O.perturbation(0.02 * i, 0.05 * i, seed=40 + i))).to(dev)
            for i in range(10)]
    off = np.concatenate([[0], np.cumsum([len(s) for s in srcs])])
    init = np.tile(np.eye(4), (10, 1, 1))
    args = (torch.cat(srcs, 0), off, t, [0, len(t)], init, 0.2, 200)
    rec_a, corr_a = ops.icp_batch(*args, tgt_of_problem=[0] * 10, want_corr=True)
    rec_b, corr_b = ops.icp_batch(*args, tgt_of_problem=[0] * 10, want_corr=True)
    assert torch.equal(rec_a, rec_b) and torch.equal(corr_a, corr_b)
    its = rec_a[:, ops.ICP_ITERATIONS].cpu().numpy()
    print("iterations per problem:", its.astype(int).tolist())
    assert len(set(its.tolist())) > 1                            # the problems stop at different rounds
    for i in (0, 3, 9):
        rec_1, corr_1 = ops.icp_batch(srcs[i], [0, len(srcs[i])], t, [0, len(t)], init[:1], 0.2, 200, want_corr=True)
        assert torch.equal(rec_1[0], rec_a[i])
        assert torch.equal(corr_1, corr_a[off[i]:off[i + 1]])


def test_degenerate_inputs_stay_finite(dev):
    rng = np.random.default_rng(3)
    tgt = rng.uniform(-5.0, 5.0, size=(500, 3)).astype(np.float32)
    init = O.perturbation(0.3, 3.0, seed=4)
    # nothing within reach: init comes back, fitness 0, rmse 0
    far = _run(dev, tgt + np.float32(100.0), tgt, init, 0.2, 50)
    assert np.array_equal(far["T"], init) and far["fitness"] == 0.0 and far["rmse"] == 0.0 and far["n_corr"] == 0
    assert far["iterations"] == 1 and (far["corr"] == -1).all() and np.isfinite(far["rec"].cpu().numpy()).all()
    # two correspondences only; a collinear and a planar correspondence set
    two = np.concatenate([tgt[:2] + np.float32(0.01), tgt[2:6] + np.float32(50.0)])
    line_t = np.stack([np.linspace(-5, 5, 200), np.zeros(200), np.zeros(200)], 1).astype(np.float32)
    plane_t = np.concatenate([rng.uniform(-5, 5, size=(400, 2)), np.zeros((400, 1))], 1).astype(np.float32)
    for name, s, t in (("two", two, tgt), ("collinear", line_t + np.float32([0.01, 0.02, 0.0]), line_t),
                       ("planar", plane_t + np.float32([0.01, 0.0, 0.02]), plane_t),
                       ("one point", tgt[:1] + np.float32(0.01), tgt[:1])):
        r = _run(dev, s, t, None, 0.2, 50)
        rec = r["rec"].cpu().numpy()
        print(name, "->", r["n_corr"], "correspondences,", r["iterations"], "iterations, rmse", r["rmse"])
        assert np.isfinite(rec).all()
        R = r["T"][:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and np.linalg.det(R) > 0.999
        assert r["n_corr"] >= 1 and 0 < r["iterations"] <= 50


def _parent_aggregate_frames(key_xyz, complement_xyz, complement_poses, voxel_size):
    """aggregate_frames as it stood before the `refine` keyword."""
    from apr_amd import ops
    from apr_amd.fcgf.lib import apg
    moved = [apg.apply_transform(x, M) for x, M in zip(complement_xyz, complement_poses)]
    nghb = apg.crop_to_radius(key_xyz, torch.cat(moved, 0))
    m = ops.build_map(ops.voxelize(nghb, voxel_size, 0), want_first=True)
    ops.finalize_maps([m])
    return nghb, m.first


def _voxel_set(nghb, sel, n, voxel_size):
    pts = nghb[sel[:n]].cpu().numpy() if n is not None else nghb.cpu().numpy()
    c = np.floor(pts / np.float32(voxel_size)).astype(np.int64)
    return set(map(tuple, np.unique(c, axis=0)))


def test_aggregate_frames_from_raw_odometry(dev):
    """End to end: four complement frames 3 and 6 m either side of the key frame, their planted poses perturbed by 0.15 m /
    0.5 deg, refined inside aggregate_frames.  The voxel-set bound: poses at the bar move a point by at most 1e-3 m +
    80 m * 1e-3 deg = 2.4e-3 m, which takes it across a face of its 0.3 m voxel with probability <= 3 * 2.4e-3 / 0.3 =
    2.4 %; every such point can empty one voxel and open another, so at most 5 % of the voxels may differ."""
    from scipy.spatial import cKDTree
    from apr_amd.fcgf.lib import apg
    frames, planted = O.synthetic_frames([0.0, -6.0, -3.0, 3.0, 6.0])
    key, cmpls, planted = frames[0], frames[1:], planted[1:]
    Ms = [O.perturbation(0.15, 0.5, seed=20 + i) @ T for i, T in enumerate(planted)]
    key_d = torch.from_numpy(key).to(dev)
    cmpl_d = [torch.from_numpy(x).to(dev) for x in cmpls]

    poses, results = apg.refine_complement_poses(key_d, cmpl_d, Ms, return_results=True)
    # the oracle solves the same ICP inputs: the reduction picks the oracle's rows exactly, the float32 transform differs
    # from numpy's in the last bit (contraction), which the stopping rule could turn into another iteration count
    sels = apg.voxel_first_rows([key_d] + cmpl_d, 0.05)
    for x, sel in zip([key] + cmpls, sels):
        assert np.array_equal(sel.cpu().numpy(), O.voxel_first_rows(x, 0.05))
    curr = key[sels[0].cpu().numpy()]
    tree = cKDTree(curr.astype(np.float64))
    want = []
    for x, x_d, sel, M in zip(cmpls, cmpl_d, sels[1:], Ms):
        moved = apg.apply_transform(x_d[sel].contiguous(), M).cpu().numpy()
        assert np.abs(moved - O.apply_transform(x[sel.cpu().numpy()], M)).max() < 2e-5
        reg = O.icp(moved, curr, None, 0.2, 200, fp32_round=True, tree=tree)
        want.append((reg["T"] @ M, reg))
    for i, (P, (W, reg), res, T) in enumerate(zip(poses, want, results, planted)):
        d = O.pose_error(P, W)
        mine, theirs = O.pose_error(P, T), O.pose_error(W, T)
        print(f"frame {i}: vs oracle {d[0]:.2e} m / {d[1]:.2e} deg, iterations {res.iterations} / {reg['iterations']}, "
              f"residual to planted {mine[0]:.4f} m / {mine[1]:.4f} deg (oracle {theirs[0]:.4f} / {theirs[1]:.4f})")
        assert d[0] < BAR_M and d[1] < BAR_DEG
        assert mine[0] <= 2 * theirs[0] and mine[1] <= 2 * theirs[1]
        assert mine[0] < 0.15 and mine[1] < 0.5                  # and it did refine

    one = apg.refine_pose(key_d, cmpl_d[2], Ms[2])
    assert np.array_equal(one, poses[2])                          # the batch is the single call, bit for bit

    nghb, sel = apg.aggregate_frames(key_d, cmpl_d, Ms, 0.3, refine=True)
    nghb_o, sel_o = apg.aggregate_frames(key_d, cmpl_d, [W for W, _ in want], 0.3)
    a, b = _voxel_set(nghb, None, None, 0.3), _voxel_set(nghb_o, None, None, 0.3)
    print(f"APG voxels {len(a)} / {len(b)}, symmetric difference {len(a ^ b)}")
    assert len(a ^ b) <= 0.05 * len(b)

    # refine=False (the default) is the parent's function, bit for bit
    n0, s0 = apg.aggregate_frames(key_d, cmpl_d, planted, 0.3)
    n1, s1 = _parent_aggregate_frames(key_d, cmpl_d, planted, 0.3)
    n2, s2 = apg.aggregate_frames(key_d, cmpl_d, planted, 0.3, refine=False)
    assert torch.equal(n0, n1) and torch.equal(n0, n2)
    k = len(_voxel_set(n0, None, None, 0.3))
    assert torch.equal(s0[:k], s1[:k]) and torch.equal(s0[:k], s2[:k])


def test_predator_pair_refinement_is_the_same_code(dev):
    from apr_amd.fcgf.lib import apg
    from apr_amd.predator.datasets import kitti
    frames, planted = O.synthetic_frames([0.0, 3.0])
    M = O.perturbation(0.05, 0.2, seed=30) @ planted[1]
    a, b = torch.from_numpy(frames[0]).to(dev), torch.from_numpy(frames[1]).to(dev)
    P = kitti.refine_pair_pose(b, a, M, icp_voxel_size=0.05)
    assert np.array_equal(P, apg.refine_pose(a, b, M))
    rte, rre = O.pose_error(P, planted[1])
    print(f"residual to planted {rte:.4f} m / {rre:.4f} deg")
    assert rte < 0.05 and rre < 0.2


def test_registration_icp_mirror(dev):
    from apr_amd import ops
    from apr_amd.fcgf import registration as reg
    src, tgt, _ = _case(0.05, 0.2)
    src, tgt = src[::4].copy(), tgt
    init = O.perturbation(0.01, 0.05, seed=6)
    crit = reg.ICPConvergenceCriteria(max_iteration=20)
    assert (crit.relative_fitness, crit.relative_rmse) == (1e-6, 1e-6) and reg.ICPConvergenceCriteria().max_iteration == 30
    r = reg.registration_icp(src, tgt, 0.2, init, reg.TransformationEstimationPointToPoint(), crit)
    raw = _run(dev, src, tgt, init, 0.2, 20)
    assert isinstance(r.transformation, np.ndarray) and r.transformation.dtype == np.float64
    assert r.transformation.shape == (4, 4) and np.array_equal(r.transformation, raw["T"])
    assert isinstance(r.fitness, float) and isinstance(r.inlier_rmse, float)
    assert r.fitness == raw["fitness"] and r.inlier_rmse == raw["rmse"] and r.iterations == raw["iterations"]
    cs = r.correspondence_set
    assert cs.dtype == np.int64 and cs.shape == (raw["n_corr"], 2)
    assert np.array_equal(cs[:, 1], raw["corr"][cs[:, 0]]) and (raw["corr"] >= 0).sum() == len(cs)
    d = reg.registration_icp(torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), 0.2)   # defaults: eye(4), 30
    assert d.iterations <= 30 and d.fitness > 0.5

    class TransformationEstimationPointToPlane:
        pass
    with pytest.raises(NotImplementedError):
        reg.registration_icp(src, tgt, 0.2, init, TransformationEstimationPointToPlane())
    assert ops.ICP_RECORD_DOUBLES == 20
