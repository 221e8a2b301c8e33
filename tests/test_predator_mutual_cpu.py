"""CPU-side checks of the mutual-matching work: the pair-list RANSAC oracle against a brute-force restatement, the conditions
the fixture tests/golden/predator_mutual_ref.npz promises about its own inputs, and the C-ABI boundary of the new entries."""
import os

import numpy as np
import pytest
import torch

from tests import pairs_ransac_oracle as PO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predator_mutual_ref.npz")
CASES = ["odd", "one", "row", "col", "ties", "pose"]


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}


def _case(gold, name):
    return {k.split(".", 1)[1]: v for k, v in gold.items() if k.startswith(name + ".")}


def _tiny_pair(seed, n=40, m=36, n_true=14):
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(-4, 4, (n, 3)).astype(np.float32)
    x1 = rng.uniform(-4, 4, (m, 3)).astype(np.float32)
    a = np.deg2rad(17.0)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    t = np.array([0.4, -0.3, 0.2])
    i, j = rng.choice(n, n_true, replace=False), rng.choice(m, n_true, replace=False)
    x1[j] = (x0[i].astype(np.float64) @ R.T + t + rng.normal(0, 0.01, (n_true, 3))).astype(np.float32)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    pairs = np.stack([i, j], 1)
    wrong = np.stack([rng.choice(n, 6), rng.choice(m, 6)], 1)
    return x0, x1, np.concatenate([pairs[:9], wrong], 0), T


def test_pair_list_oracle_matches_brute_force():
    x0, x1, pairs, T_gt = _tiny_pair(0)
    T_k, info_k = PO.ransac_pairs_geometric(x0, x1, pairs, 0.08, 50000, 120, seed=3)
    T_b, info_b = PO.ransac_pairs_geometric(x0, x1, pairs, 0.08, 50000, 120, seed=3, nn="brute")
    assert info_k["n_valid"] == info_b["n_valid"] == 120 and len(info_k["counts"]) == 120
    assert np.array_equal(info_k["counts"], info_b["counts"]) and np.allclose(info_k["rmses"], info_b["rmses"], rtol=0, atol=1e-12)
    assert info_k["best_iteration"] == info_b["best_iteration"] >= 0 and np.array_equal(T_k, T_b)
    # the best hypothesis is the first one at the top count with the lowest rmse, and it finds the planted motion
    top = info_k["counts"].max()
    cand = np.nonzero(info_k["counts"] == top)[0]
    assert info_k["best_iteration"] == cand[np.argmin(info_k["rmses"][cand])] and info_k["inliers"] == top >= 9
    assert np.abs(T_k - T_gt).max() < 0.05
    # samples come from the kernels' counter stream and stay inside the list
    assert info_k["samples"].shape == (120, 4) and info_k["samples"].min() >= 0 and info_k["samples"].max() < len(pairs)
    # min(max_iter, max_validation) iterations either way round
    assert PO.ransac_pairs_geometric(x0, x1, pairs, 0.08, 50, 1000, seed=3)[1]["n_valid"] == 50


def test_pair_list_oracle_defaults_without_enough_pairs_or_inliers():
    x0, x1, pairs, _ = _tiny_pair(1)
    for k in (0, 3):
        T, info = PO.ransac_pairs_geometric(x0, x1, pairs[:k], 0.08, seed=0)
        assert np.array_equal(T, np.eye(4)) and info["inliers"] == 0 and info["best_iteration"] == -1 and info["fitness"] == 0.0
    # no hypothesis has an inlier: the default result stays (open3d compares fitness strictly)
    far = x1 + np.float32(100.0)
    T, info = PO.ransac_pairs_geometric(x0 * np.float32(1e-3), far * np.float32(50.0), pairs, 1e-6, 50000, 20, seed=0)
    assert info["counts"].max() == 0 and np.array_equal(T, np.eye(4)) and info["best_iteration"] == -1


@pytest.mark.parametrize("name", CASES)
def test_fixture_keeps_its_own_conditions(gold, name):
    c = _case(gold, name)
    thr = float(gold["threshold"])
    sf, tf = c["src_feat"], c["tgt_feat"]
    assert sf.dtype == np.float32 and sf.shape[1] == 32 and tf.shape[1] == 32
    assert np.abs(np.linalg.norm(sf.astype(np.float64), axis=1) - 1).max() < 1e-6
    s = sf.astype(np.float64) @ tf.astype(np.float64).T

    def gap(scores, other):
        arg = scores.argmax(1)
        same = (other[None, :, :] == other[arg][:, None, :]).all(2)
        return (scores.max(1) - np.where(same, -np.inf, scores).max(1)).min()

    assert gap(s, tf) >= 1e-4 and gap(s.T, sf) >= 1e-4
    # the mask is the float64 arg-max pair list, ties to the lowest index
    ra, ca = s.argmax(1), s.argmax(0)
    keep = np.nonzero(ca[ra] == np.arange(len(sf)))[0]
    assert np.array_equal(c["row_sel"], keep) and np.array_equal(c["col_sel"], ra[keep])
    assert c["mask"].dtype == np.bool_ and np.array_equal(np.stack(np.nonzero(c["mask"])), np.stack([keep, ra[keep]]))
    p = c["src_pcd"].astype(np.float64) @ c["rot"].astype(np.float64).T + c["trans"][:, 0].astype(np.float64)
    d_wo = np.linalg.norm(p - c["tgt_pcd"].astype(np.float64)[ra], axis=1)
    d_w = np.linalg.norm(p[keep] - c["tgt_pcd"].astype(np.float64)[ra[keep]], axis=1)
    assert np.abs(d_wo - thr).min() >= 1e-5 and np.abs(d_w - thr).min() >= 1e-5
    assert np.abs(d_wo - c["dist_wo"]).max() < 1e-5 and np.abs(d_w - c["dist_w"]).max() < 1e-5
    assert abs(float(c["ratio_wo"]) - (d_wo < thr).mean()) < 1e-6 and abs(float(c["ratio_w"]) - (d_w < thr).mean()) < 1e-6


def test_fixture_ties_decide_and_ratios_are_informative(gold):
    c = _case(gold, "ties")
    dups = c["dups"]
    assert (dups[:, 0] == 1).sum() == 3 and (dups[:, 0] == 0).sum() == 3
    s = c["src_feat"].astype(np.float64) @ c["tgt_feat"].astype(np.float64).T
    for axis, a, b in dups:
        lo, hi = min(a, b), max(a, b)
        if axis == 1:                  # two equal target rows: some source row has both as its maximum, the lower one wins
            rows = np.nonzero(s.max(1) == s[:, lo])[0]
            assert np.array_equal(c["tgt_feat"][a], c["tgt_feat"][b]) and len(rows) >= 1
            assert not c["mask"][:, hi][rows].any()
        else:
            cols = np.nonzero(s.max(0) == s[lo])[0]
            assert np.array_equal(c["src_feat"][a], c["src_feat"][b]) and len(cols) >= 1
            assert not c["mask"][hi][cols].any()
    for name in ("odd", "ties", "pose"):
        cc = _case(gold, name)
        assert 0.15 < float(cc["ratio_wo"]) < 0.5 and 0.3 < float(cc["ratio_w"]) < 0.8
    assert os.path.getsize(GOLDEN) < 400 * 1024


def test_new_entries_check_their_arguments_without_a_gpu(lib):
    assert lib.apr_mutual_select(None, None, 10, None, None, 10, None, None, None) == -1
    assert b"apr_mutual_select" in lib.apr_last_error()
    assert lib.apr_inlier_ratio(None, 1 << 24, None, 10, None, None, None, None, None, 10, 0.1, None, None, None, None) == -1
    assert b"2^24" in lib.apr_last_error()
    assert lib.apr_dense_argmax(None, 0, 5, None, None, None) == -1
    assert lib.apr_ransac_pairs_geometric_scratch_bytes(400, 380, 200, 50000, 1000) > 1000 * 120
    assert lib.apr_ransac_pairs_geometric_scratch_bytes(400, 380, 200, 1 << 20, 1 << 20) == 0       # more hypotheses than the list holds
    import ctypes as C
    res = (C.c_double * 20)()
    assert lib.apr_ransac_pose_pairs_geometric(None, 400, None, 380, None, 200, 0.1, 1 << 20, 1 << 20, 0, None, 0, res, None) == -1
    assert b"min(max_iter, max_validation)" in lib.apr_last_error()


def test_mutual_entry_points_reach_the_library_and_refuse_cpu_tensors():
    from apr_amd import ops
    from apr_amd._lib import AprHipError
    from apr_amd.predator.lib import benchmark_utils as BU
    f = torch.zeros(4, 32)
    i = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(AprHipError):
        ops.score_argmax(f, f)
    with pytest.raises(AprHipError):
        ops.mutual_select(i, i)
    with pytest.raises(AprHipError):
        ops.dense_argmax(torch.zeros(4, 4))
    with pytest.raises(AprHipError):
        ops.inlier_ratio(torch.zeros(4, 3), torch.zeros(4, 3), torch.eye(3), torch.zeros(3, 1), i, torch.zeros((4, 2), dtype=torch.int32),
                         torch.zeros(1, dtype=torch.int32), 0.1)
    with pytest.raises(AprHipError):
        ops.ransac_pose_pairs_geometric(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros((4, 2), dtype=torch.int32), 4, 0.1)
    if not torch.cuda.is_available():
        # mutual=True no longer stops at NotImplementedError: it reaches the library loader, which refuses host data
        z3, z32 = torch.zeros(4, 3), torch.zeros(4, 32)
        with pytest.raises(AprHipError):
            BU.ransac_pose_estimation(z3, z3, z32, z32, mutual=True)
        with pytest.raises(AprHipError):
            BU.get_inlier_ratio(z3, z3, z32, z32, torch.eye(3), torch.zeros(3, 1))
        with pytest.raises(AprHipError):
            BU.mutual_pairs(z32.numpy(), z32.numpy())
        with pytest.raises(AprHipError):
            BU.mutual_selection(np.zeros((1, 4, 4), np.float32))
