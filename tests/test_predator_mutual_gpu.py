"""Mutual-check matching, inlier ratios and the pair-list RANSAC of the Predator tester against the reference's own
functions (tests/golden/predator_mutual_ref.npz, made by make_predator_mutual_ref_golden.py) and the float64 oracle of
tests/pairs_ransac_oracle.py."""
import os

import numpy as np
import pytest
import torch

from apr_amd import ops
from apr_amd.fcgf import registration
from apr_amd.predator.lib import benchmark_utils as BU
from tests import pairs_ransac_oracle as PO

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predator_mutual_ref.npz")
CASES = ["odd", "one", "row", "col", "ties", "pose"]
POSE_DIST = 0.15          # max_correspondence_distance of the RANSAC cases: 7 sigma of the planted 0.02 m noise


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}


def _case(gold, name):
    return {k.split(".", 1)[1]: v for k, v in gold.items() if k.startswith(name + ".")}


def _scores(src_feat, tgt_feat):
    """src_feat @ tgt_feat.T in float32, the 32 products of every entry added in one fixed order: duplicated rows give
    bitwise equal entries whatever BLAS is installed."""
    s = np.zeros((len(src_feat), len(tgt_feat)), np.float32)
    for k in range(src_feat.shape[1]):
        s += src_feat[:, k, None] * tgt_feat[None, :, k]
    return s


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


@pytest.mark.parametrize("name", CASES)
def test_mutual_selection_and_pairs_equal_the_reference(dev, gold, name):
    c = _case(gold, name)
    row_sel, col_sel = BU.mutual_pairs(c["src_feat"], c["tgt_feat"])
    assert row_sel.dtype == np.int64 and col_sel.dtype == np.int64
    assert np.array_equal(row_sel, c["row_sel"]) and np.array_equal(col_sel, c["col_sel"])
    scores = _scores(c["src_feat"], c["tgt_feat"])
    for arg in (scores, scores[None], torch.from_numpy(scores)):
        mask = BU.mutual_selection(arg)
        assert mask.dtype == np.bool_ and mask.shape == (1,) + scores.shape
        assert np.array_equal(mask[0], c["mask"])


@pytest.mark.parametrize("name", CASES)
def test_get_inlier_ratio_matches_the_reference(dev, gold, name):
    c = _case(gold, name)
    thr = float(gold["threshold"])
    res = BU.get_inlier_ratio(c["src_pcd"], c["tgt_pcd"], c["src_feat"], c["tgt_feat"], c["rot"], c["trans"], thr)
    assert set(res) == {"w", "wo"}
    for leg, dist, ratio in (("wo", c["dist_wo"], c["ratio_wo"]), ("w", c["dist_w"], c["ratio_w"])):
        assert set(res[leg]) == {"distance", "inlier_ratio"}
        d, r = res[leg]["distance"], res[leg]["inlier_ratio"]
        assert isinstance(d, np.ndarray) and d.dtype == np.float32 and d.shape == dist.shape
        assert torch.is_tensor(r) and r.dtype == torch.float32 and r.dim() == 0 and r.device.type == "cpu"
        err = float(np.abs(d.astype(np.float64) - dist.astype(np.float64)).max())
        n_in, n_ref = int((d < np.float32(thr)).sum()), int((dist < np.float32(thr)).sum())
        print(f"{name}/{leg}: max |distance - ref| {err:.3e}, inliers {n_in} vs {n_ref}, ratio {float(r):.7f} vs {float(ratio):.7f}")
        assert err <= 1e-5
        assert n_in == n_ref
        assert abs(float(r) - float(ratio)) <= 1e-6
        assert abs(float(r) - n_in / len(d)) <= 1e-6           # the ratio is the count over the length


def _pose_args(gold):
    c = _case(gold, "pose")
    T_gt = np.eye(4)
    T_gt[:3, :3], T_gt[:3, 3] = c["rot"].astype(np.float64), c["trans"][:, 0].astype(np.float64)
    return c, T_gt


def test_ransac_mutual_matches_the_oracle_hypothesis_for_hypothesis(dev, gold):
    c, T_gt = _pose_args(gold)
    assert len(c["src_pcd"]) == 400 and abs(len(c["planted"]) / 400 - 0.3) < 0.05
    T, row_sel, col_sel, info = BU.ransac_pose_estimation(c["src_pcd"], c["tgt_pcd"], c["src_feat"], c["tgt_feat"], mutual=True,
                                                          distance_threshold=POSE_DIST, seed=7, return_info=True)
    assert np.array_equal(row_sel, c["row_sel"]) and np.array_equal(col_sel, c["col_sel"])
    out3 = BU.ransac_pose_estimation(c["src_pcd"], c["tgt_pcd"], c["src_feat"], c["tgt_feat"], mutual=True,
                                     distance_threshold=POSE_DIST, seed=7)
    assert len(out3) == 3 and np.array_equal(out3[0], T) and np.array_equal(out3[1], row_sel)
    pairs = np.stack([c["row_sel"], c["col_sel"]], 1)
    T_o, info_o = PO.ransac_pairs_geometric(c["src_pcd"], c["tgt_pcd"], pairs, POSE_DIST, 50000, 1000, seed=7)
    print("device", info, "oracle", {k: v for k, v in info_o.items() if np.ndim(v) == 0})
    assert info["n_valid"] == info_o["n_valid"] == 1000 and info["n_pairs"] == len(pairs)
    assert info["best_iteration"] == info_o["best_iteration"] and info["inliers"] == info_o["inliers"] > 0
    rte, rre = registration.rte_rre(T, T_o)
    assert rte < 1e-3 and rre < 1e-3
    rte, rre = registration.rte_rre(T, T_gt)
    print(f"to the planted motion: {rte:.4f} m, {rre:.4f} deg")
    assert rte < 0.1 and rre < 0.5
    # every hypothesis, not only the best: the same stream with fewer iterations ends at the oracle's running best
    for n_it in (1, 2, 17, 300):
        cnt = info_o["counts"][:n_it]
        top = cnt.max()
        if top == 0:
            want = -1
        else:
            cand = np.nonzero(cnt == top)[0]
            want = int(cand[np.argmin(info_o["rmses"][cand])])
        _, inf = ops.ransac_pose_pairs_geometric(_t(c["src_pcd"], dev), _t(c["tgt_pcd"], dev), _t(pairs, dev, torch.int32),
                                                 len(pairs), POSE_DIST, 50000, n_it, seed=7)
        assert inf["best_iteration"] == want and inf["inliers"] == int(top) and inf["n_valid"] == n_it


def test_ransac_pair_list_of_four_and_of_three(dev, gold):
    c, T_gt = _pose_args(gold)
    x0, x1 = _t(c["src_pcd"], dev), _t(c["tgt_pcd"], dev)
    four = c["planted"][[0, 40, 80, 119]]
    T, info = ops.ransac_pose_pairs_geometric(x0, x1, _t(four, dev, torch.int32), 4, POSE_DIST, 50000, 1000, seed=1)
    T_o, info_o = PO.ransac_pairs_geometric(c["src_pcd"], c["tgt_pcd"], four, POSE_DIST, 50000, 1000, seed=1)
    print("device", info, "oracle", {k: v for k, v in info_o.items() if np.ndim(v) == 0})
    assert info["inliers"] == info_o["inliers"] > 4 and info["n_valid"] == 1000
    # 4^4 = 256 possible samples in 1000 draws: the draws that hold the same entries as often pose the same least-squares
    # problem and tie up to summation order, so the winner is pinned as a sample, not as an iteration number
    s = info_o["samples"]
    assert sorted(s[info["best_iteration"]]) == sorted(s[info_o["best_iteration"]])
    rte, rre = registration.rte_rre(T, T_o)
    assert rte < 1e-3 and rre < 1e-3
    rte, rre = registration.rte_rre(T, T_gt)
    assert rte < 0.1 and rre < 0.5
    # the buffer may be longer than the list: rows past n_pairs are not read (they point outside both clouds here)
    longer = np.concatenate([four, np.full((5, 2), 1 << 20)], 0)
    T2, info2 = ops.ransac_pose_pairs_geometric(x0, x1, _t(longer, dev, torch.int32), 4, POSE_DIST, 50000, 1000, seed=1)
    assert np.array_equal(T2, T) and info2 == info
    T3, info3 = ops.ransac_pose_pairs_geometric(x0, x1, _t(four, dev, torch.int32), 3, POSE_DIST, 50000, 1000, seed=1)
    assert np.array_equal(T3, np.eye(4)) and info3["inliers"] == 0 and info3["fitness"] == 0.0
    assert info3["best_iteration"] == -1 and info3["n_valid"] == 0
    T3o, info3o = PO.ransac_pairs_geometric(c["src_pcd"], c["tgt_pcd"], four[:3], POSE_DIST, seed=1)
    assert np.array_equal(T3o, np.eye(4)) and info3o["inliers"] == 0


def test_two_calls_give_equal_outputs(dev, gold):
    c = _case(gold, "odd")
    sf, tf = _t(c["src_feat"], dev), _t(c["tgt_feat"], dev)
    x0, x1 = _t(c["src_pcd"], dev), _t(c["tgt_pcd"], dev)
    rot, trans = _t(c["rot"], dev), _t(c["trans"], dev)
    runs = []
    for _ in range(2):
        row_arg, col_arg = ops.score_argmax(sf, tf)
        pairs, count = ops.mutual_select(row_arg, col_arg)
        n = int(count.item())
        dist_wo, dist_w, out = ops.inlier_ratio(x0, x1, rot, trans, row_arg, pairs, count, 0.1)
        T, info = ops.ransac_pose_pairs_geometric(x0, x1, pairs, n, 0.1, 50000, 200, seed=4)
        runs.append((pairs[:n].clone(), count.clone(), dist_wo, dist_w[:n].clone(), out, torch.from_numpy(T),
                     torch.tensor([info["inliers"], info["best_iteration"], info["n_valid"]])))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_mutual_list_from_sub_lists_matches_brute_force(dev, gold):
    """apr_gathered_argmax on index sub-lists whose device-side lengths are shorter than the buffers (130 of 300, 1 of 257, and
    the other way round): the pair list holds list POSITIONS, only `count` rows are written, nothing past the lengths is read."""
    c = _case(gold, "odd")
    rng = np.random.default_rng(5)
    sf, tf = _t(c["src_feat"], dev), _t(c["tgt_feat"], dev)
    for na, nb in ((130, 1), (1, 100), (130, 100), (300, 257)):
        a_idx = rng.permutation(300).astype(np.int32)
        b_idx = rng.permutation(257).astype(np.int32)
        a_dev, b_dev = a_idx.copy(), b_idx.copy()
        a_dev[na:] = 0            # past the lengths: a valid row, so that a kernel that did look there would not fault but
        b_dev[nb:] = 0            # would see copies of row 0 compete for the arg-max
        n = _t(np.array([na, nb], np.int32), dev)
        row_arg, col_arg = ops.gathered_argmax(sf, _t(a_dev, dev), n[0:1], tf, _t(b_dev, dev), n[1:2])
        row_arg[na:] = -7         # entries past the lengths hold nothing the kernel may rely on
        col_arg[nb:] = 1 << 29
        pairs, count = ops.mutual_select(row_arg, col_arg, n[0:1], n[1:2])
        assert pairs.shape == (257, 2) and pairs.dtype == torch.int32
        s = c["src_feat"][a_idx[:na]].astype(np.float64) @ c["tgt_feat"][b_idx[:nb]].astype(np.float64).T
        ra, ca = s.argmax(1), s.argmax(0)
        keep = np.nonzero(ca[ra] == np.arange(na))[0]
        want = np.stack([keep, ra[keep]], 1)
        k = int(count.item())
        assert k == len(want) >= 1 and np.array_equal(pairs[:k].cpu().numpy(), want)
        assert not pairs[k:].any()            # untouched (the wrapper hands out zeros)


def test_mutual_false_path_is_untouched(dev):
    """The mutual=False call of tests/test_predator_pose_mining_gpu.py, its own arguments and seeds: bit for bit the direct
    call of the geometric RANSAC entry that path has always made."""
    from oracle import match_pose_oracle as MO  # noqa: F401
    from tests.test_match_pose_gpu import _synthetic_pair
    for seed, inlier in ((0, 0.5), (3, 0.3)):
        xyz0, xyz1, F0, F1, _ = _synthetic_pair(seed, n=2500, inlier=inlier)
        T, info = BU.ransac_pose_estimation(xyz0, xyz1, F0, F1, mutual=False, distance_threshold=0.3, ransac_n=4,
                                            seed=seed, return_info=True)
        corr = ops.feature_nn(_t(F0, dev), _t(F1, dev))
        T_d, info_d = ops.ransac_pose_geometric(_t(xyz0, dev), _t(xyz1, dev), corr, 0.3, 0.9, 50000, 1000, seed)
        assert np.array_equal(T, T_d) and info == info_d


def test_feature_widths_other_than_32_are_refused(dev):
    from apr_amd._lib import AprHipError
    f = torch.zeros((8, 16), device=dev)
    with pytest.raises(AprHipError, match="32"):
        ops.score_argmax(f, f)
    with pytest.raises(AprHipError, match="32"):
        BU.mutual_pairs(np.zeros((8, 64), np.float32), np.zeros((8, 64), np.float32))
