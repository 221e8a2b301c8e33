"""The tester epoch of FCGF_APR on the HIP kernels: `ops.ransac_pose_async` against `ops.ransac_pose`, `FCGFTestEpoch`
(apr_amd/fcgf/lib/tester.py) against the chain of public functions that existed before it, one host round trip each
(`eval.find_corr`, `registration.ransac_feature_matching`, `ops.inlier_ratio`), the overflow replay, and `train_and_test`.

Everything compared here runs the same kernels on the same inputs in both forms, so equality is what is asserted: poses
bit for bit, counts equal.  The hit counts of the chain are taken on the float32 restatement of `evaluate_nn_dist`
(tests/fcgf_test_oracle.py: every operation rounded, the kernel's order), which tests/test_fcgf_test_pair_gpu.py holds to
the kernel at 2 ulp and to the reference's rows at a derived bar; both are rounded operation by operation in one order, so
here the ten counts must be equal.
"""
import os
import time
import types

import numpy as np
import pytest
import torch

from apr_amd import MinkowskiEngine as ME
from apr_amd import ops
from apr_amd.fcgf import registration
from apr_amd.fcgf.lib import learned
from apr_amd.fcgf.lib import tester as FT
from apr_amd.fcgf.lib.eval import find_corr
from apr_amd.fcgf.model import load_model
from tests import fcgf_test_oracle as FO

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VS, SUB, N_POINTS, ITERS = 0.3, 3000, 2800, 5000


def test_ransac_pose_async_decodes_to_ransac_pose_bit_for_bit(dev):
    g = np.load(os.path.join(GOLD, "pose_small.npz"))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    p0, q1, corr = up(g["p0"].astype(np.float32)), up(g["q1"].astype(np.float32)), up(g["corr"].astype(np.int64))
    for iters, seed in ((5000, 7), (20000, 7), (777, 1)):
        T, info = ops.ransac_pose(p0, q1, corr, 0.3, 0.9, iters, seed)
        raw = ops.ransac_pose_async(p0, q1, corr, 0.3, 0.9, iters, seed)
        assert raw.dtype == torch.uint8 and raw.is_cuda and raw.numel() == int(ops._lib_().apr_ransac_raw_bytes())
        T2, info2 = ops.ransac_decode(raw.cpu().numpy(), len(p0))
        assert T2.tobytes() == T.tobytes() and info2 == info, (iters, info, info2)
        assert info["inliers"] > 0 and info["n_valid"] > 0
    T, info = ops.ransac_pose(p0, q1, corr, 0.3, 0.9, 20000, 7)
    assert info["inliers"] == int(g["inliers"]) and info["n_valid"] == int(g["n_valid"])      # the fixture's own run


@pytest.fixture(scope="module")
def world(dev):
    torch.manual_seed(3)
    model = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(dev)
    # 16 beams: about 3400 + 3600, 630 + 620 and 2700 + 3000 voxels
    pairs = [learned.synthetic_pair(dev, seed, n_beams=16, n_azimuth=az, k=1)[0] for seed, az in ((3, 400), (4, 40), (6, 300))]
    return dict(model=model, pairs=pairs)


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def _chained(model, pairs, variant, seeds):
    """The reference's loop body on the public functions, one host round trip each."""
    model.eval()
    rows = []
    with torch.no_grad():
        for d, seed in zip(pairs, seeds):
            F0, F1 = [model(ME.SparseTensor(d[f"sinput{k}_F"], coordinates=d[f"sinput{k}_C"])).F for k in ("0", "1")]
            xyz0, xyz1, T_gt = d["pcd0"][0], d["pcd1"][0], d["T_gt"].numpy().astype(np.float32)
            drew = len(F0) > SUB
            c0, c1 = find_corr(xyz0, xyz1, F0, F1, subsample_size=SUB)
            c0, c1 = c0.cpu().numpy(), c1.cpu().numpy()
            d32 = FO.dists_f32(c0, c1, np.arange(len(c0)), np.arange(len(c0)), T_gt)
            r0, r1, G0, G1 = xyz0, xyz1, F0, F1
            sampled = []
            if variant == "fcgf":                                  # random_sample (test_fcgf.py:54-73), side 0 then side 1
                out = []
                for pts, feats in ((xyz0, F0), (xyz1, F1)):
                    n = len(pts)
                    if n != N_POINTS:
                        choice = np.random.permutation(n)[:N_POINTS] if n > N_POINTS else np.random.choice(n, N_POINTS)
                        idx = torch.from_numpy(choice).to(pts.device)
                        pts, feats = pts[idx], feats[idx]
                    sampled.append("cut" if n > N_POINTS else ("pad" if n < N_POINTS else "keep"))
                    out.append((pts.contiguous(), feats.contiguous()))
                (r0, G0), (r1, G1) = out
            T, info = registration.ransac_feature_matching(r0, r1, G0, G1, VS * 1.0, 4, 0.9, ITERS, seed=seed, return_info=True)
            corr = registration.feature_correspondences(G0, G1)
            shares = []
            for M in (T.astype(np.float32), T_gt):
                rot = torch.from_numpy(np.ascontiguousarray(M[:3, :3])).to(r0.device)
                trans = torch.from_numpy(np.ascontiguousarray(M[:3, 3:])).to(r0.device)
                out8 = ops.inlier_ratio(r0, r1, rot, trans, corr.int(), torch.zeros((1, 2), dtype=torch.int32, device=r0.device),
                                        torch.zeros(1, dtype=torch.int32, device=r0.device), VS * 1.0)[2]
                shares.append(float(out8[0].cpu()))
            rows.append(dict(T=T, info=info, d32=d32, m0=len(c0), k0=len(r0), k1=len(r1), shares=shares, drew=drew, sampled=sampled))
    return rows


@pytest.mark.parametrize("variant", ["apr", "fcgf"])
def test_epoch_equals_the_chain_of_public_functions(world, dev, variant):
    model, pairs = world["model"], world["pairs"]
    seeds = [5, 9, 2]
    epoch = FT.FCGFTestEpoch(model, variant=variant, voxel_size=VS, ransac_iters=ITERS, subsample_size=SUB, n_points=N_POINTS)
    model.train()
    np.random.seed(21)
    summary, rec = epoch.epoch(pairs, seeds=seeds, keep_dists=True)
    state = np.random.get_state()
    assert model.training                                             # left in the mode it was in
    np.random.seed(21)
    ref = _chained(model, pairs, variant, seeds)
    replay = np.random.get_state()
    assert state[0] == replay[0] and np.array_equal(state[1], replay[1]) and state[2:] == replay[2:]
    print("rows", [(w["m0"], w["k0"], w["k1"]) for w in ref], "drew", [w["drew"] for w in ref], "sampled", [w["sampled"] for w in ref])
    assert any(w["drew"] for w in ref) and not all(w["drew"] for w in ref)          # both branches of find_corr
    if variant == "fcgf":
        assert {s for w in ref for s in w["sampled"]} >= {"cut", "pad"}             # both drawing branches of random_sample
    assert rec.shape == (3, ops.FTEST_RECORD_FLOATS) and rec.dtype == np.float64 and summary["n_replayed"] == 0
    T_gt = np.stack([d["T_gt"].numpy().astype(np.float32) for d in pairs])
    for i, (r, w) in enumerate(zip(rec, ref)):
        T32 = w["T"].astype(np.float32)
        assert r[ops.FTEST_T:ops.FTEST_T + 16].tobytes() == T32.astype(np.float64).reshape(16).tobytes(), i
        assert r[ops.FTEST_INLIERS] == w["info"]["inliers"] and r[ops.FTEST_N_VALID] == w["info"]["n_valid"]
        assert r[ops.FTEST_BEST_ITERATION] == w["info"]["best_iteration"]
        assert np.float64(r[ops.FTEST_RMSE]).tobytes() == np.float64(w["info"]["rmse"]).tobytes()
        assert (r[ops.FTEST_M0], r[ops.FTEST_K0], r[ops.FTEST_K1]) == (w["m0"], w["k0"], w["k1"])
        assert r[ops.FTEST_BAD] == 0 and r[ops.FTEST_OVERFLOW] == 0
        assert [r[ops.FTEST_INLIER_EST], r[ops.FTEST_INLIER_GT]] == w["shares"], (i, r[29:31], w["shares"])
        assert summary["dists_nn"][i].dtype == np.float32 and _ulps(summary["dists_nn"][i], w["d32"]) <= 2
        assert r[ops.FTEST_HITS:ops.FTEST_HITS + 10].tolist() == [float((w["d32"].astype(np.float64) < t).sum()) for t in FO.HIT_LEVELS]
        # the record's own figures against the host arithmetic on the same float32 poses
        assert abs(r[ops.FTEST_RTE] - np.linalg.norm(T32[:3, 3].astype(np.float64) - T_gt[i, :3, 3])) < 1e-9
        assert abs(r[ops.FTEST_DIST] - float(summary["dists"][i])) < 1e-5
    want = FT.test_summary(rec[:, ops.FTEST_T:ops.FTEST_T + 16].astype(np.float32).reshape(-1, 4, 4), T_gt)
    for key in ("recall", "success_sum", "success_count"):
        assert summary[key] == want[key]
    for key in ("list_rte", "list_rre", "dists_success", "dists_fail"):
        assert np.array_equal(summary[key], want[key], equal_nan=True)
    assert summary["hit_ratios"].shape == (10, 3) and summary["fmrs"].shape == (10, 10)
    # pairs_per_fetch = 1 and = all, a second run, an explicit RandomState: the same records
    np.random.seed(21)
    _, rec1 = FT.FCGFTestEpoch(model, variant=variant, voxel_size=VS, ransac_iters=ITERS, subsample_size=SUB, n_points=N_POINTS,
                               pairs_per_fetch=1).epoch(pairs, seeds=seeds)
    assert rec1.tobytes() == rec.tobytes()
    np.random.seed(21)
    _, rec2 = epoch.epoch(pairs, seeds=seeds)
    assert rec2.tobytes() == rec.tobytes()
    _, rec3 = epoch.epoch(pairs, seeds=seeds, rng=np.random.RandomState(21))
    assert rec3.tobytes() == rec.tobytes()


class _PlantedModel:
    """Stands in for the encoder: hands out the given feature tensors in call order."""

    def __init__(self, feats):
        self.feats, self.calls, self.training = feats, 0, False

    def eval(self):
        return self.train(False)

    def train(self, mode=True):
        self.training = mode
        return self

    def __call__(self, sparse_tensor):
        self.calls += 1
        return types.SimpleNamespace(F=self.feats[(self.calls - 1) % len(self.feats)])


def test_a_pair_whose_single_round_overflows_is_replayed_through_ransac_pose(dev):
    """Perfect correspondences: every hypothesis passes both checkers, so with max_iter = 1.5 * 2^20 (a sample that repeats a row is no hypothesis: headroom for those) the single round
    reports total_valid > 2^20 and its pose is not final."""
    iters, n = 3 << 19, 400
    rng = np.random.default_rng(0)
    key = torch.from_numpy(rng.uniform(-20, 20, (n, 3)).astype(np.float32)).to(dev)
    m = ops.build_map(ops.voxelize(key, VS, 0), want_first=True)
    ops.finalize_maps([m])
    p0 = key[m.first.long()].contiguous()
    a = np.deg2rad(7.0)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = [6.0, -0.5, 0.1]
    Tt = torch.from_numpy(T)
    p1 = (p0 @ Tt[:3, :3].t().to(dev) + Tt[:3, 3].to(dev)).contiguous()
    f = rng.standard_normal((m.n, 32))
    feats = torch.from_numpy((f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)).to(dev)
    d = {"pcd0": [p0], "pcd1": [p1], "sinput0_C": m.coords, "sinput0_F": torch.ones((m.n, 1), device=dev),
         "sinput1_C": m.coords, "sinput1_F": torch.ones((m.n, 1), device=dev), "T_gt": Tt}
    model = _PlantedModel([feats, feats])
    t0 = time.perf_counter()
    summary, rec = FT.FCGFTestEpoch(model, variant="apr", voxel_size=VS, ransac_iters=iters).epoch([d], seeds=[4])
    print(f"{time.perf_counter() - t0:.2f} s; n_valid {rec[0, ops.FTEST_N_VALID]}, inliers {rec[0, ops.FTEST_INLIERS]} of {m.n}")
    assert summary["n_replayed"] == 1 and summary["replayed"] == [0] and model.calls == 2
    corr = torch.arange(m.n, dtype=torch.int64, device=dev)
    raw = ops.ransac_pose_async(p0, p1, corr, VS, 0.9, iters, 4)
    _, single = ops.ransac_decode(raw.cpu().numpy(), m.n)
    assert single["n_valid"] > 1 << 20                                # the single round did overflow
    T_want, info = ops.ransac_pose(p0, p1, corr, VS, 0.9, iters, 4)
    r = rec[0]
    assert r[ops.FTEST_T:ops.FTEST_T + 16].tobytes() == T_want.astype(np.float32).astype(np.float64).reshape(16).tobytes()
    assert r[ops.FTEST_INLIERS] == info["inliers"] == m.n and r[ops.FTEST_N_VALID] == info["n_valid"]
    assert r[ops.FTEST_BEST_ITERATION] == info["best_iteration"] and r[ops.FTEST_OVERFLOW] == 0
    assert np.float64(r[ops.FTEST_RMSE]).tobytes() == np.float64(info["rmse"]).tobytes()
    assert r[ops.FTEST_SUCCESS] == 1.0 and summary["recall"] == 1.0 and r[ops.FTEST_HITS] == m.n


KEYS = {"losses", "summary", "fmr", "records", "recall", "n_replayed", "train_seeds", "test_seeds", "voxels", "ransac_iters", "seconds"}


def test_train_and_test_repeats_bit_for_bit(dev):
    """The budget of tests/test_valid_epoch_gpu.py's learned-features test: ResUNetBN2C-32 on 16 x 600-ray pairs, 4 training
    and 3 held-out pairs, 800 iterations.  No recall bar."""
    t0 = time.perf_counter()
    kw = dict(n_train=4, n_test=3, iterations=800, trainer="apr", model="ResUNetBN2C", n_out=32, n_beams=16, n_azimuth=600,
              seed=0, k=2, lr=0.05, num_pos=256, num_hn=128, ransac_iters=20000, subsample_size=2500, n_points=2500)
    a = learned.train_and_test(dev, **kw)
    b = learned.train_and_test(dev, **kw)
    s = a["summary"]
    print(f"{time.perf_counter() - t0:.1f} s; seconds {a['seconds']}; loss {a['losses'][0]:.4f} -> {a['losses'][-1]:.4f}; recall "
          f"{a['recall']} n_replayed {a['n_replayed']} rte {s['list_rte']} rre {s['list_rre']} hit ratio at 0.3 m {a['fmr']['hit_ratios'][2]}")
    assert set(a) == KEYS and {"data", "train", "test", "total"} <= set(a["seconds"])
    assert a["losses"] == b["losses"] and len(a["losses"]) == 800 and np.isfinite(a["losses"]).all()
    assert a["records"].tobytes() == b["records"].tobytes() and a["records"].shape == (3, ops.FTEST_RECORD_FLOATS)
    assert 0 <= a["recall"] <= 1 and a["recall"] == s["recall"] == s["success_sum"] / s["success_count"]
    assert a["n_replayed"] == s["n_replayed"] and a["fmr"]["fmrs"].shape == (10, 10)
    for key in ("rte_avg", "rte_var", "rre_avg", "rre_var", "dists_success", "dists_fail", "list_rte", "list_rre", "rres", "rtes",
                "dists", "T_gt", "T_est", "hit_ratios", "fmrs", "replayed"):
        assert key in s, key


def test_train_and_test_with_the_fcgf_trainer(dev):
    kw = dict(n_train=2, n_test=2, iterations=6, trainer="fcgf", model="ResUNetBN2C", n_out=32, n_beams=16, n_azimuth=300,
              seed=1, k=1, lr=0.05, num_pos=256, num_hn=128, ransac_iters=5000, subsample_size=1500, n_points=1500)
    a = learned.train_and_test(dev, **kw)
    assert set(a) == KEYS and len(a["losses"]) == 6 and np.isfinite(a["losses"]).all() and 0 <= a["recall"] <= 1
    assert (a["records"][:, ops.FTEST_K0] == 1500).all() and (a["records"][:, ops.FTEST_K1] == 1500).all()
    with pytest.raises(ValueError):
        learned.train_and_test(dev, 1, 1, 0, trainer="fcgf", symmetric=True)
    with pytest.raises(ValueError):
        learned.train_and_test(dev, 1, 1, 0, trainer="other")
