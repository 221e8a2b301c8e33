"""apr_valid_pair (csrc/valid.hip): the matching metrics of one validation pair in one launch, against the fixture the
REFERENCE's own text produced (tests/golden/valid_ref.npz; generator tests/golden/make_valid_ref_golden.py) and against
float64 recomputations from the kernel's own pose.  Tolerances are bounded from the data in each test, not chosen."""
import os

import numpy as np
import pytest
import torch

from apr_amd import ops
from apr_amd.fcgf.lib.validation import GenerativePairValidStep, reduce_records
from apr_amd.fcgf.registration import rte_rre
from apr_amd.fcgf.util.transform_estimation import est_quad_linear_robust

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "valid_ref.npz"), allow_pickle=False)
EPS = 2.0 ** -24


def _records(dev, n=1):
    return torch.full((n, ops.VALID_RECORD_FLOATS), -7.0, dtype=torch.float32, device=dev)


def _fixture_call(dev, rec=None, slot=0):
    """The fixture's pair through the step's own subsample + NN + apr_valid_pair chain -> (record, inds0, inds1, nn)."""
    t = lambda k: torch.from_numpy(G[k]).to(dev)
    step = GenerativePairValidStep(None, None, subsample_size=int(G["subsample_size"]), hit_ratio_thresh=float(G["hit_thresh"]))
    np.random.seed(int(G["seed"]))
    inds0, inds1 = step.draw_subsample(len(G["F0"]), len(G["F1"]))
    sel0, sel1 = torch.from_numpy(inds0).to(dev), torch.from_numpy(inds1).to(dev)
    nn = ops.feature_nn(t("F0").index_select(0, sel0), t("F1").index_select(0, sel1))
    rec = _records(dev) if rec is None else rec
    ops.valid_pair(t("xyz0"), t("xyz1"), nn, t("T_gt").reshape(-1), rec, slot, sel0=sel0, sel1=sel1,
                   hit_thresh=float(G["hit_thresh"]))
    return rec, inds0, inds1, nn


def _small_angle_deg(Ta, Tb):
    """Angle of Ra^T Rb in degrees from its skew-symmetric part (sin of the angle): well conditioned near zero."""
    R = Ta[:3, :3].astype(np.float64).T @ Tb[:3, :3].astype(np.float64)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
    return float(np.degrees(np.arcsin(min(np.linalg.norm(v), 1.0))))


def _corr64(inds0, inds1, nn):
    return G["xyz0"][inds0].astype(np.float64), G["xyz1"][inds1[nn]].astype(np.float64)


def test_subsample_nn_and_pose_match_the_reference_fixture(dev):
    rec, inds0, inds1, nn = _fixture_call(dev)
    nn = nn.cpu().numpy()
    assert np.array_equal(inds0, G["inds0"]) and np.array_equal(inds1, G["inds1"])      # the reference's two draws
    assert np.array_equal(nn, G["nn"])
    r = rec.cpu().numpy()[0]
    assert r[ops.VALID_N_CORR] == len(inds0)
    T = r[ops.VALID_T_EST:ops.VALID_T_EST + 16].reshape(4, 4)
    # shared device code: the bits of est_quad_linear_robust on the same correspondences
    p0, p1 = torch.from_numpy(G["xyz0"][inds0]).to(dev), torch.from_numpy(G["xyz1"][inds1[nn]]).to(dev)
    T_irls = est_quad_linear_robust(p0, p1).numpy()
    assert T.tobytes() == T_irls.tobytes()
    # the bar of tests/test_ref_fixtures_gpu.py for this function: 1e-3 m, 1e-3 deg.  The angle between the two float32
    # matrices is taken from the skew part of R^T R_ref: `rte_rre`'s arccos cannot resolve 1e-3 deg here -- twenty
    # float32 compositions leave the reference's own matrix 1e-7 off orthonormal, and rte_rre(G["T_est"], G["T_est"])
    # already reads 0.036 deg
    rte, _ = rte_rre(T, G["T_est"])
    rre = _small_angle_deg(T, G["T_est"])
    print(f"T_est vs reference fixture: {rte:.3e} m, {rre:.3e} deg, max |dT| {np.abs(T - G['T_est']).max():.2e}")
    assert rte < 1e-3 and rre < 1e-3, (rte, rre)
    # the reference's five numbers, for the record: corr_dist / rte / rre move with the pose within the same bar
    print("record", r[:5], "fixture", [float(G[k]) for k in ("corr_dist", "rte", "rre", "hit_ratio")])
    assert bool(reduce_records(r[None], 0.1)["feat_match_ratio"]) == bool(G["feat_match"])


def test_hit_ratio_is_the_count_of_float64_hits(dev):
    rec, inds0, inds1, nn = _fixture_call(dev)
    r = rec.cpu().numpy()[0]
    p0, p1 = _corr64(inds0, inds1, nn.cpu().numpy())
    Tg = G["T_gt"].astype(np.float64)
    d = np.sqrt(((p0 @ Tg[:3, :3].T + Tg[:3, 3] - p1) ** 2).sum(1) + 1e-6)
    thr = float(G["hit_thresh"])
    sure = int((d < thr - 1e-5).sum())
    border = int((np.abs(d - thr) <= 1e-5).sum())
    count = int(r[ops.VALID_N_HIT])
    print(f"hits {count}, sure {sure}, borderline {border} of {len(d)}; fixture ratio {float(G['hit_ratio'])}")
    assert border <= len(d) / 1000
    assert sure <= count <= sure + border
    assert r[ops.VALID_HIT_RATIO] == np.float32(count) / np.float32(len(d))
    assert sure <= round(float(G["hit_ratio"]) * len(d)) <= sure + border            # the reference counts the same hits


def _expected64(r, xyz0, T_gt):
    T = r[ops.VALID_T_EST:ops.VALID_T_EST + 16].reshape(4, 4).astype(np.float64)
    Tg = np.asarray(T_gt, dtype=np.float64).reshape(4, 4)
    x = xyz0.astype(np.float64)
    gap = np.linalg.norm((x @ T[:3, :3].T + T[:3, 3]) - (x @ Tg[:3, :3].T + Tg[:3, 3]), axis=1)
    cos = (np.trace(T[:3, :3].T @ Tg[:3, :3]) - 1) / 2
    return np.minimum(gap, 1.0).mean(), np.linalg.norm(T[:3, 3] - Tg[:3, 3]), cos


def test_corr_dist_rte_rre_against_float64_from_the_kernels_own_pose(dev):
    rec, _, _, _ = _fixture_call(dev)
    r = rec.cpu().numpy()[0]
    cd, rte, cos = _expected64(r, G["xyz0"], G["T_gt"])
    # a dozen float32 roundings on coordinates of magnitude max|x|
    bound = 16 * EPS * float(np.abs(G["xyz0"]).max())
    rre = np.arccos(cos)
    rre_bound = 8 * EPS / np.sin(rre) + 2 * EPS * rre        # cosine within 8 * 2^-24, then the float32 store of the angle
    print(f"corr_dist {r[0]} vs {cd} (bound {bound:.2e}); rte {r[1]} vs {rte}; rre {r[2]} vs {rre} (bound {rre_bound:.2e})")
    assert np.degrees(rre) > 0.5                             # the fixture keeps the angle where the bound means something
    assert abs(float(r[ops.VALID_CORR_DIST]) - cd) <= bound
    assert abs(float(r[ops.VALID_RTE]) - rte) <= bound
    assert abs(float(r[ops.VALID_RRE]) - rre) <= rre_bound
    # and the reference's own float32 numbers lie within the same bounds plus what the 1e-3 pose bar allows
    assert abs(float(r[ops.VALID_CORR_DIST]) - float(G["corr_dist"])) < 2e-3
    assert abs(float(r[ops.VALID_RTE]) - float(G["rte"])) < 1e-3 + bound


def test_cosine_above_one_gives_nan_and_the_epoch_skips_it(dev):
    """Identical clouds (pose fit: the identity) and a hand-made ground truth whose rotation has 1 + 2^-23 on the diagonal,
    as a float32 rotation matrix can after rounding: trace / 2 - 1/2 = 1 + 1.5 * 2^-23 > 1 -> NaN as np.arccos gives."""
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.uniform(-20, 20, (700, 3)).astype(np.float32)).to(dev)
    T_gt = np.eye(4, dtype=np.float32)
    T_gt[0, 0] = T_gt[1, 1] = T_gt[2, 2] = np.float32(1) + np.float32(2.0 ** -23)
    nn = torch.arange(700, dtype=torch.int64, device=dev)
    rec = _records(dev, 2)
    ops.valid_pair(x, x, nn, torch.from_numpy(T_gt).to(dev).reshape(-1), rec, 0)
    good = np.eye(4, dtype=np.float32)
    good[:3, 3] = [0.5, 0.0, 0.0]
    ops.valid_pair(x, x, nn, torch.from_numpy(good).to(dev).reshape(-1), rec, 1)
    r = rec.cpu().numpy()
    _, _, cos = _expected64(r[0], x.cpu().numpy(), T_gt)
    assert cos > 1.0 and np.isnan(r[0, ops.VALID_RRE])
    assert np.isfinite(r[0, [0, 1, 3, 4]]).all() and r[0, ops.VALID_N_CORR] == 700
    assert r[1, ops.VALID_RRE] == 0.0 and abs(r[1, ops.VALID_RTE] - 0.5) < 1e-6
    r[:, ops.VALID_CHAMFER:ops.VALID_REG + 1] = 0.0
    out = reduce_records(r, 0.1)
    assert out["rre"] == 0.0 and np.isfinite(out["rte"])      # the NaN pair is left out of the rre mean only


def test_same_bits_on_a_second_call_and_null_selection_is_identity(dev):
    rec = _records(dev, 4)
    _fixture_call(dev, rec, 0)
    _, inds0, inds1, nn = _fixture_call(dev, rec, 1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x0, x1 = t(G["xyz0"][inds0]), t(G["xyz1"][inds1])
    Tg = t(G["T_gt"]).reshape(-1)
    ops.valid_pair(x0, x1, nn, Tg, rec, 2)
    ident0 = torch.arange(len(inds0), dtype=torch.int64, device=dev)
    ident1 = torch.arange(len(inds1), dtype=torch.int64, device=dev)
    ops.valid_pair(x0, x1, nn, Tg, rec, 3, sel0=ident0, sel1=ident1)
    r = rec.cpu().numpy()
    used = list(range(21)) + [ops.VALID_N_HIT]
    assert r[0, used].tobytes() == r[1, used].tobytes()
    assert r[2, used].tobytes() == r[3, used].tobytes()
    assert (r[:, ops.VALID_CHAMFER:ops.VALID_REG + 1] == -7.0).all()          # the caller's two floats are left alone


def test_out_of_range_indices_are_reported_not_followed(dev):
    x = torch.zeros((10, 3), device=dev)
    nn = torch.arange(10, dtype=torch.int64, device=dev)
    nn[3] = 10
    nn[7] = -1
    rec = _records(dev)
    ops.valid_pair(x, x, nn, torch.eye(4, device=dev).reshape(-1), rec, 0)
    r = rec.cpu().numpy()
    assert r[0, ops.VALID_N_CORR] == -2
    with pytest.raises(ValueError):
        reduce_records(r, 0.1)
    with pytest.raises(Exception):
        ops.valid_pair(x, x, nn, torch.eye(4, device=dev).reshape(-1), rec, 1)      # slot outside the buffer
