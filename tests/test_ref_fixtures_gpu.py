"""HIP kernels against fixtures produced by the REFERENCE's own function text (tests/golden/fcgf_ref.npz; generator:
tests/golden/make_fcgf_ref_golden.py): SURVEY 8 rows F9 (find_nn_gpu), F11 (est_quad_linear_robust), F12
(hardest-contrastive + _hash), next-1 (NPR regulariser / point assembly), next-2 (APG transform + crop)."""
import os

import numpy as np
import pytest
import torch

from apr_amd.fcgf.lib import apg
from apr_amd.fcgf.lib.eval import find_nn_gpu
from apr_amd.fcgf.lib.trainer import HardestContrastiveLoss
from apr_amd.fcgf.registration import rte_rre
from apr_amd.fcgf.util.transform_estimation import est_quad_linear_robust
from tests import apg_oracle as O

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "fcgf_ref.npz"))


def test_irls_pose_matches_reference_text(dev):
    """Pose within 1e-3 m / 1e-3 deg of the reference's fp32 torch result (BASELINE north_star tolerance)."""
    p0, p1 = torch.from_numpy(G["irls_p0"]).to(dev), torch.from_numpy(G["irls_p1"]).to(dev)
    for key, w in (("irls_T", None), ("irls_T_weighted", torch.from_numpy(G["irls_w"]).to(dev))):
        T = est_quad_linear_robust(p0, p1, w).numpy()
        rte, rre = rte_rre(T, G[key])
        assert rte < 1e-3 and rre < 1e-3, (key, rte, rre)


def test_find_nn_gpu_matches_reference_text(dev):
    F0, F1 = torch.from_numpy(G["nn_F0"]).to(dev), torch.from_numpy(G["nn_F1"]).to(dev)
    inds, d2 = find_nn_gpu(F0, F1, nn_max_n=500, return_distance=True)
    assert inds.dtype == torch.int64 and not inds.is_cuda and tuple(d2.shape) == (len(F0), 1)
    assert np.array_equal(inds.numpy(), G["nn_inds"])             # bit-exact indices, planted tie included
    assert np.allclose(d2.numpy(), G["nn_d2"], rtol=1e-5, atol=1e-6)
    _, d = find_nn_gpu(F0, F1, return_distance=True, dist_type='L2')
    assert np.allclose(d.numpy(), G["nn_d"], rtol=1e-5, atol=1e-6)


def test_hardest_contrastive_matches_reference_text(dev):
    F0, F1 = torch.from_numpy(G["hc_F0"]).to(dev), torch.from_numpy(G["hc_F1"]).to(dev)
    pos = torch.from_numpy(G["hc_pos"])
    crit = HardestContrastiveLoss(pos_thresh=0.1, neg_thresh=1.4)
    for tag in ("a", "b"):
        num_pos, num_hn = (int(v) for v in G[f"hc_{tag}_args"])
        draws = (G[f"hc_{tag}_sel0"], G[f"hc_{tag}_sel1"], G[f"hc_{tag}_pos_sel"] if len(pos) > num_pos else None)
        with torch.no_grad():
            pl, nl = crit.contrastive_hardest_negative_loss(F0, F1, pos, num_pos=num_pos, num_hn_samples=num_hn,
                                                            draws=draws)
        want = G[f"hc_{tag}_loss"]
        assert abs(float(pl) - want[0]) < 1e-5 * max(1.0, abs(want[0])), (tag, float(pl), want)
        assert abs(float(nl) - want[1]) < 1e-5 * max(1.0, abs(want[1])), (tag, float(nl), want)
    # seeded NumPy RNG: the three draws are consumed in the reference's order
    np.random.seed(77)
    with torch.no_grad():
        pl, nl = crit.contrastive_hardest_negative_loss(F0, F1, pos, num_pos=1024, num_hn_samples=256)
    assert abs(float(pl) - G["hc_a_loss"][0]) < 1e-5 and abs(float(nl) - G["hc_a_loss"][1]) < 1e-5


def test_npr_regulariser_and_points_match_reference_text(dev):
    gen = torch.from_numpy(G["npr_generated"]).to(dev)
    coords = torch.from_numpy(G["npr_coords"]).to(dev)
    for kind in ("L2", "RepelL2", "RepelL1"):
        got = float(apg.npr_regulariser(gen, kind, alpha=0.1))
        assert abs(got - float(G[f"npr_reg_{kind}"])) < 1e-5 * max(1.0, abs(float(G[f"npr_reg_{kind}"]))), kind
    pts = apg.npr_points(gen, coords, 0.3, 4)
    assert np.allclose(pts.cpu().numpy(), G["npr_mod_generated"], rtol=0, atol=1e-5)


def test_apg_transform_and_crop_match_reference_text(dev):
    moved = [apg.apply_transform(f, M) for f, M in zip(G["apg_frames"], G["apg_poses"])]
    got = apg.crop_to_radius(G["apg_key"], torch.cat(moved, 0)).cpu().numpy()
    ref = G["apg_nghb"]
    assert abs(len(got) - len(ref)) <= 2                          # fp32 rounding exactly at the crop radius
    # row by row, whatever the counts (tests/apg_oracle.py): order preserved, the same input rows kept as the reference kept,
    # coordinates to fp32 rounding
    moved_host = torch.cat(moved, 0).cpu().numpy()
    O.check_aggregation(G["apg_key"], G["apg_frames"], G["apg_poses"], moved_host, got, ref, atol=2e-5)
