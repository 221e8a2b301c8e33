"""Helpers of the descriptor-loss tests: the fixture tests/golden/predator_loss_ref.npz (made by
tests/golden/make_predator_loss_ref_golden.py) and the small pair the whole-iteration test trains on."""
import os

import numpy as np
import torch

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "predator_loss_ref.npz"), allow_pickle=False)
CASES = ("kitti", "short", "cluster")
STATS = ("circle_loss", "recall", "overlap_loss", "overlap_recall", "overlap_precision", "saliency_loss", "saliency_recall",
         "saliency_precision")
GRADS = ("src_feats", "tgt_feats", "scores_overlap", "scores_saliency")


def case_inputs(name, dtype=torch.float64, device="cpu"):
    out = {}
    for k in ("src_pcd", "tgt_pcd", "src_feats", "tgt_feats", "correspondence", "rot", "trans", "scores_overlap",
              "scores_saliency"):
        v = np.asarray(G[f"{name}/in/{k}"])
        out[k] = torch.from_numpy(v.astype(np.int64)).to(device) if k == "correspondence" \
            else torch.from_numpy(v.astype(np.float64)).to(dtype).to(device)
    return out


def fixture_grad(name, key, shape):
    """The fp64 leg's gradient, dense (the feature gradients are stored by non-zero row)."""
    g = np.asarray(G[f"{name}/fp64/grad_{key}"])
    if f"{name}/fp64/grad_{key}_rows" in G.files:
        full = np.zeros(shape)
        full[np.asarray(G[f"{name}/fp64/grad_{key}_rows"])] = g
        return full
    return g



LOSS_KEYS = ("pos_margin", "neg_margin", "max_points", "safe_radius", "matchability_radius", "pos_radius")
TRAIN = dict(w_circle_loss=1.0, w_overlap_loss=1.0, w_saliency_loss=0.0, loss_ratio=0.001, regularization_strength=0.01)
# Predator_APR/configs/train/kitti.yaml:41-53


def train_config():
    from apr_amd.predator.configs.models import kitti_config
    from tests.predator_loss_oracle import KITTI
    return kitti_config(**{k: KITTI[k] for k in LOSS_KEYS}, **TRAIN)


def small_pair(seed=13, beams=16, azimuth=400):
    """synth.make_pair(seed) with one barycentre per 0.3 m cell (the reference's own grid subsampling, oracle/_ref),
    correspondences within 0.45 m, and a stand-in APG cloud per frame (its own points doubled and jittered)."""
    from scipy.spatial import cKDTree
    from apr_amd import synth
    from oracle import predator_points_oracle as PREF
    a, b, T = synth.make_pair(seed, n_beams=beams, n_azimuth=azimuth)
    pts, lens = PREF.subsample_batch(np.concatenate([a, b]), np.array([len(a), len(b)], np.int32), sampleDl=0.3)
    src, tgt = pts[:lens[0]], pts[lens[0]:]
    R, t = T[:3, :3].astype(np.float32), T[:3, 3].astype(np.float32)
    hits = cKDTree(tgt.astype(np.float64)).query_ball_point((src @ R.T + t).astype(np.float64), 0.45)
    corr = np.array([(i, j) for i, h in enumerate(hits) for j in sorted(h)], np.int64).reshape(-1, 2)
    rng = np.random.default_rng(seed)
    nghb = [(np.tile(p, (2, 1)) + rng.normal(0, 0.1, (2 * len(p), 3))).astype(np.float32) for p in (src, tgt)]
    return dict(src=src, tgt=tgt, rot=R, trans=t.reshape(3, 1), corr=corr, src_nghb=nghb[0], tgt_nghb=nghb[1])


def collated(pair, cfg, limits, dev):
    """collate_fn_descriptor's dict for one pair with the trainer's extra keys, on the device."""
    from apr_amd.predator.datasets.dataloader import collate_fn_descriptor
    t = lambda v: torch.from_numpy(v).to(dev)
    one = lambda p: np.ones((len(p), 1), np.float32)
    item = (pair["src"], pair["tgt"], one(pair["src"]), one(pair["tgt"]), t(pair["rot"]), t(pair["trans"]), t(pair["corr"]),
            t(pair["src"]), t(pair["tgt"]), t(pair["src_nghb"]), t(pair["tgt_nghb"]), None)
    return collate_fn_descriptor([item], cfg, limits)
