"""A restatement of Predator_APR's `MetricLoss` (lib/loss.py:16-178, with `square_distance`, lib/utils.py:78-98) in plain
torch ops, in the dtype of its inputs: float64 on the CPU it is the yardstick of the HIP kernels, float32 on the GPU it is
the speed baseline of scripts/predator_loss_time.py.  Against the reference's own text (tests/golden/
predator_loss_ref.npz, fp64 leg) it agrees to 1e-12 (tests/test_predator_loss_cpu.py).

Differences from the reference's text, none of which changes a value: the unique index lists are sorted (the reference
takes them from a Python set), precision / recall are counted with tensor ops (the reference calls sklearn), nothing names
a device, the permutation is an argument, and arg-maxes / arg-mins can be pinned by the caller.
"""
import numpy as np
import torch
import torch.nn.functional as F

KITTI = dict(pos_margin=0.1, neg_margin=1.4, max_points=512, safe_radius=0.75, matchability_radius=0.3, pos_radius=0.21,
             log_scale=16, pos_optimal=0.1, neg_optimal=1.4)


def square_distance(src, dst, normalised=False):
    dist = -2 * torch.matmul(src, dst.transpose(-1, -2))
    if normalised:
        dist = dist + 2
    else:
        dist = dist + torch.sum(src ** 2, dim=-1)[..., :, None] + torch.sum(dst ** 2, dim=-1)[..., None, :]
    return torch.clamp(dist, min=1e-12, max=None)


def circle_loss(coords_dist, feats_dist, p=KITTI):
    pos_mask = coords_dist < p["pos_radius"]
    neg_mask = coords_dist > p["safe_radius"]
    row_sel = ((pos_mask.sum(-1) > 0) * (neg_mask.sum(-1) > 0)).detach()
    col_sel = ((pos_mask.sum(-2) > 0) * (neg_mask.sum(-2) > 0)).detach()
    pos_weight = feats_dist - 1e5 * (~pos_mask).to(feats_dist.dtype)
    pos_weight = pos_weight - p["pos_optimal"]
    pos_weight = torch.max(torch.zeros_like(pos_weight), pos_weight).detach()
    neg_weight = feats_dist + 1e5 * (~neg_mask).to(feats_dist.dtype)
    neg_weight = p["neg_optimal"] - neg_weight
    neg_weight = torch.max(torch.zeros_like(neg_weight), neg_weight).detach()
    ls = p["log_scale"]
    lse_pos_row = torch.logsumexp(ls * (feats_dist - p["pos_margin"]) * pos_weight, dim=-1)
    lse_pos_col = torch.logsumexp(ls * (feats_dist - p["pos_margin"]) * pos_weight, dim=-2)
    lse_neg_row = torch.logsumexp(ls * (p["neg_margin"] - feats_dist) * neg_weight, dim=-1)
    lse_neg_col = torch.logsumexp(ls * (p["neg_margin"] - feats_dist) * neg_weight, dim=-2)
    loss_row = F.softplus(lse_pos_row + lse_neg_row) / ls
    loss_col = F.softplus(lse_pos_col + lse_neg_col) / ls
    return (loss_row[row_sel].mean() + loss_col[col_sel].mean()) / 2


def recall(coords_dist, feats_dist, p=KITTI, sel_idx=None):
    pos_mask = coords_dist < p["pos_radius"]
    n_gt_pos = (pos_mask.sum(-1) > 0).to(coords_dist.dtype).sum() + 1e-12
    if sel_idx is None:
        _, sel_idx = torch.min(feats_dist, -1)
    sel_dist = torch.gather(coords_dist, dim=-1, index=sel_idx[:, None])[pos_mask.sum(-1) > 0]
    return (sel_dist < p["pos_radius"]).to(coords_dist.dtype).sum() / n_gt_pos


def weighted_bce(prediction, gt):
    """-> (loss, precision, recall): nn.BCELoss (log clamped at -100), class weights from the label share, round() half to
    even, zero denominators -> 0 as sklearn's precision_recall_fscore_support(average='binary')."""
    class_loss = F.binary_cross_entropy(prediction, gt, reduction='none')
    weights = torch.ones_like(gt)
    w_negative = gt.sum() / gt.size(0)
    w_positive = 1 - w_negative
    weights[gt >= 0.5] = w_positive
    weights[gt < 0.5] = w_negative
    loss = torch.mean(weights * class_loss)
    hat = prediction.detach().round() > 0.5
    pos = gt > 0.5
    tp, fp, fn = (hat & pos).sum(), (hat & ~pos).sum(), (~hat & pos).sum()
    one = lambda a, b: (a.to(gt.dtype) / b.to(gt.dtype)) if int(b) > 0 else torch.zeros((), dtype=gt.dtype, device=gt.device)
    return loss, one(tp, tp + fp), one(tp, tp + fn)


def forward(src_pcd, tgt_pcd, src_feats, tgt_feats, correspondence, rot, trans, scores_overlap, scores_saliency, p=KITTI,
            choice=None, pins=None, keep=None):
    """The reference's forward.  `choice`: the permutation of :157 (None: drawn from np.random as the reference does).
    `pins`: dict with any of row_arg / col_arg (:135, :137) and nn (:73) to take those decisions from the caller.
    `keep`: dict that receives the intermediates (index lists, arg-maxes, distances, margins)."""
    pins, keep = pins or {}, {} if keep is None else keep
    src_pcd = (torch.matmul(rot, src_pcd.transpose(0, 1)) + trans).transpose(0, 1)
    stats = dict()
    src_idx = torch.unique(correspondence[:, 0])
    tgt_idx = torch.unique(correspondence[:, 1])
    src_gt = torch.zeros(src_pcd.size(0), dtype=src_pcd.dtype, device=src_pcd.device)
    src_gt[src_idx] = 1.
    tgt_gt = torch.zeros(tgt_pcd.size(0), dtype=src_pcd.dtype, device=src_pcd.device)
    tgt_gt[tgt_idx] = 1.
    gt_labels = torch.cat((src_gt, tgt_gt))
    stats['overlap_loss'], stats['overlap_precision'], stats['overlap_recall'] = weighted_bce(scores_overlap, gt_labels)

    src_feats_sel, src_pcd_sel = src_feats[src_idx], src_pcd[src_idx]
    tgt_feats_sel, tgt_pcd_sel = tgt_feats[tgt_idx], tgt_pcd[tgt_idx]
    scores = torch.matmul(src_feats_sel, tgt_feats_sel.transpose(0, 1))
    idx1 = pins["row_arg"] if "row_arg" in pins else scores.max(1)[1]
    distance_1 = torch.norm(src_pcd_sel - tgt_pcd_sel[idx1], p=2, dim=1)
    idx2 = pins["col_arg"] if "col_arg" in pins else scores.max(0)[1]
    distance_2 = torch.norm(tgt_pcd_sel - src_pcd_sel[idx2], p=2, dim=1)
    r = p["matchability_radius"]
    gt_labels = torch.cat(((distance_1 < r).to(src_pcd.dtype), (distance_2 < r).to(src_pcd.dtype)))
    n_src = src_pcd.size(0)
    sal = torch.cat((scores_saliency[:n_src][src_idx], scores_saliency[n_src:][tgt_idx]))
    stats['saliency_loss'], stats['saliency_precision'], stats['saliency_recall'] = weighted_bce(sal, gt_labels)
    keep.update(src_idx=src_idx, tgt_idx=tgt_idx, row_arg=idx1, col_arg=idx2, scores=scores.detach(),
                saliency_dist=torch.cat((distance_1, distance_2)).detach(), saliency_labels=gt_labels, saliency_pred=sal.detach(),
                overlap_gt=torch.cat((src_gt, tgt_gt)))

    c_dist = torch.norm(src_pcd[correspondence[:, 0]] - tgt_pcd[correspondence[:, 1]], dim=1)
    c_select = c_dist < p["pos_radius"] - 0.001
    keep.update(c_dist=c_dist.detach(), n_filtered=int(c_select.sum()))
    correspondence = correspondence[c_select]
    if correspondence.size(0) > p["max_points"]:
        if choice is None:
            choice = np.random.permutation(correspondence.size(0))[:p["max_points"]]
        correspondence = correspondence[torch.as_tensor(np.asarray(choice), device=correspondence.device)]
    keep["choice"] = choice
    s_idx, t_idx = correspondence[:, 0], correspondence[:, 1]
    a_pcd, b_pcd = src_pcd[s_idx], tgt_pcd[t_idx]
    a_f, b_f = src_feats[s_idx], tgt_feats[t_idx]
    coords_dist = torch.sqrt(square_distance(a_pcd[None], b_pcd[None]).squeeze(0))
    feats_dist = torch.sqrt(square_distance(a_f[None], b_f[None], normalised=True)).squeeze(0)
    keep.update(coords_dist=coords_dist.detach(), feats_dist=feats_dist.detach())
    stats['recall'] = recall(coords_dist, feats_dist, p, pins.get("nn"))
    stats['circle_loss'] = circle_loss(coords_dist, feats_dist, p)
    return stats
