"""CPU side of Predator_APR's descriptor loss: the float64 restatement (tests/predator_loss_oracle.py) against the
reference's own text (tests/golden/predator_loss_ref.npz, made by make_predator_loss_ref_golden.py), and the public
interface of apr_amd.predator.lib.loss.MetricLoss.  No GPU compute here."""
import inspect

import numpy as np
import pytest
import torch

from apr_amd.predator.configs.models import kitti_config
from tests import predator_loss_oracle as O

from tests.predator_loss_fixture import CASES, G, GRADS, STATS, case_inputs, fixture_grad


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_fp64_leg(name):
    inp = case_inputs(name)
    for k in GRADS:
        inp[k].requires_grad_(True)
    stats = O.forward(**inp, choice=np.asarray(G[f"{name}/choice"]))
    for k in STATS:
        assert rel(float(stats[k]), float(G[f"{name}/fp64/{k}"])) < 1e-12, (k, float(stats[k]), float(G[f"{name}/fp64/{k}"]))
    (stats["circle_loss"] + stats["overlap_loss"] + stats["saliency_loss"]).backward()
    for k in GRADS:
        ref = fixture_grad(name, k, tuple(inp[k].shape))
        assert np.linalg.norm(inp[k].grad.numpy() - ref) <= 1e-12 * np.linalg.norm(ref), k


def test_fixture_covers_the_branches_it_is_meant_to():
    assert int(G["kitti/n_filtered"]) > O.KITTI["max_points"] and len(G["kitti/choice"]) == O.KITTI["max_points"]
    assert 0 < int(G["short/n_filtered"]) < O.KITTI["max_points"]
    assert 0.2 < float(G["kitti/fp64/circle_loss"]) < 2.0 and 0.3 < float(G["kitti/fp64/recall"]) < 0.97
    # the cluster case: the anchor at the centre of the ball has a positive and no negative
    inp, keep = case_inputs("cluster"), {}
    O.forward(**inp, choice=np.asarray(G["cluster/choice"]), keep=keep)
    cd = keep["coords_dist"]
    no_neg = ((cd < O.KITTI["pos_radius"]).sum(1) > 0) & ((cd > O.KITTI["safe_radius"]).sum(1) == 0)
    assert 0 < int(no_neg.sum()) < len(cd)
    # the short case: an exact tie at the top of a score row
    keep = {}
    O.forward(**case_inputs("short"), choice=np.asarray(G["short/choice"]), keep=keep)
    top = keep["scores"].topk(2, dim=1)[0]
    assert int((top[:, 0] == top[:, 1]).sum()) >= 1


def test_restatement_bce_at_the_clamps():
    p = torch.from_numpy(np.asarray(G["bce/in/prediction"]).astype(np.float64)).requires_grad_(True)
    gt = torch.from_numpy(np.asarray(G["bce/in/gt"]).astype(np.float64))
    assert {0.0, 0.5, 1.0} <= set(np.asarray(G["bce/in/prediction"])[:12].tolist())
    loss, prec, rec = O.weighted_bce(p, gt)
    loss.backward()
    assert rel(float(loss), float(G["bce/fp64/loss"])) < 1e-12
    assert float(prec) == float(G["bce/fp64/precision"]) and float(rec) == float(G["bce/fp64/recall"])
    ref = np.asarray(G["bce/fp64/grad"])
    assert np.linalg.norm(p.grad.numpy() - ref) <= 1e-12 * np.linalg.norm(ref)


def _loss_config():
    return kitti_config(**{k: O.KITTI[k] for k in ("pos_margin", "neg_margin", "max_points", "safe_radius",
                                                   "matchability_radius", "pos_radius")})


def test_metric_loss_has_the_reference_interface():
    """Constructor and forward parameter names of Predator_APR/lib/loss.py:20, :100 (plus the one keyword `choice`)."""
    from apr_amd.predator.lib.loss import MetricLoss
    assert list(inspect.signature(MetricLoss.__init__).parameters) == ["self", "configs", "log_scale", "pos_optimal", "neg_optimal"]
    d = {k: v.default for k, v in inspect.signature(MetricLoss.__init__).parameters.items()}
    assert (d["log_scale"], d["pos_optimal"], d["neg_optimal"]) == (16, 0.1, 1.4)
    fwd = inspect.signature(MetricLoss.forward).parameters
    assert list(fwd) == ["self", "src_pcd", "tgt_pcd", "src_feats", "tgt_feats", "correspondence", "rot", "trans",
                         "scores_overlap", "scores_saliency", "choice"]
    assert fwd["choice"].default is None
    for name, params in (("get_circle_loss", ["self", "coords_dist", "feats_dist"]), ("get_recall", ["self", "coords_dist", "feats_dist"]),
                         ("get_weighted_bce_loss", ["self", "prediction", "gt"])):
        assert list(inspect.signature(getattr(MetricLoss, name)).parameters) == params
    m = MetricLoss(_loss_config())
    assert (m.pos_radius, m.safe_radius, m.matchability_radius, m.max_points) == (0.21, 0.75, 0.3, 512)


def test_metric_loss_refuses_cpu_tensors():
    from apr_amd._lib import AprHipError
    from apr_amd.predator.lib.loss import MetricLoss
    m = MetricLoss(_loss_config())
    inp = case_inputs("cluster", torch.float32)
    with pytest.raises(AprHipError):
        m(**inp)
    with pytest.raises(AprHipError):
        m.get_weighted_bce_loss(torch.rand(8), torch.ones(8))
    with pytest.raises(AprHipError):
        m.get_circle_loss(torch.rand(4, 4), torch.rand(4, 4))
    with pytest.raises(AprHipError):
        m.get_recall(torch.rand(4, 4), torch.rand(4, 4))
