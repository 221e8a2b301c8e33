"""KPFCNNDecoder (the symmetric generator of Predator_APR, models/architectures.py:215-340) on the host: its schedule, its
`state_dict` layout against the fixture the reference itself wrote (tests/golden/make_predator_decoder_ref_golden.py) and
the schedule of KPFCNN, which the shared walk must not have changed."""
import os

import numpy as np
import torch

from apr_amd.predator.configs.models import architectures, kitti_config
from apr_amd.predator.models import blocks
from apr_amd.predator.models.architectures import KPFCNN, KPFCNNDecoder, plan_architecture, plan_decoder_architecture

GOLD = os.path.join(os.path.dirname(__file__), "golden", "predator_decoder_ref.npz")

# plan_architecture(kitti_config()) of the commit before KPFCNNDecoder existed
KPFCNN_PLAN = (
    [('simple', 1.275, 1, 256, 0), ('resnetb', 1.275, 128, 256, 0), ('resnetb_strided', 1.275, 256, 256, 0),
     ('resnetb', 2.55, 256, 512, 1), ('resnetb', 2.55, 512, 512, 1), ('resnetb_strided', 2.55, 512, 512, 1),
     ('resnetb', 5.1, 512, 1024, 2), ('resnetb', 5.1, 1024, 1024, 2), ('resnetb_strided', 5.1, 1024, 1024, 2),
     ('resnetb', 10.2, 1024, 2048, 3), ('resnetb', 10.2, 2048, 2048, 3)],
    [('nearest_upsample', 10.2, 2048, 258, 3), ('unary', 5.1, 1282, 129, 2), ('nearest_upsample', 5.1, 129, 129, 2),
     ('unary', 2.55, 641, 64, 1), ('nearest_upsample', 2.55, 64, 64, 1), ('last_unary', 1.275, 320, 32, 0)],
    [2, 5, 8, 11], [256, 512, 1024, 2048], [1, 3, 5], 2048)


def _symmetric_config(**over):
    return kitti_config(symmetric=True, switch_to_decoder=True, **over)


def _pair_of_models():
    """main.py:52-63 under the fixture's seeds: KPFCNN with switch_to_decoder = False, then the decoder"""
    np.random.seed(0)
    torch.manual_seed(0)
    cfg = kitti_config(symmetric=True, switch_to_decoder=False)
    enc = KPFCNN(cfg)
    cfg.switch_to_decoder = True
    return enc, KPFCNNDecoder(cfg)


def test_kpfcnn_schedule_is_what_it_was():
    assert plan_architecture(kitti_config()) == KPFCNN_PLAN
    # the two config keys the generator reads do not reach the schedule (block_decider reads them)
    assert plan_architecture(_symmetric_config()) == KPFCNN_PLAN


def test_decoder_schedule():
    enc, dec, skips, skip_widths, concats, _ = plan_decoder_architecture(_symmetric_config())
    assert [r[2:4] for r in enc] == [(32, 256), (128, 256), (256, 256), (256, 512), (512, 512), (512, 512), (512, 1024),
                                     (1024, 1024), (1024, 1024), (1024, 2048), (2048, 2048)]
    assert [r[:1] + r[2:] for r in dec] == [('nearest_upsample', 2048, 2048, 3), ('unary', 3072, 1024, 2),
                                            ('nearest_upsample', 1024, 1024, 2), ('unary', 1536, 512, 1),
                                            ('nearest_upsample', 512, 512, 1), ('last_unary', 768, 256, 0)]
    assert [r[1] for r in enc] == [r[1] for r in KPFCNN_PLAN[0]] and [r[1] for r in dec] == [r[1] for r in KPFCNN_PLAN[1]]
    assert (skips, skip_widths, concats) == ([2, 5, 8, 11], [256, 512, 1024, 2048], [1, 3, 5])


def test_same_seeds_give_the_reference_layout_and_weights():
    g = np.load(GOLD)
    enc, dec = _pair_of_models()
    sd = dec.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["dec_keys"]] and len(sd) == 50
    assert list(enc.state_dict().keys()) == [str(k) for k in g["enc_keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g["dec_shapes"]]
    assert list(sd.keys())[0] == "epsilon" and float(sd["epsilon"]) == -5.0
    assert sum(p.numel() for p in dec.parameters()) == 23991792
    for model, key in ((enc, "enc_weight_abs_sum"), (dec, "dec_weight_abs_sum")):
        wsum = float(sum(v.double().abs().sum() for v in model.state_dict().values()))
        assert abs(wsum - float(g[key])) <= 1e-9 * wsum, (key, wsum, float(g[key]))
    # a strict load of its own state_dict into a fresh module: no key missing, none unexpected
    fresh = KPFCNNDecoder(_symmetric_config())
    fresh.load_state_dict(sd, strict=True)


def test_widths_and_attributes():
    _, dec = _pair_of_models()
    sd = dec.state_dict()
    assert tuple(sd["encoder_blocks.0.KPConv.weights"].shape) == (15, 32, 128)
    assert tuple(sd["encoder_blocks.10.KPConv.weights"].shape) == (15, 512, 512)
    assert dec.encoder_blocks[10].out_dim == 2048
    assert tuple(sd["decoder_blocks.1.mlp.weight"].shape) == (1024, 3072)
    assert tuple(sd["decoder_blocks.3.mlp.weight"].shape) == (512, 1536)
    assert tuple(sd["decoder_blocks.5.mlp.weight"].shape) == (12, 768)
    assert isinstance(dec.decoder_blocks[5], blocks.LastUnaryBlock)
    assert dec.encoder_skips == [2, 5, 8, 11] and dec.encoder_skip_dims == [256, 512, 1024, 2048]
    assert dec.decoder_concats == [1, 3, 5]
    assert not hasattr(dec, "bottle") and not hasattr(dec, "gnn") and not hasattr(dec, "proj_gnn")
    no_grad = [n for n, p in dec.named_parameters() if not p.requires_grad]
    assert no_grad == [n for n, _ in dec.named_parameters() if n.endswith("kernel_points")] and len(no_grad) == 11


def test_modelnet_block_list_builds():
    np.random.seed(0)
    torch.manual_seed(0)
    dec = KPFCNNDecoder(_symmetric_config(architecture=architectures['modelnet']))
    assert len(dec.encoder_blocks) == 9 and len(dec.decoder_blocks) == 6
    assert dec.decoder_concats == [1, 4] and dec.encoder_skips == [3, 6, 9]
    assert tuple(dec.state_dict()["decoder_blocks.5.mlp.weight"].shape)[0] == 12
