"""Generates tests/golden/predator_decoder_ref.npz with the REFERENCE itself (build container only).

  * imports /root/reference/Predator_APR/models/architectures.py:KPFCNN and KPFCNNDecoder the way make_predator_golden.py
    does (cwd = a temp dir holding a copy of the kernel-disposition .ply), builds them in main.py's order (:52-63: KPFCNN with
    switch_to_decoder = False, then the decoder with switch_to_decoder = True) under np.random.seed(0) / torch.manual_seed(0),
  * runs the pair tests/predator_loss_fixture.small_pair() collated by oracle/kpfcnn_oracle.collate with limits
    [30, 30, 30, 30]: encoder in train() -> `second_features`; decoder in train() -> [N0, 12]; loss = sum(out * G) with a
    seeded G; backward,
  * stores ARRAYS ONLY (second_features in predator_decoder_ref_features.npz, the rest in predator_decoder_ref.npz: one
    file would pass the size limit of a committed file): the pair, second_features, the output, G, the full gradients of
    encoder_blocks.0.KPConv.weights and decoder_blocks.5.mlp.weight, the L2 norm of every parameter gradient, both key lists, the decoder's shapes and both
    absolute weight sums (the 24 M parameters themselves do not fit a fixture: apr_amd's models built under the same seeds
    hold them bit for bit, which the key lists and the sums pin).
It asserts that no pre-normalisation row has norm below 1e-6 (F.normalize's clamp stays out of the comparison) and that
`epsilon` and the kernel points are the only parameters without a gradient.
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/Predator_APR"
sys.path.insert(0, ROOT)

from apr_amd.predator.configs.models import kitti_config  # noqa: E402
from oracle import kpfcnn_oracle as KO  # noqa: E402
from tests.predator_loss_fixture import small_pair  # noqa: E402

LIMITS = [30, 30, 30, 30]


def reference_models():
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "kernels", "dispositions"))
    shutil.copy(os.path.join(REF, "kernels/dispositions/k_015_center_3D.ply"),
                os.path.join(tmp, "kernels", "dispositions"))
    cwd = os.getcwd()
    os.chdir(tmp)
    sys.path.insert(0, REF)
    try:
        from models.architectures import KPFCNN, KPFCNNDecoder
        np.random.seed(0)
        torch.manual_seed(0)
        cfg = kitti_config(symmetric=True, switch_to_decoder=False)
        enc = KPFCNN(cfg)
        cfg.switch_to_decoder = True
        dec = KPFCNNDecoder(cfg)
    finally:
        os.chdir(cwd)
        sys.path.remove(REF)
    return enc, dec, cfg


def main():
    enc, dec, cfg = reference_models()
    pair = small_pair()
    batch = KO.collate(pair["src"], pair["tgt"], cfg, LIMITS)
    enc.train()
    dec.train()
    feats, _, _ = enc(batch)
    batch["second_features"] = feats
    seen = {}
    hook = dec.decoder_blocks[-1].register_forward_hook(lambda m, i, o: seen.__setitem__("raw", o.detach()))
    out = dec(batch)
    hook.remove()
    norms = seen["raw"].norm(dim=1)
    print("pre-normalisation row norms: min", float(norms.min()), "max", float(norms.max()))
    assert float(norms.min()) >= 1e-6, "F.normalize's clamp would enter the comparison"
    n0 = len(pair["src"]) + len(pair["tgt"])
    assert tuple(out.shape) == (n0, cfg.point_generation_ratio * 3)
    G = torch.from_numpy(np.random.default_rng(0).standard_normal(tuple(out.shape)).astype(np.float32))
    (out * G).sum().backward()
    assert all(p.grad is None for p in enc.parameters()), "the detach cuts the generator off from the encoder"
    no_grad = [n for n, p in dec.named_parameters() if p.grad is None]
    assert no_grad == ["epsilon"] + [n for n, _ in dec.named_parameters() if n.endswith("kernel_points")], no_grad
    names = [n for n, p in dec.named_parameters() if p.grad is not None]
    arrays = dict(
        src=pair["src"], tgt=pair["tgt"], limits=np.array(LIMITS),
        out=out.detach().numpy(), G=G.numpy(),
        grad_first_kpconv=dec.encoder_blocks[0].KPConv.weights.grad.numpy(),
        grad_last_unary=dec.decoder_blocks[5].mlp.weight.grad.numpy(),
        grad_names=np.array(names), grad_norms=np.array([float(dict(dec.named_parameters())[n].grad.norm()) for n in names]),
        dec_keys=np.array(list(dec.state_dict().keys())), enc_keys=np.array(list(enc.state_dict().keys())),
        dec_weight_abs_sum=float(sum(v.double().abs().sum() for v in dec.state_dict().values())),
        enc_weight_abs_sum=float(sum(v.double().abs().sum() for v in enc.state_dict().values())),
        dec_shapes=np.array([str(tuple(v.shape)) for v in dec.state_dict().values()]),
        level_sizes=np.array([len(p) for p in batch['points']]))
    np.savez_compressed(os.path.join(HERE, "predator_decoder_ref.npz"), **arrays)
    # a file of its own: with the [N0, 32] descriptors inside, the fixture would pass the size limit of a committed file
    np.savez_compressed(os.path.join(HERE, "predator_decoder_ref_features.npz"), second_features=feats.detach().numpy())
    print("levels", [len(p) for p in batch['points']], "decoder keys", len(dec.state_dict()),
          "parameters", sum(p.numel() for p in dec.parameters()), "wrote predator_decoder_ref.npz")


if __name__ == "__main__":
    main()
