"""Generates tests/golden/kpconv_modes_ref.npz with the REFERENCE itself (build container only; needs /root/reference):
    python tests/golden/make_kpconv_modes_ref_golden.py

  * imports /root/reference/Predator_APR/models/blocks.py as it is (cwd = a temp dir holding a copy of the
    kernel-disposition .ply, as make_kpconv_deform_ref_golden.py does),
  * for the five (KP_influence, aggregation_mode) pairs other than (linear, sum) and the three kinds of layer -- r: rigid,
    d: deformable, dm: deformable + modulated -- builds KPConv(15, 3, 8, 8, extent 1.2, radius 1.5, ...) under
    np.random.seed(1) / torch.manual_seed(1) and stores under `<influence>-<aggregation>/<kind>/`: its float32 state_dict
    (sd/...), then, with the module cast to float64 on the seeded inputs of in/...: out, and for the deformable kinds min_d2,
    deformed_KP, offset_features (offset_bias is drawn non-zero first), and the gradients of sum(out * G) with respect to x,
    weights, offset_conv.weights and offset_bias.  Where the reference's graph gives None (the constant influence moves no
    kernel point) zeros are stored and none/<name> = 1.  Where the reference's own backward raises (gaussian + closest on a
    deformable layer: its in-place product with the one-hot overwrites what exp's backward needs) no_backward = 1 and no
    gradient is stored.
Only arrays are stored.
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/Predator_APR"
PAIRS = [("constant", "sum"), ("constant", "closest"), ("linear", "closest"), ("gaussian", "sum"), ("gaussian", "closest")]
KINDS = {"r": (False, False), "d": (True, False), "dm": (True, True)}


def in_reference(fn):
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "kernels", "dispositions"))
    shutil.copy(os.path.join(REF, "kernels/dispositions/k_015_center_3D.ply"), os.path.join(tmp, "kernels", "dispositions"))
    cwd = os.getcwd()
    os.chdir(tmp)
    sys.path.insert(0, REF)
    try:
        return fn()
    finally:
        os.chdir(cwd)
        sys.path.remove(REF)


def module_inputs():
    rng = np.random.default_rng(11)
    ns, nq, H, cin, cout = 40, 25, 12, 8, 8
    s = rng.uniform(-1.5, 1.5, (ns, 3)).astype(np.float32)
    q = s[:nq] + rng.uniform(-0.2, 0.2, (nq, 3)).astype(np.float32)
    nbr = rng.integers(0, ns + 1, (nq, H)).astype(np.int64)
    nbr[3] = ns                                              # a row of padding: an all-zero output row in every mode
    x = rng.standard_normal((ns, cin)).astype(np.float32) + np.float32(0.3)
    G = rng.standard_normal((nq, cout)).astype(np.float32)
    b = (rng.standard_normal(60) * 0.1).astype(np.float32)
    return dict(s=s, q=q, nbr=nbr, x=x, G=G, bias=b)


def main():
    out = {}

    def run():
        from models import blocks as RB
        inp = module_inputs()
        out.update({f"in/{k}": v for k, v in inp.items()})
        t = lambda a: torch.from_numpy(a.astype(np.float64))
        for inf, agg in PAIRS:
            for kind, (deformable, modulated) in KINDS.items():
                p = f"{inf}-{agg}/{kind}"
                np.random.seed(1)
                torch.manual_seed(1)
                conv = RB.KPConv(15, 3, 8, 8, 1.2, 1.5, KP_influence=inf, aggregation_mode=agg, deformable=deformable,
                                 modulated=modulated)
                for k, v in conv.state_dict().items():
                    out[f"{p}/sd/{k}"] = v.numpy().copy()
                conv = conv.double()
                if deformable:
                    with torch.no_grad():
                        conv.offset_bias.copy_(torch.from_numpy(inp["bias"][:conv.offset_dim].astype(np.float64)))
                x = t(inp["x"]).requires_grad_(True)
                y = conv(t(inp["q"]), t(inp["s"]), torch.from_numpy(inp["nbr"]), x)
                assert torch.isfinite(y).all() and not y[3].any()
                out[f"{p}/out"] = y.detach().numpy()
                try:
                    (y * t(inp["G"])).sum().backward()
                    out[f"{p}/no_backward"] = np.array(0)
                except RuntimeError as e:      # the reference multiplies exp's output by the one-hot IN PLACE (blocks.py:342)
                    assert "inplace" in str(e), e
                    out[f"{p}/no_backward"] = np.array(1)
                    print(p, "the reference's own backward fails:", str(e)[:90])
                grads = dict(d_x=(x.grad, x), d_weights=(conv.weights.grad, conv.weights))
                if deformable:
                    out[f"{p}/min_d2"] = conv.min_d2.detach().numpy()
                    out[f"{p}/deformed_KP"] = conv.deformed_KP.detach().numpy()
                    out[f"{p}/offset_features"] = conv.offset_features.detach().numpy()
                    grads.update(d_offset_conv_weights=(conv.offset_conv.weights.grad, conv.offset_conv.weights),
                                 d_offset_bias=(conv.offset_bias.grad, conv.offset_bias))
                if out[f"{p}/no_backward"]:
                    grads = {}
                for k, (gr, like) in grads.items():
                    out[f"{p}/none/{k}"] = np.array(int(gr is None))
                    out[f"{p}/{k}"] = np.zeros(tuple(like.shape)) if gr is None else gr.numpy().copy()
                    assert np.isfinite(out[f"{p}/{k}"]).all(), (p, k)
                print(p, "None gradients:", [k for k in grads if out[f"{p}/none/{k}"]])
    in_reference(run)
    path = os.path.join(HERE, "kpconv_modes_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays")


if __name__ == "__main__":
    main()
