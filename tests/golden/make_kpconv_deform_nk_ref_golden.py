"""Generates tests/golden/kpconv_deform_nk_ref.npz with the REFERENCE itself (build container only; needs /root/reference):
    python tests/golden/make_kpconv_deform_nk_ref_golden.py

By the method of make_kpconv_deform_ref_golden.py:
  * imports /root/reference/Predator_APR/models/blocks.py as it is (cwd = a temp dir, in which the reference makes and keeps
    the kernel dispositions it does not ship: `kernels/dispositions/k_007_center_3D.ply`, `k_020_none_3D.ply`),
  * k7_center/m{0,1}/..., k20_none/m{0,1}/...: KPConv(K, 3, 8, 8, extent 1.2, radius 1.5, fixed_kernel_points,
    deformable=True, modulated=False / True) built under np.random.seed(1) / torch.manual_seed(1): its float32 state_dict,
    then the module cast to float64 on the seeded inputs of that script: out, min_d2, deformed_KP, offset_features and the
    gradients of sum(out * G) with respect to x, weights, offset_conv.weights and offset_bias (offset_bias is drawn non-zero
    first, so the bias path is exercised).
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
LAYERS = ((7, "center"), (20, "none"))


def in_reference(fn):
    tmp = tempfile.mkdtemp()
    cwd = os.getcwd()
    os.chdir(tmp)
    sys.path.insert(0, REF)
    try:
        return fn()
    finally:
        os.chdir(cwd)
        sys.path.remove(REF)
        shutil.rmtree(tmp, ignore_errors=True)


def module_inputs():
    rng = np.random.default_rng(7)
    ns, nq, H, cin, cout = 40, 25, 12, 8, 8
    s = rng.uniform(-1.5, 1.5, (ns, 3)).astype(np.float32)
    q = s[:nq] + rng.uniform(-0.2, 0.2, (nq, 3)).astype(np.float32)
    nbr = rng.integers(0, ns + 1, (nq, H)).astype(np.int64)
    nbr[3] = ns                                              # a row of padding: nothing in range, an all-zero output row
    x = rng.standard_normal((ns, cin)).astype(np.float32) + np.float32(0.3)
    G = rng.standard_normal((nq, cout)).astype(np.float32)
    b = (rng.standard_normal(4 * 20) * 0.1).astype(np.float32)
    return dict(s=s, q=q, nbr=nbr, x=x, G=G, bias=b)


def module_fixture(out):
    def run():
        from models import blocks as RB
        inp = module_inputs()
        out.update({f"in/{k}": v for k, v in inp.items()})
        for K, fixed in LAYERS:
            for m in (0, 1):
                p = f"k{K}_{fixed}/m{m}"
                np.random.seed(1)
                torch.manual_seed(1)
                conv = RB.KPConv(K, 3, 8, 8, 1.2, 1.5, fixed_kernel_points=fixed, deformable=True, modulated=bool(m))
                assert conv.offset_dim == (4 if m else 3) * K
                for k, v in conv.state_dict().items():
                    out[f"{p}/sd/{k}"] = v.numpy().copy()
                conv = conv.double()
                with torch.no_grad():
                    conv.offset_bias.copy_(torch.from_numpy(inp["bias"][:conv.offset_dim].astype(np.float64)))
                t = lambda a: torch.from_numpy(a.astype(np.float64))
                x = t(inp["x"]).requires_grad_(True)
                y = conv(t(inp["q"]), t(inp["s"]), torch.from_numpy(inp["nbr"]), x)
                (y * t(inp["G"])).sum().backward()
                assert torch.isfinite(y).all() and not y[3].any()
                out[f"{p}/out"] = y.detach().numpy()
                out[f"{p}/min_d2"] = conv.min_d2.detach().numpy()
                out[f"{p}/deformed_KP"] = conv.deformed_KP.detach().numpy()
                out[f"{p}/offset_features"] = conv.offset_features.detach().numpy()
                out[f"{p}/d_x"] = x.grad.numpy()
                out[f"{p}/d_weights"] = conv.weights.grad.numpy()
                out[f"{p}/d_offset_conv_weights"] = conv.offset_conv.weights.grad.numpy()
                out[f"{p}/d_offset_bias"] = conv.offset_bias.grad.numpy()
                for k in ("d_x", "d_weights", "d_offset_conv_weights", "d_offset_bias"):
                    assert np.isfinite(out[f"{p}/{k}"]).all(), k
    in_reference(run)


def main():
    out = {}
    module_fixture(out)
    path = os.path.join(HERE, "kpconv_deform_nk_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e6:.3f} MB, {len(out)} arrays")


if __name__ == "__main__":
    main()
