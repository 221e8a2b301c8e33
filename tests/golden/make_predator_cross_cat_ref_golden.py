"""Generates tests/golden/predator_cross_cat_ref.npz with the REFERENCE itself (build container only).

Imports /root/reference/Predator_APR/models/gcn.py the way make_predator_golden.py imports architectures.py (the reference's
root on sys.path) and stores ARRAYS ONLY:

(a) GCN(4, 64, 10, ['cross_cat']) built under torch.manual_seed(SEED_A), evaluated in float64 on n = 37, m = 23:
    a_sd/<key>      the full state_dict (float32: the values the float64 copy holds exactly), attn.distribute.* and
                    attn.proj.0.* both present as the reference has them
    a_c0, a_c1      coordinates [n, 3], [m, 3] (float32, within +-80);  a_x0, a_x1 descriptors [n, 64], [m, 64] (float32)
    a_o0, a_o1      both outputs as rows (float64)
    a_gx0, a_gx1    d loss / d descriptors for loss = o0.sum() + (o1 ** 2).sum() (float64)
    a_g/<name>      d loss / d parameter for every name of named_parameters() (float32 roundings of the float64 values:
                    6e-8 relative, four orders below the 1e-4 the tests hold)
    a_f32/<what>    the same run in float32 on the CPU: rel-L2 against the float64 values, one number per output and gradient
(b) GCN(4, 256, 10, ['self', 'cross_cat', 'self']) built under torch.manual_seed(SEED_B), float64 on n = 150, m = 130:
    b_seed; b_keys, b_sum, b_sumsq   per-tensor float64 sum and sum of squares of the state_dict (not the weights)
    b_c0, b_c1; b_x0q, b_x1q         coordinates; descriptors as int16 multiples of 1 / 1024 (exact in float32)
    b_o0, b_o1                       outputs (float32 roundings of the float64 values)
    b_f32/o0, b_f32/o1               the same run in float32 on the CPU: rel-L2 against the float64 outputs
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/Predator_APR"
SEED_A, SEED_B = 11, 12


def reference_gcn():
    sys.path.insert(0, REF)
    try:
        from models.gcn import GCN
    finally:
        sys.path.remove(REF)
    return GCN


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def run(model, c0, c1, x0, x1, grad):
    """rows in, rows out: the reference wants [1, C, N]"""
    x0 = x0.clone().requires_grad_(grad)
    x1 = x1.clone().requires_grad_(grad)
    o0, o1 = model(c0.t()[None], c1.t()[None], x0.t()[None], x1.t()[None])
    o0, o1 = o0[0].t(), o1[0].t()
    if not grad:
        return o0.detach(), o1.detach()
    model.zero_grad()
    (o0.sum() + (o1 ** 2).sum()).backward()
    return o0.detach(), o1.detach(), x0.grad, x1.grad, {k: p.grad.clone() for k, p in model.named_parameters()}


def main():
    GCN = reference_gcn()
    out = {}
    rng = np.random.default_rng(2024)
    # (a)
    torch.manual_seed(SEED_A)
    m32 = GCN(4, 64, 10, ['cross_cat'])
    n, m = 37, 23
    c0 = torch.from_numpy(rng.uniform(-80, 80, (n, 3)).astype(np.float32))
    c1 = torch.from_numpy(rng.uniform(-80, 80, (m, 3)).astype(np.float32))
    x0 = torch.from_numpy(rng.standard_normal((n, 64)).astype(np.float32))
    x1 = torch.from_numpy(rng.standard_normal((m, 64)).astype(np.float32))
    sd = m32.state_dict()
    assert "layers.0.attn.distribute.weight" in sd and "layers.0.attn.proj.0.weight" in sd
    for k, v in sd.items():
        out["a_sd/" + k] = v.numpy().copy()
    import copy
    m64 = copy.deepcopy(m32).double()
    o0, o1, gx0, gx1, g = run(m64, c0.double(), c1.double(), x0.double(), x1.double(), True)
    p0, p1, hx0, hx1, h = run(m32, c0, c1, x0, x1, True)
    out.update(a_c0=c0.numpy(), a_c1=c1.numpy(), a_x0=x0.numpy(), a_x1=x1.numpy(), a_o0=o0.numpy(), a_o1=o1.numpy(),
               a_gx0=gx0.numpy(), a_gx1=gx1.numpy())
    f32 = {"o0": rel(p0, o0), "o1": rel(p1, o1), "gx0": rel(hx0, gx0), "gx1": rel(hx1, gx1)}
    for k in g:
        out["a_g/" + k] = g[k].numpy().astype(np.float32)
        f32["g/" + k] = rel(h[k], g[k])
    for k, v in f32.items():
        out["a_f32/" + k] = np.float64(v)
    print("(a) float32 rel-L2:", {k: f"{v:.2e}" for k, v in f32.items()})
    # (b)
    torch.manual_seed(SEED_B)
    mb = GCN(4, 256, 10, ['self', 'cross_cat', 'self'])
    sdb = mb.state_dict()
    out["b_seed"] = np.int64(SEED_B)
    out["b_keys"] = np.array(list(sdb.keys()))
    out["b_sum"] = np.array([float(v.double().sum()) for v in sdb.values()])
    out["b_sumsq"] = np.array([float((v.double() ** 2).sum()) for v in sdb.values()])
    n, m = 150, 130
    c0 = rng.uniform(-80, 80, (n, 3)).astype(np.float32)
    c1 = rng.uniform(-80, 80, (m, 3)).astype(np.float32)
    x0q = np.clip(np.rint(rng.standard_normal((n, 256)) * 1024), -32000, 32000).astype(np.int16)
    x1q = np.clip(np.rint(rng.standard_normal((m, 256)) * 1024), -32000, 32000).astype(np.int16)
    mb = mb.eval()
    with torch.no_grad():
        p0, p1 = run(mb, torch.from_numpy(c0), torch.from_numpy(c1), torch.from_numpy(x0q).float() / 1024,
                     torch.from_numpy(x1q).float() / 1024, False)
        mb = mb.double()
        o0, o1 = run(mb, torch.from_numpy(c0).double(), torch.from_numpy(c1).double(), torch.from_numpy(x0q).double() / 1024,
                     torch.from_numpy(x1q).double() / 1024, False)
    out["b_f32/o0"], out["b_f32/o1"] = np.float64(rel(p0, o0)), np.float64(rel(p1, o1))
    print("(b) float32 rel-L2:", float(out["b_f32/o0"]), float(out["b_f32/o1"]))
    out.update(b_c0=c0, b_c1=c1, b_x0q=x0q, b_x1q=x1q, b_o0=o0.numpy().astype(np.float32), b_o1=o1.numpy().astype(np.float32))
    path = os.path.join(HERE, "predator_cross_cat_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
