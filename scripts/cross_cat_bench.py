"""One 'cross_cat' layer of the overlap-attention module (AttentionalPropagationCat, C = 256, 4 heads) at the size of KITTI's
coarsest level, n = m = 1400, against two alternatives on the same weights and inputs:

    cat        the layer as the module runs it: inference = projections head-major, apr_mha_cat_headmajor (fp32 MFMA, the
               coordinate columns beside the value columns), merge on the padded rows; training = apr_mha_cat_train_forward /
               _backward (MHACatFunction)
    composed   the same layer from what the library offered before: value and coordinates concatenated per head,
               apr_mha_train_forward / _backward with vdim = dim + 3 (MHAFunction), torch ops for aug1 / aug2 and the row layout
    cross      the plain 'cross' layer (AttentionalPropagation) of the same width: what the geometry costs on top

forward (no_grad: the inference route), the training path's forward alone (grad enabled, no backward) and forward + backward;
"backward" is the difference of the last two medians.  All legs warmed and alternated in ONE process; RUNS windows per leg
between two events, each of REPS calls: median and spread (max - min) of the per-call times in microseconds.  One JSON line at
the end (DESIGN section 37 quotes it)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from apr_amd.predator import kp_ops
from apr_amd.predator.models import gcn

N = M = int(os.environ.get("CROSS_CAT_BENCH_N", "1400"))
C, HEADS, RUNS, REPS = 256, 4, 21, 5
dev = torch.device("cuda:0")
torch.manual_seed(0)
cat = gcn.AttentionalPropagationCat(C, HEADS).to(dev)
cross = gcn.AttentionalPropagation(C, HEADS).to(dev)
x0, x1 = torch.randn(N, C, device=dev), torch.randn(M, C, device=dev)
c0, c1 = (torch.rand(N, 3, device=dev) - 0.5) * 160, (torch.rand(M, 3, device=dev) - 0.5) * 160
dout = torch.randn(N, C, device=dev)
_cache = [gcn._Packed() for _ in range(6)]


def composed(f0, f1):
    at = cat.attn
    n, m, dim = f0.shape[0], f1.shape[0], at.dim
    q, k, v = [gcn.conv1x1(x, l, c) for l, x, c in zip(at.proj, (f0, f1, f1), _cache[:3])]
    vc = torch.cat([v.view(m, dim, HEADS), c1[:, :, None].expand(m, 3, HEADS)], dim=1).reshape(m, -1)
    o = kp_ops.MHAFunction.apply(q, k, vc, HEADS).view(n, dim + 3, HEADS)
    aug1 = o[:, dim:] - c0[:, :, None]
    y = torch.cat([o, aug1, torch.norm(aug1, dim=1, keepdim=True)], dim=1).reshape(n, -1)
    message = gcn.conv1x1(y, at.merge, _cache[3])
    h = gcn.conv1x1(torch.cat([f0, message], dim=1), cat.mlp[0], _cache[4])
    h = kp_ops.instance_norm_act(h, eps=cat.mlp[1].eps, relu=True)
    return gcn.conv1x1(h, cat.mlp[3], _cache[5])


def forward(fn):
    def run():
        with torch.no_grad():
            return fn(x0, x1)
    return run


def fwdbwd(fn, params, backward=True):
    def run():
        for p in params:
            p.grad = None
        a, b = x0.detach().requires_grad_(True), x1.detach().requires_grad_(True)
        out = fn(a, b)
        if not backward:
            return out
        out.backward(dout)
        return a.grad
    return run


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps       # us per call


cat_fn = lambda a, b: cat(a, b, c0, c1)
fns = {"cat": (cat_fn, list(cat.parameters())), "composed": (composed, list(cat.parameters())), "cross": (cross, list(cross.parameters()))}
legs = {f"{name}_fwd": forward(fn) for name, (fn, _) in fns.items()}
legs.update({f"{name}_trainfwd": fwdbwd(fn, params, backward=False) for name, (fn, params) in fns.items()})
legs.update({f"{name}_fwdbwd": fwdbwd(fn, params) for name, (fn, params) in fns.items()})
ref, got = legs["composed_fwd"](), legs["cat_fwd"]()
route = cat.attn.last_route
diff = float((got - ref).norm() / ref.norm())
gdiff = float((legs["cat_fwdbwd"]() - legs["composed_fwdbwd"]()).norm() / legs["composed_fwdbwd"]().norm())
for fn in legs.values():
    for _ in range(3):
        fn()
t = {name: [] for name in legs}
for _ in range(RUNS):
    for name, fn in legs.items():
        t[name].append(window(fn, REPS))
med = {k: round(statistics.median(v), 1) for k, v in t.items()}
spread = {k: round(max(v) - min(v), 1) for k, v in t.items()}
for name in ("cat", "composed", "cross"):
    print(f"{name:9s} forward {med[name + '_fwd']:8.1f} us (+-{spread[name + '_fwd']:.1f})   training forward "
          f"{med[name + '_trainfwd']:8.1f} us (+-{spread[name + '_trainfwd']:.1f})   forward + backward "
          f"{med[name + '_fwdbwd']:8.1f} us (+-{spread[name + '_fwdbwd']:.1f})   backward "
          f"{med[name + '_fwdbwd'] - med[name + '_trainfwd']:8.1f} us", flush=True)
print(json.dumps(dict(n=N, m=M, c=C, heads=HEADS, runs=RUNS, reps=REPS, inference_route=route, us=med, spread_us=spread,
                      cat_vs_composed_fwd_rel_l2=diff, cat_vs_composed_dx_rel_l2=gdiff)))
