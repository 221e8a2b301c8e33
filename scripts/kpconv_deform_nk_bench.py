"""Deformed KPConv correlation (modulated, linear influence, sum aggregation) per level of the KITTI pyramid -- the layer sizes of
DESIGN sections 31 / 38: mid widths 64, 128, 256, 512 on the synthetic KITTI pair of scripts/kpconv_bench.py -- at K = 7, 15,
16, 17, 25 kernel points (the environment variables KP_BENCH_KS / KP_BENCH_LEVELS choose a subset), given the query's own
kernel points dkp [N, K, 3] and modulations mod [N, K] (what offset_conv hands over; offset_conv itself is a rigid layer,
scripts/kpconv_nk_bench.py):

    nk      forward: apr_row_sums + apr_kpconv_deform_weighted_nk + the dense GEMM over [N, K c]; forward + backward:
            kp_ops.KPConvDeformFunction (d x, d W, d dkp, d mod) on the *_nk entries            (csrc/kpconv_deform_nk.hip)
    k15     at K = 15 only: the same on the apr_kpconv_deform_*_mode entries (csrc/kpconv_deform.hip), next to `nk`
    torch   the route such a layer took before the *_nk kernels: the module's torch formulation
            (KPConv._forward_autograd_deformable on the same device), forward under no_grad and forward + backward

All legs warmed, alternated in ONE process, every window at least MIN_WINDOW seconds of device time between two events,
ALTERNATIONS alternations: median and spread (max - min) of the per-call times in microseconds; peak device memory of one
forward + backward of either route above what is resident before it.  One JSON line at the end (DESIGN section 40 quotes it)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from apr_amd import _lib, synth
from apr_amd.predator import kp_ops, point_ops
from apr_amd.predator.configs.models import kitti_config
from apr_amd.predator.datasets.dataloader import collate_fn_descriptor
from apr_amd.predator.kernels import kernel_points as KP
from apr_amd.predator.models import blocks
from bench_predator import LIMITS

MIN_WINDOW, ALTERNATIONS = 0.1, 3
KS = tuple(int(v) for v in os.environ.get("KP_BENCH_KS", "7,15,16,17,25").split(","))
LEVELS = tuple(int(v) for v in os.environ.get("KP_BENCH_LEVELS", "0,1,2,3").split(","))
dev = torch.device("cuda:0")
cfg = kitti_config()
a, b, _ = synth.make_pair(0)
pts, lens = point_ops.grid_subsample(torch.cat([torch.from_numpy(a), torch.from_numpy(b)]).to(dev),
                                     np.array([len(a), len(b)], np.int32), 0.3)
src, tgt = pts[:lens[0]], pts[lens[0]:]
ones = lambda p: torch.ones((len(p), 1), device=dev)
batch = collate_fn_descriptor([(src, tgt, ones(src), ones(tgt))], cfg, LIMITS)
rng = np.random.default_rng(0)
for K in KS:
    if K != 15:      # random points of the ball: a made disposition costs host time and does not change what is timed
        d = rng.standard_normal((K, 3))
        d *= (0.66 * rng.uniform(0.5, 1.0, (K, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
        d[0] = 0.0
        KP.set_disposition(K, "center", d)
lib = _lib.load()
real_load = _lib.load


class NkAt15:
    """the library with the 15-point deformable entries answered by the *_nk ones: times `nk` at K = 15 through the same
    autograd function"""
    SWAP = {f"apr_kpconv_deform_{n}_mode": f"apr_kpconv_deform_{n}_nk" for n in ("weighted", "dfeat_contrib", "dgeom")}

    def __getattr__(self, name):
        return getattr(lib, self.SWAP.get(name, name))


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps       # us per call


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


rows = []
for level, c in [(lv, 64 << lv) for lv in LEVELS]:
    P, nbr = batch['points'][level], batch['neighbors'][level]
    N, H = nbr.shape
    radius = cfg.first_subsampling_dl * cfg.conv_radius * 2 ** level
    extent = radius * cfg.KP_extent / cfg.conv_radius
    x = torch.randn(N, c, device=dev).abs()
    dout = torch.randn(N, c, device=dev)
    for K in KS:
        torch.manual_seed(level)
        np.random.seed(level)
        conv = blocks.KPConv(K, 3, c, c, extent, radius, deformable=True, modulated=True).to(dev)
        dkp = (conv.kernel_points[None] + 0.1 * extent * torch.randn(N, K, 3, device=dev)).contiguous()
        mod = (2 * torch.sigmoid(torch.randn(N, K, device=dev))).contiguous()
        wf = torch.empty((N, K * c), dtype=torch.float32, device=dev)
        assert kp_ops.deform_ok(x, c, H, K)

        def step1(entry):
            def run():
                rs = kp_ops.row_sums(x)
                _lib.check(entry(_lib.ptr(P), N, _lib.ptr(P), N, _lib.ptr(nbr), H, _lib.ptr(x), c, c, _lib.ptr(dkp), _lib.ptr(mod), K,
                                 float(extent), _lib.ptr(rs), _lib.ptr(wf), K * c, None, 1, 0, _lib.stream()))
                return kp_ops.linear(wf, conv._weight())
            return run

        def torch_fwd():
            with torch.no_grad():
                return conv._forward_autograd_deformable(P, P, nbr, x, dkp, mod)

        def leaves():
            conv.zero_grad(set_to_none=True)
            return x.detach().requires_grad_(True), dkp.detach().requires_grad_(True), mod.detach().requires_grad_(True)

        def hip_fwdbwd(handle):
            def run():
                _lib.load = kp_ops._lib.load = handle
                try:
                    xx, kk, mm = leaves()
                    y, _ = kp_ops.KPConvDeformFunction.apply(P, P, nbr, xx, conv.weights, kk, mm, extent)
                    y.backward(dout)
                finally:
                    _lib.load = kp_ops._lib.load = real_load
                return xx.grad, conv.weights.grad, kk.grad, mm.grad
            return run

        def torch_fwdbwd():
            xx, kk, mm = leaves()
            conv._forward_autograd_deformable(P, P, nbr, xx, kk, mm).backward(dout)
            return xx.grad, conv.weights.grad, kk.grad, mm.grad

        proxy = NkAt15()
        legs = {"nk_fwd": step1(lib.apr_kpconv_deform_weighted_nk), "torch_fwd": torch_fwd,
                "nk_fwdbwd": hip_fwdbwd((lambda: proxy) if K == 15 else real_load), "torch_fwdbwd": torch_fwdbwd}
        if K == 15:
            legs["k15_fwd"] = step1(lib.apr_kpconv_deform_weighted_mode)
            legs["k15_fwdbwd"] = hip_fwdbwd(real_load)
        rel = lambda g, r: float(((g - r).flatten(1).norm(dim=1) / torch.clamp(r.flatten(1).norm(dim=1), min=float(
            r.flatten(1).norm(dim=1).median()))).max())
        diff = rel(legs["nk_fwd"](), torch_fwd())
        # per gradient: d_dkp alone is discontinuous in the geometry (a neighbour crossing the edge of a ball switches a whole
        # term diff / (d extent) P on or off), so among millions of triples a float32 decision at the edge shows there only
        gdiff = {n: rel(g, r) for n, g, r in zip(("d_x", "d_W", "d_dkp", "d_mod"), legs["nk_fwdbwd"](),
                                                 [t.clone() for t in torch_fwdbwd()])}
        mem = {"nk": peak_mb(legs["nk_fwdbwd"]), "torch": peak_mb(torch_fwdbwd)}
        reps = {}
        for name, fn in legs.items():
            for _ in range(2):
                fn()
            reps[name] = max(2, int(MIN_WINDOW * 1e6 / window(fn, 2)) + 1)
        t = {name: [] for name in legs}
        for _ in range(ALTERNATIONS):
            for name, fn in legs.items():
                t[name].append(window(fn, reps[name]))
        med = {k: round(statistics.median(v), 1) for k, v in t.items()}
        spread = {k: round(max(v) - min(v), 1) for k, v in t.items()}
        rows.append(dict(level=level, N=N, H=H, c=c, K=K, us=med, spread_us=spread, nk_vs_torch_rows_rel_l2=diff,
                         nk_vs_torch_grads_rows_rel_l2=gdiff, peak_fwdbwd_mb=mem))
        print(f"level {level} N={N} H={H} c={c} K={K}: " + "  ".join(f"{k} {med[k]:.1f} (+-{spread[k]:.1f})" for k in legs) +
              f"  peak MB nk {mem['nk']} torch {mem['torch']}  nk vs torch rows rel-L2 fwd {diff:.2e} grads " +
              " ".join(f"{k} {v:.2e}" for k, v in gdiff.items()), flush=True)
        del conv, dkp, mod, wf
        torch.cuda.empty_cache()
print(json.dumps(rows))
