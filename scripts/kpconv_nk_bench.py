"""Rigid KPConv forward (row sums + step 1 + GEMM) per level of the KITTI pyramid -- the layer sizes of DESIGN section 31: mid
widths 64, 128, 256, 512 on the synthetic KITTI pair of scripts/kpconv_bench.py -- at K = 7, 15, 16, 17, 25 kernel points:

    nk      apr_row_sums + apr_kpconv_weighted_nk + the dense GEMM over [N, K c]          (csrc/kpconv_nk.hip)
    k15     at K = 15 only: the same with apr_kpconv_weighted_mode (csrc/kpconv.hip), next to `nk`
    torch   the module's torch formulation (blocks.KPCONV_NK_HIP = False: _forward_autograd on the same device)

All legs warmed, alternated in ONE process, every window at least MIN_WINDOW seconds of device time between two events,
ALTERNATIONS alternations: median and spread (max - min) of the per-call times in microseconds.  The kernel points are random
points of the ball (a made disposition costs up to half a minute of host time at K = 25 and does not change what is timed).
One JSON line at the end (DESIGN section 38 quotes it)."""
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
KS = (7, 15, 16, 17, 25)
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
    if K != 15:
        d = rng.standard_normal((K, 3))
        d *= (0.66 * rng.uniform(0.5, 1.0, (K, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
        d[0] = 0.0
        KP.set_disposition(K, "center", d)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps       # us per call


rows = []
lib = _lib.load()
for level, c in ((0, 64), (1, 128), (2, 256), (3, 512)):
    P, nbr = batch['points'][level], batch['neighbors'][level]
    N, H = nbr.shape
    radius = cfg.first_subsampling_dl * cfg.conv_radius * 2 ** level
    extent = radius * cfg.KP_extent / cfg.conv_radius
    x = torch.randn(N, c, device=dev).abs()
    for K in KS:
        torch.manual_seed(level)
        np.random.seed(level)
        conv = blocks.KPConv(K, 3, c, c, extent, radius).to(dev)
        kpts = conv.kernel_points.contiguous()
        wf = torch.empty((N, K * c), dtype=torch.float32, device=dev)

        def step1(entry):
            def run():
                rs = kp_ops.row_sums(x)
                _lib.check(entry(_lib.ptr(P), N, _lib.ptr(P), N, _lib.ptr(nbr), H, _lib.ptr(x), c, c, _lib.ptr(kpts), K, float(extent),
                                 _lib.ptr(rs), _lib.ptr(wf), K * c, 1, 0, _lib.stream()))
                return kp_ops.linear(wf, conv._weight())
            return run

        def torch_fwd():
            with torch.no_grad():
                return conv._forward_autograd(P, P, nbr, x)

        legs = {"nk": step1(lib.apr_kpconv_weighted_nk), "torch": torch_fwd}
        if K == 15:
            legs["k15"] = step1(lib.apr_kpconv_weighted_mode)
        ref, got = torch_fwd(), legs["nk"]()
        with torch.no_grad():
            assert torch.equal(conv(P, P, nbr, x), got) or K == 15      # the module's own route at K != 15 is the `nk` leg
        diff = float(((got - ref).norm(dim=1) / torch.clamp(ref.norm(dim=1), min=float(ref.norm(dim=1).median()))).max())
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
        rows.append(dict(level=level, N=N, H=H, c=c, K=K, us=med, spread_us=spread, nk_vs_torch_rows_rel_l2=diff))
        print(f"level {level} N={N} H={H} c={c} K={K}: " + "  ".join(f"{k} {med[k]:.1f} (+-{spread[k]:.1f})" for k in legs) +
              f"  nk vs torch rows rel-L2 {diff:.2e}", flush=True)
print(json.dumps(rows))
