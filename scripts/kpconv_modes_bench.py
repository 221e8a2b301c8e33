"""Rigid KPConv layers of the KITTI pyramid's four levels (mid widths 64, 128, 256, 512) on the synthetic KITTI pair of
scripts/kpconv_bench.py, in each of the six (KP_influence, aggregation_mode) combinations:

    hip     blocks.KPConv on apr_kpconv_weighted(_mode) + the dense GEMM; training adds apr_kpconv_dfeat_contrib(_mode), the
            ordered gather and apr_spconv_wgrad
    torch   the same module's torch formulation (_forward_autograd: the reference's ops on the same device)

forward (no_grad) and forward + backward.  All legs warmed, alternated in ONE process, every window at least MIN_WINDOW
seconds of device time between two events, ALTERNATIONS alternations: median and spread (max - min) of the per-call times in
microseconds.  One JSON line at the end (DESIGN section 34 quotes it)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from apr_amd import synth
from apr_amd.predator import point_ops
from apr_amd.predator.configs.models import kitti_config
from apr_amd.predator.datasets.dataloader import collate_fn_descriptor
from apr_amd.predator.models import blocks
from bench_predator import LIMITS

blocks.KPCONV_MODES = True      # the modes are behind a switch that is off by default (APR_KPCONV_MODES)
MIN_WINDOW, ALTERNATIONS = 0.1, 3
MODES = [(i, a) for i in ("constant", "linear", "gaussian") for a in ("sum", "closest")]
dev = torch.device("cuda:0")
cfg = kitti_config()
a, b, _ = synth.make_pair(0)
pts, lens = point_ops.grid_subsample(torch.cat([torch.from_numpy(a), torch.from_numpy(b)]).to(dev),
                                     np.array([len(a), len(b)], np.int32), 0.3)
src, tgt = pts[:lens[0]], pts[lens[0]:]
ones = lambda p: torch.ones((len(p), 1), device=dev)
batch = collate_fn_descriptor([(src, tgt, ones(src), ones(tgt))], cfg, LIMITS)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps       # us per call


rows = []
for level, c in ((0, 64), (1, 128), (2, 256), (3, 512)):
    P, nbr = batch['points'][level], batch['neighbors'][level]
    N, H = nbr.shape
    radius = cfg.first_subsampling_dl * cfg.conv_radius * 2 ** level
    extent = radius * cfg.KP_extent / cfg.conv_radius
    x = torch.randn(N, c, device=dev).abs()
    dout = torch.randn(N, c, device=dev)
    for inf, agg in MODES:
        torch.manual_seed(level)
        np.random.seed(level)
        conv = blocks.KPConv(15, 3, c, c, extent, radius, KP_influence=inf, aggregation_mode=agg).to(dev)

        def hip_fwd():
            with torch.no_grad():
                return conv(P, P, nbr, x)

        def torch_fwd():
            with torch.no_grad():
                return conv._forward_autograd(P, P, nbr, x)

        def fwdbwd(hip):
            def run():
                blocks.KPCONV_TRAIN_HIP = hip
                conv.zero_grad(set_to_none=True)
                xx = x.detach().requires_grad_(True)
                conv(P, P, nbr, xx).backward(dout)
                return xx.grad
            return run

        legs = {"hip_fwd": hip_fwd, "torch_fwd": torch_fwd, "hip_fwdbwd": fwdbwd(True), "torch_fwdbwd": fwdbwd(False)}
        ref, got = torch_fwd(), hip_fwd()
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
        blocks.KPCONV_TRAIN_HIP = True
        med = {k: round(statistics.median(v), 1) for k, v in t.items()}
        spread = {k: round(max(v) - min(v), 1) for k, v in t.items()}
        rows.append(dict(level=level, N=N, H=H, c=c, mode=f"{inf}-{agg}", us=med, spread_us=spread, hip_vs_torch_rows_rel_l2=diff))
        print(f"level {level} N={N} H={H} c={c} {inf}-{agg}: " + "  ".join(f"{k} {med[k]:.1f} (+-{spread[k]:.1f})" for k in legs) +
              f"  hip vs torch rows rel-L2 {diff:.2e}", flush=True)
print(json.dumps(rows))
