"""Fused KPConv forward (apr_kpconv_fused) against the two launches it replaces, per level of the KPFCNN pyramid on the
synthetic KITTI pair of scripts/kpconv_bench.py (same LIMITS, same levels), cin = cout = 64 / 128 / 256 / 512:

    two launches:  apr_row_sums + apr_kpconv_weighted + apr_dense_gemm_bf3      (wf [N, 15 cin] through HBM)
    fused:         apr_row_sums + apr_kpconv_fused

Both warmed, alternated in ONE process, every window at least MIN_WINDOW seconds of device time between two events, five
alternations: median and spread (max - min) of the per-call times.  Before timing, the two outputs are compared on the timed
inputs (row-relative L2).  Algorithmic bytes with and without the 2 * 4 * N * 15 * cin round trip."""
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
from apr_amd.predator.kernels.kernel_points import load_kernels
from bench_predator import LIMITS

MIN_WINDOW, ALTERNATIONS = 0.2, 5
dev = torch.device("cuda:0")
cfg = kitti_config()
a, b, _ = synth.make_pair(0)
pts, lens = point_ops.grid_subsample(torch.cat([torch.from_numpy(a), torch.from_numpy(b)]).to(dev),
                                     np.array([len(a), len(b)], np.int32), 0.3)
src, tgt = pts[:lens[0]], pts[lens[0]:]
ones = lambda p: torch.ones((len(p), 1), device=dev)
batch = collate_fn_descriptor([(src, tgt, ones(src), ones(tgt))], cfg, LIMITS)
kp = torch.from_numpy(load_kernels(1.0, 15, dimension=3, fixed='center').astype(np.float32)).to(dev)
lib = _lib.load()


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps       # us per call


def rows_rel_l2(got, ref):
    norms = ref.norm(dim=1)
    return float(((got - ref).norm(dim=1) / torch.clamp(norms, min=float(norms.median()))).max())


rows = []
for level, c in enumerate((64, 128, 256, 512)):
    P, nbr = batch['points'][level], batch['neighbors'][level]
    N, H = nbr.shape
    extent = 0.6 * 2 ** level
    kpts = (kp * extent).contiguous()
    torch.manual_seed(level)
    x = torch.randn(N, c, device=dev)
    w_info = kp_ops.pack_linear(torch.randn(15 * c, c, device=dev) / (15 * c) ** 0.5)
    two = lambda: kp_ops.linear(kp_ops.kpconv_weighted(P, P, nbr, x, kpts, extent), w_info)
    fused = lambda: kp_ops.kpconv_fused(P, P, nbr, x, kpts, extent, w_info)
    diff = rows_rel_l2(fused(), two())
    reps = {}
    for name, fn in (("two", two), ("fused", fused)):
        for _ in range(3):
            fn()
        reps[name] = max(3, int(MIN_WINDOW * 1e6 / window(fn, 5)) + 1)
    t = {"two": [], "fused": []}
    for _ in range(ALTERNATIONS):
        for name, fn in (("two", two), ("fused", fused)):
            t[name].append(window(fn, reps[name]))
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: max(v) - min(v) for k, v in t.items()}
    base = 4.0 * N * H * (3 + c) + 8.0 * N * H + 4.0 * N * c + 4.0 * N * c      # gather + table + row sums + out
    trip = 2.0 * 4.0 * N * 15 * c
    gap = med["two"] - med["fused"]
    row = dict(level=level, N=N, H=H, cin=c, cout=c, two_us=round(med["two"], 1), two_spread_us=round(spread["two"], 1),
               fused_us=round(med["fused"], 1), fused_spread_us=round(spread["fused"], 1),
               fused_faster=bool(gap > max(spread.values())), rows_rel_l2=diff, bytes_fused_mb=round(base / 1e6, 1),
               bytes_two_mb=round((base + trip) / 1e6, 1), route=int(lib.apr_kpconv_fused_route(N, c, c, H)))
    rows.append(row)
    print(f"level {level}: N={N:6d} H={H:3d} c={c:4d}: two launches {med['two']:8.1f} us (spread {spread['two']:6.1f})   fused "
          f"{med['fused']:8.1f} us (spread {spread['fused']:6.1f})   rows rel-L2 {diff:.2e}   bytes {(base + trip) / 1e6:7.1f} -> "
          f"{base / 1e6:6.1f} MB   {'FUSED FASTER' if row['fused_faster'] else 'not faster'}", flush=True)
print(json.dumps(rows))
