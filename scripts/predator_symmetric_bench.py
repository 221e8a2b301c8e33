"""Predator_APR's symmetric recipe (KPFCNNDecoder as the generator) on one full-size synthetic pair, next to the MLP recipe
of the same commit.  Prints one JSON line:

    iteration       synchronised PredatorPairTrainStep time (median of --iters, after --warmup) and
                    torch.cuda.max_memory_allocated() of the step, symmetric and MLP
    generator       KPFCNNDecoder forward + backward alone (loss = sum(out * G)), median
    level0_kpconv   kp_ops.kpconv_weighted at the generator's first layer (cin = 32, the finest level's neighbour table) on
                    both routes -- apr_kpconv_weighted_c32 and apr_kpconv_weighted's generic kernel -- alternated in one
                    process, median of --launches device-event timings each, and the largest element difference

The pair: learned.synthetic_sample at --beams x --azimuth (64 x 1875: a KITTI frame), neighbour limits from
calibrate_neighbors on it, collated by the project's own loader.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from apr_amd.predator import kp_ops  # noqa: E402
from apr_amd.predator.configs.models import kitti_config  # noqa: E402
from apr_amd.predator.datasets.dataloader import calibrate_neighbors, collate_fn_descriptor  # noqa: E402
from apr_amd.predator.lib import learned  # noqa: E402
from apr_amd.predator.lib.trainer import PredatorPairTrainStep  # noqa: E402


def event_times(fn, n):
    """device-event time of each of n calls, ms"""
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def timed_step(step, batch, warmup, iters):
    for _ in range(warmup):
        step(batch)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(iters):
        t0 = time.perf_counter()
        step(batch)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
            "peak_allocated_mb": torch.cuda.max_memory_allocated() / 2 ** 20}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", type=int, default=64)
    ap.add_argument("--azimuth", type=int, default=1875)
    ap.add_argument("--complement", type=int, default=5, help="complement scans on each side of a key frame")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--skip-iteration", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predator_symmetric_bench: needs a GPU")
    dev = torch.device("cuda:0")
    out = {"pair": f"{a.beams} x {a.azimuth}"}

    cfg = kitti_config(**learned.LOSS)
    item = learned.synthetic_sample(dev, 0, cfg, "train", a.beams, a.azimuth, a.complement)
    limits = [int(v) for v in calibrate_neighbors([item], cfg)]
    batch = collate_fn_descriptor([item], cfg, limits)
    out["limits"], out["level_sizes"] = limits, [int(p.shape[0]) for p in batch["points"]]

    # ---- the first layer of the generator on both routes
    model, gen, opt, _ = learned.build_models(dev, cfg, 0, symmetric=True)
    conv = gen.encoder_blocks[0].KPConv
    pts, nbr = batch["points"][0], batch["neighbors"][0]
    x = torch.nn.functional.normalize(torch.randn((pts.shape[0], cfg.final_feats_dim), device=dev), dim=1)
    saved = kp_ops.KPCONV_C32

    def route(on):
        kp_ops.KPCONV_C32 = on
        return kp_ops.kpconv_weighted(pts, pts, nbr, x, conv.kernel_points, conv.KP_extent)
    try:
        diff = float((route(True) - route(False)).abs().max())
        for _ in range(3):
            route(True), route(False)
        t = {True: [], False: []}
        for _ in range(a.launches):                 # alternated: both routes see the same neighbours on the machine
            for on in (True, False):
                t[on] += event_times(lambda: route(on), 1)
    finally:
        kp_ops.KPCONV_C32 = saved
    out["level0_kpconv"] = {"nq": int(nbr.shape[0]), "H": int(nbr.shape[1]), "cin": int(x.shape[1]), "launches": a.launches,
                            "includes": "apr_row_sums + the correlation kernel + the output allocation",
                            "c32_us_median": statistics.median(t[True]) * 1e3, "generic_us_median": statistics.median(t[False]) * 1e3,
                            "c32_us_min": min(t[True]) * 1e3, "generic_us_min": min(t[False]) * 1e3, "max_abs_difference": diff}

    # ---- the generator alone
    batch["second_features"] = x
    G = torch.randn((pts.shape[0], cfg.point_generation_ratio * 3), device=dev)
    gen.train()

    def fwd_bwd():
        gen.zero_grad(set_to_none=True)
        (gen(batch) * G).sum().backward()
    for _ in range(a.warmup):
        fwd_bwd()
    torch.cuda.synchronize()
    ms = event_times(fwd_bwd, a.iters)
    out["generator"] = {"forward_backward_ms_median": statistics.median(ms), "ms_min": min(ms),
                        "parameters": sum(p.numel() for p in gen.parameters())}

    # ---- the iteration, symmetric and MLP
    if not a.skip_iteration:
        np.random.seed(0)
        out["iteration"] = {"symmetric": timed_step(PredatorPairTrainStep(model, gen, opt, cfg), batch, a.warmup, a.iters)}
        del model, gen, opt
        torch.cuda.empty_cache()
        cfg2 = kitti_config(**learned.LOSS)
        model, gen, opt, _ = learned.build_models(dev, cfg2, 0)
        np.random.seed(0)
        out["iteration"]["mlp"] = timed_step(PredatorPairTrainStep(model, gen, opt, cfg2), batch, a.warmup, a.iters)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
