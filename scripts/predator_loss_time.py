"""Predator_APR's descriptor loss at KITTI size: the HIP path (apr_amd/predator/lib/loss.py) against the fp32 torch
restatement of the reference's forward (tests/predator_loss_oracle.py) on the same GPU, and one PredatorPairTrainStep.

    python scripts/predator_loss_time.py            # prints one JSON line; CALLS=50 WARMUP=5 by default

One full-size synthetic pair (2 x ~118 k points, one point per 0.3 m voxel, correspondences within 0.45 m), trained-like
features (a smooth function of the world position plus noise).  Per path: milliseconds per forward + backward (HIP events
around CALLS calls after WARMUP), kernel launches per call (torch.profiler's device-kernel events of one call) and peak
extra device memory of one call.  The baseline draws its permutation and fetches its counts as the reference does; the HIP
path is timed both with `choice=None` (one 4-byte fetch) and with `choice` given (no synchronisation).  The train step
runs on the pair collated at the same size when the reference's grid subsampling (oracle/_ref) is present.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from apr_amd import ops, synth
from apr_amd.fcgf.lib import apg
from apr_amd.predator.lib.loss import MetricLoss
from tests import predator_loss_oracle as O
from tests.predator_loss_fixture import train_config

CALLS, WARMUP = int(os.environ.get("CALLS", "50")), int(os.environ.get("WARMUP", "5"))


def make_inputs(dev, seed=0, beams=64, azimuth=1875):
    xyz0, xyz1, T = synth.make_pair(seed, n_beams=beams, n_azimuth=azimuth)
    pts = []
    for xyz in (xyz0, xyz1):
        key = torch.from_numpy(xyz).to(dev)
        m = ops.build_map(ops.voxelize(key, 0.3, 0), want_first=True)
        ops.finalize_maps([m])
        pts.append(key[m.first.long()].contiguous())
    Tt = torch.from_numpy(T).float().to(dev)
    corr = apg.get_matching_indices(pts[0], pts[1], Tt, 0.45).contiguous()
    g = torch.Generator(device="cpu").manual_seed(seed)
    W = (torch.randn(3, 32, generator=g) * 0.35).to(dev)
    ph = (torch.rand(32, generator=g) * 6.2831853).to(dev)
    world = pts[0] @ Tt[:3, :3].T + Tt[:3, 3]
    feat = lambda w: torch.nn.functional.normalize(torch.sin(w @ W + ph) + 0.25 * torch.randn(len(w), 32, generator=g).to(dev), dim=1)
    n = len(pts[0]) + len(pts[1])
    return dict(src_pcd=pts[0], tgt_pcd=pts[1], src_feats=feat(world), tgt_feats=feat(pts[1]), correspondence=corr,
                rot=Tt[:3, :3].contiguous(), trans=Tt[:3, 3:].contiguous(),
                scores_overlap=torch.sigmoid(torch.randn(n, generator=g)).to(dev),
                scores_saliency=torch.sigmoid(torch.randn(n, generator=g)).to(dev))


def measure(call, dev):
    for _ in range(WARMUP):
        call()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    call()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    launches = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    except Exception as exc:                                   # the count is a convenience; the times do not depend on it
        launches = f"not counted ({type(exc).__name__})"
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(CALLS):
        call()
    e1.record()
    torch.cuda.synchronize()
    return {"ms_per_call": e0.elapsed_time(e1) / CALLS, "launches_per_call": launches, "peak_extra_bytes": int(peak)}


def main():
    dev = torch.device("cuda:0")
    inp = make_inputs(dev)
    cfg = train_config()
    m = MetricLoss(cfg).to(dev)
    leaves = ("src_feats", "tgt_feats", "scores_overlap", "scores_saliency")

    def fresh():
        d = dict(inp)
        for k in leaves:
            d[k] = inp[k].detach().requires_grad_(True)
        return d

    def hip(choice=None):
        d = fresh()
        s = m(**d, choice=choice)
        (s["circle_loss"] + s["overlap_loss"] + s["saliency_loss"]).backward()

    def torch_fp32():
        d = fresh()
        s = O.forward(**d)
        (s["circle_loss"] + s["overlap_loss"] + s["saliency_loss"]).backward()

    out = {"points": [int(inp["src_pcd"].shape[0]), int(inp["tgt_pcd"].shape[0])],
           "correspondences": int(inp["correspondence"].shape[0]), "calls": CALLS}
    filt, count = m.select(inp["src_pcd"], inp["tgt_pcd"], inp["correspondence"], inp["rot"], inp["trans"])
    n_f = int(count)
    gt, si, ti, counts = ops.overlap_labels(inp["correspondence"], out["points"][0], out["points"][1])
    out["filtered"], out["overlap_rows"] = n_f, [int(counts[0]), int(counts[1])]
    out["score_matrix_bytes"] = out["overlap_rows"][0] * out["overlap_rows"][1] * 4
    np.random.seed(0)
    choice = torch.from_numpy(np.ascontiguousarray(m.draw_choice(n_f), dtype=np.int64)).to(dev)
    out["hip_choice_none"] = measure(lambda: hip(None), dev)
    out["hip_choice_given"] = measure(lambda: hip(choice), dev)
    try:
        out["torch_fp32_restatement"] = measure(torch_fp32, dev)
    except torch.OutOfMemoryError as exc:
        out["torch_fp32_restatement"] = f"does not fit: {exc}"
    # the whole iteration
    try:
        from oracle import predator_points_oracle as PREF
        if not PREF.available():
            raise RuntimeError("oracle/_ref not built")
        from apr_amd.predator.lib.trainer import PredatorPairTrainStep
        from apr_amd.predator.models.architectures import KPFCNN
        from apr_amd.predator.models.mlp import GenerativeMLP_98
        from tests.predator_loss_fixture import collated, small_pair
        pair = small_pair(0, 64, 1875)
        batch = collated(pair, cfg, [30, 30, 30, 30], dev)
        torch.manual_seed(0)
        model = KPFCNN(cfg).to(dev)
        gen = GenerativeMLP_98(in_channel=32, out_points=cfg.point_generation_ratio, radius=None, bn_momentum=0.02).to(dev)
        opt = torch.optim.SGD([{"params": model.parameters()}, {"params": gen.parameters()}], lr=1e-3, momentum=0.98,
                              weight_decay=1e-6)
        step = PredatorPairTrainStep(model, gen, opt, cfg)
        for _ in range(3):
            step(batch)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        iters = 10
        for _ in range(iters):
            step(batch)
        e1.record()
        torch.cuda.synchronize()
        out["train_step"] = {"ms_per_iteration": e0.elapsed_time(e1) / iters, "points": [len(pair["src"]), len(pair["tgt"])],
                             "correspondences": len(pair["corr"])}
    except Exception as exc:
        out["train_step"] = f"not measured: {type(exc).__name__}: {exc}"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
