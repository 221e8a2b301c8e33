"""The symmetric recipe's new ground, measured: the generator's 5^3 conv1 on the big-kernel MFMA kernel
(spconv_bigk.hip) against the generic kernel it replaces, and the symmetric training iteration next to the MLP one.

    python scripts/symmetric_bench.py [--rounds 5] [--iters 8] [--out FILE.json]

Layer table, at the recipe's shape (one full-size synthetic pair, both frames stacked, the real (1, 1, 5) kernel map):
conv1 forward (128 -> 32, K = 125), its input gradient (32 -> 128 over the same table, flip-transposed weights) and the
weight gradient, in us per launch.  APR_SPCONV_BIGK is read once per process, so A (new kernel) and B (APR_SPCONV_BIGK=0:
k_spconv_generic, what the parent commit ran) are FRESH CHILD PROCESSES run alternately A B A B ... on the same device; each
child reports the median of its timing windows, the table gives the median over the rounds with the min .. max spread.
Then one child measures the symmetric iteration (complement_trainer.measure(symmetric=True)) and the MLP iteration
(workloads.apr_train_step's measure) back to back.  A child that fails ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _windows(fn, n_windows=7, per=20):
    """us per launch of `fn(batch)`-enqueued work: `per` launches leave through ONE library call, timed by a HIP event pair."""
    import torch
    out = []
    for _ in range(n_windows + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        work = fn(per)
        torch.cuda.synchronize()
        e0.record()
        work()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1000 / per)
    return out[2:]      # the first two windows warm up


def child_layers():
    import numpy as np
    import torch
    from apr_amd import ops, synth
    from apr_amd.MinkowskiEngine.core import CoordinateManager
    dev = torch.device("cuda:0")
    xyz0, xyz1, _ = synth.make_pair(0)
    maps = [ops.build_map(ops.voxelize(torch.from_numpy(x).to(dev), 0.3, b)) for b, x in enumerate((xyz0, xyz1))]
    ops.finalize_maps(maps)
    cm = CoordinateManager(torch.cat([m.coords for m in maps]))
    nbr = cm.kernel_map(1, 1, 5)
    n = nbr.shape[0]
    occ = nbr >= 0
    P = int(occ.sum())
    # MFMA padding of the kernel's tiling: pairs of one (64-row tile, offset) padded to groups of 16
    pad_rows = (-n) % 64
    tiles = torch.cat([occ, occ.new_zeros((pad_rows, 125))]).reshape(-1, 64, 125).sum(1)
    padded = int(((tiles + 15) // 16 * 16).sum())
    g = torch.Generator(device="cpu").manual_seed(0)
    res = {"rows": n, "pairs": P, "pairs_per_row": P / n, "max_pairs_per_row": int(occ.sum(1).max()),
           "active_offsets_per_tile": float((tiles > 0).sum(1).float().mean()), "padding_share": 1.0 - P / padded,
           "bigk": os.environ.get("APR_SPCONV_BIGK", "1") != "0"}
    W = (torch.randn(125, 128, 32, generator=g) / 126.0).to(dev)
    x = torch.randn(n, 128, generator=g).to(dev)
    dy = torch.randn(n, 32, generator=g).to(dev)
    for name, inp, w, cin, cout in (("conv1_forward", x, W, 128, 32), ("conv1_input_gradient", dy, ops.weights_flip_transpose(W, True), 32, 128)):
        wp = ops.pack_weights(w)
        out = torch.empty(n, cout, device=dev)

        def enqueue(per, inp=inp, wp=wp, cin=cin, cout=cout, out=out):
            b = ops.SpconvBatch()
            for _ in range(per):
                b.add(inp, nbr, 125, cin, cout, wp, out=out)
            return b.launch
        us = _windows(enqueue)
        res[name] = {"us": float(np.median(us)), "min": min(us), "max": max(us), "checksum": float(out.double().norm())}

    def wgrad(per):
        def run():
            for _ in range(per):
                ops.spconv_wgrad(x, dy, nbr, 125, 128, 32, same_level=True)
        return run
    us = _windows(wgrad, per=5)
    res["weight_gradient"] = {"us": float(np.median(us)), "min": min(us), "max": max(us),
                              "scratch_bytes": int(ops._lib_().apr_spconv_wgrad_scratch_bytes(n, 125, 128, 32))}
    print("RESULT " + json.dumps(res), flush=True)


def child_iteration(iters):
    import torch
    from apr_amd.fcgf.lib import complement_trainer as CT
    dev = torch.device("cuda:0")
    res = {}
    for name, sym in (("symmetric", True), ("mlp", False)):
        r = CT.measure(dev, iters=iters, symmetric=sym)
        res[name] = {"ms": r["value"], "unsynchronised_ms": r["ms_per_iteration_unsynchronised_loop"], "stages_ms": r["stages_ms"],
                     "voxels": r["voxels"], "loss_first_last": r["loss_first_last"]}
    print("RESULT " + json.dumps(res), flush=True)


def run_child(args, env_extra, timeout):
    env = dict(os.environ, **env_extra)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"child {args} {env_extra} ended with {p.returncode}: stopping")
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child == "layers":
        return child_layers()
    if a.child == "iteration":
        return child_iteration(a.iters)
    import numpy as np
    runs = {"new": [], "generic": []}
    for r in range(a.rounds):      # A B A B ...: both see the same drift of the shared machine
        for tag, flag in (("new", "1"), ("generic", "0")):
            runs[tag].append(run_child(["--child", "layers"], {"APR_SPCONV_BIGK": flag}, 300))
            print(f"round {r} {tag}: " + ", ".join(f"{k} {runs[tag][-1][k]['us']:.1f} us" for k in
                                                    ("conv1_forward", "conv1_input_gradient", "weight_gradient")), flush=True)
    table = {}
    for k in ("conv1_forward", "conv1_input_gradient", "weight_gradient"):
        table[k] = {}
        for tag in runs:
            v = [x[k]["us"] for x in runs[tag]]
            table[k][tag] = {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)}
    for k in ("conv1_forward", "conv1_input_gradient"):      # faster by more than the run-to-run spread?
        table[k]["new_is_faster_beyond_spread"] = table[k]["new"]["max_us"] < table[k]["generic"]["min_us"]
        a_, b_ = runs["new"][0][k]["checksum"], runs["generic"][0][k]["checksum"]
        table[k]["checksum_rel_diff"] = abs(a_ - b_) / abs(b_)
    shape = {k: runs["new"][0][k] for k in ("rows", "pairs", "pairs_per_row", "max_pairs_per_row", "active_offsets_per_tile",
                                            "padding_share")}
    shape["wgrad_scratch_bytes"] = runs["new"][0]["weight_gradient"]["scratch_bytes"]
    out = {"shape": shape, "layers_us": table, "iteration": run_child(["--child", "iteration", "--iters", str(a.iters)], {}, 900)}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
