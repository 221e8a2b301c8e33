"""Reference-pinned fixture of Predator_APR's descriptor loss: tests/golden/predator_loss_ref.npz.

Run where the reference checkout is present (sklearn and matplotlib importable):
    python tests/golden/make_predator_loss_ref_golden.py

Same rule as make_predator_ref_golden.py: `square_distance` (Predator_APR/lib/utils.py:78-98) and the four methods of
`MetricLoss` (lib/loss.py:34-178) are cut out of the reference's files with `ast`, compiled unchanged and executed on
seeded inputs.  `forward` names `torch.device('cuda')` (:123): the name `torch` in the exec namespace is bound to a proxy
whose `device()` answers the CPU.  Two legs per case: fp32 (the reference as it is) and fp64 (the same text on float64
inputs, the yardstick; there `torch.zeros(n)` and `.float()`, which name float32 in the text, are made to mean float64).  Only numeric arrays are stored: inputs, the eight stats, the gradients with respect to src_feats /
tgt_feats (their non-zero rows) / scores_overlap / scores_saliency of the fp64 leg -- of the fp32 leg only the relative L2
distance of each gradient from the fp64 leg's, to stay under the repository's 1 MiB file limit --, the permutation drawn at :157 and the next value of
the NumPy stream after the call.

Cases
  kitti    synth.make_pair(13, 16 beams x 400), one barycentre per 0.3 m cell, correspondences within 0.45 m; more than
           max_points = 512 of them pass the pos_radius filter, so :157 draws.  Features: a smooth function of the world
           position plus noise (trained-like: neither the circle loss nor the recall is degenerate); rows outside the
           overlap region are zero (no output depends on them; it keeps the file small).
  short    fewer than max_points filtered correspondences; two target rows of the overlap region share one feature row
           (a planted exact score tie).
  cluster  anchors inside a 0.7 m ball with one source anchor at its centre: that row has no negative (row_sel false).
  bce      get_weighted_bce_loss alone with predictions at exactly 0.5, 0 and 1.

Decision margins: on these inputs the fp64 leg must not sit within fp32 rounding of any decision (|p - 0.5|, |distance -
radius|, the top-two score gap outside the planted tie); checked here, so the GPU test's exclusion lists stay empty for
the yardstick itself.
"""
import ast
import os
import sys
import textwrap
import types

import numpy as np
import torch
from scipy.spatial import cKDTree

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
PRED = "/root/reference/Predator_APR"

from tests.predator_loss_oracle import KITTI  # noqa: E402


def _defs(path, names, ns, cls=None):
    src = open(path, encoding="utf-8").read()
    body = ast.parse(src).body
    if cls is not None:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == cls).body
    found = {n.name: textwrap.dedent("\n".join(src.splitlines()[n.lineno - 1:n.end_lineno]))
             for n in body if isinstance(n, ast.FunctionDef) and n.name in names}
    assert set(found) == set(names), set(names) - set(found)
    for name in names:
        exec(compile(found[name], f"{path}:{name}", "exec"), ns)
    return ns


class _TorchOnCpu:
    """`torch` for the reference's text: everything is torch's, `device()` answers the CPU."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def device(*_a, **_k):
        return torch.device("cpu")


def reference_loss():
    import torch.nn as nn
    import torch.nn.functional as F
    from sklearn.metrics import precision_recall_fscore_support
    ns = {"torch": _TorchOnCpu(), "nn": nn, "F": F, "np": np, "precision_recall_fscore_support": precision_recall_fscore_support}
    _defs(os.path.join(PRED, "lib/utils.py"), ["square_distance"], ns)
    names = ["get_circle_loss", "get_recall", "get_weighted_bce_loss", "forward"]
    _defs(os.path.join(PRED, "lib/loss.py"), names, ns, cls="MetricLoss")
    stub = types.SimpleNamespace(**{k: KITTI[k] for k in KITTI})
    for n in names:
        setattr(stub, n, types.MethodType(ns[n], stub))
    return stub


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def barycentres(xyz, dl):
    key = np.floor(xyz.astype(np.float64) / dl).astype(np.int64)
    _, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    out = np.zeros((inv.max() + 1, 3))
    np.add.at(out, inv, xyz.astype(np.float64))
    return (out / np.bincount(inv)[:, None]).astype(np.float32)


def pairs_within(src_w, tgt, radius):
    hits = cKDTree(tgt.astype(np.float64)).query_ball_point(src_w.astype(np.float64), radius)
    return np.array([(i, j) for i, h in enumerate(hits) for j in sorted(h)], np.int64).reshape(-1, 2)


def smooth_features(world, rng, noise, scale=0.35):
    W = rng.standard_normal((3, 32)) * scale
    ph = rng.uniform(0, 2 * np.pi, 32)
    f = np.sin(world.astype(np.float64) @ W + ph) + noise * rng.standard_normal((len(world), 32))
    return (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)


def scores(rng, gt, n):
    """overlap-like scores: the label with noise through a sigmoid, strictly inside (0, 1)."""
    z = (gt * 2 - 1) * 1.2 + rng.standard_normal(n)
    return (1 / (1 + np.exp(-z))).astype(np.float32)


def finish(rng, src, tgt, R, t, corr, fs, ft):
    n, m = len(src), len(tgt)
    gt = np.zeros(n + m)
    gt[np.unique(corr[:, 0])] = 1
    gt[n + np.unique(corr[:, 1])] = 1
    return dict(src_pcd=src, tgt_pcd=tgt, src_feats=fs, tgt_feats=ft, correspondence=corr, rot=R.astype(np.float32),
                trans=t.astype(np.float32).reshape(3, 1), scores_overlap=scores(rng, gt, n + m),
                scores_saliency=scores(rng, rng.integers(0, 2, n + m).astype(np.float64), n + m))


def case_kitti():
    from apr_amd import synth
    rng = np.random.default_rng(13)
    a, b, T = synth.make_pair(13, n_beams=16, n_azimuth=400)
    src, tgt = barycentres(a, 0.3), barycentres(b, 0.3)
    R, t = T[:3, :3], T[:3, 3]
    src_w = src @ R.T.astype(np.float32) + t.astype(np.float32)
    corr = pairs_within(src_w, tgt, 0.45)
    base2 = np.random.default_rng(5)
    W = base2.standard_normal((3, 32)) * 0.35
    ph = base2.uniform(0, 2 * np.pi, 32)
    noise = np.random.default_rng(6)
    mk = lambda w: (lambda f: (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32))(
        np.sin(w.astype(np.float64) @ W + ph) + 0.25 * noise.standard_normal((len(w), 32)))
    fs, ft = mk(src_w), mk(tgt)
    keep_s = np.zeros(len(src), bool)
    keep_t = np.zeros(len(tgt), bool)
    keep_s[corr[:, 0]] = True
    keep_t[corr[:, 1]] = True
    fs[~keep_s] = 0
    ft[~keep_t] = 0
    return finish(rng, src, tgt, R, t, corr, fs, ft)


def _random_pair(rng, n, extra, jitter, box):
    a = np.deg2rad(9.0)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    t = np.array([1.5, -0.7, 0.2])
    tgt_core = rng.uniform(-box, box, (n, 3))
    src_w = tgt_core + rng.normal(0, jitter, (n, 3))
    src = np.concatenate([(src_w - t) @ R, rng.uniform(40, 60, (extra, 3))]).astype(np.float32)    # R^T (w - t)
    tgt = np.concatenate([tgt_core, rng.uniform(-60, -40, (extra, 3))]).astype(np.float32)
    return src, tgt, R, t


def case_short():
    rng = np.random.default_rng(21)
    src, tgt, R, t = _random_pair(rng, 220, 80, 0.08, 9.0)
    src_w = src @ R.T.astype(np.float32) + t.astype(np.float32)
    corr = pairs_within(src_w, tgt, 0.45)
    W = rng.standard_normal((3, 32)) * 0.5
    ph = rng.uniform(0, 2 * np.pi, 32)
    mk = lambda w: (lambda f: (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32))(
        np.sin(w.astype(np.float64) @ W + ph) + 0.3 * rng.standard_normal((len(w), 32)))
    fs, ft = mk(src_w), mk(tgt)
    rows = np.unique(corr[:, 1])
    ft[rows[7]] = ft[rows[3]]                                 # the planted exact tie: two listed target rows, one feature row
    fs[np.unique(corr[:, 0])[5]] = ft[rows[3]]                # ... and a source row whose best score is that pair
    return finish(rng, src, tgt, R, t, corr, fs, ft)


def case_cluster():
    rng = np.random.default_rng(33)
    n = 70
    d = rng.standard_normal((n, 3))
    core = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.05, 0.7, (n, 1)) + np.array([3.0, 2.0, 1.0])
    core[0] = [3.0, 2.0, 1.0]                                  # the centre: every anchor within 0.75 m of it
    a = np.deg2rad(-6.0)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    t = np.array([-0.4, 0.9, 0.1])
    src_w = core + rng.normal(0, 0.004, (n, 3))
    src_w[0] = core[0]
    src = np.concatenate([(src_w - t) @ R, rng.uniform(20, 30, (60, 3))]).astype(np.float32)
    tgt = np.concatenate([core, rng.uniform(-30, -20, (60, 3))]).astype(np.float32)
    src_w32 = src @ R.T.astype(np.float32) + t.astype(np.float32)
    corr = pairs_within(src_w32, tgt, 0.45)
    fs, ft = smooth_features(src_w32, np.random.default_rng(34), 0.3, 1.5), smooth_features(tgt, np.random.default_rng(34), 0.3, 1.5)
    return finish(rng, src, tgt, R, t, corr, fs, ft)


def case_bce():
    rng = np.random.default_rng(44)
    n = 300
    gt = (rng.random(n) < 0.35).astype(np.float32)
    p = scores(rng, gt.astype(np.float64), n)
    p[:12] = [0.5, 0.5, 0.0, 0.0, 1.0, 1.0, 0.5, 0.0, 1.0, 0.5, 0.0, 1.0]
    gt[:12] = [0, 1, 0, 1, 0, 1, 1, 0, 1, 0, 1, 0]
    return p, gt


# ---------------------------------------------------------------------------------------------------------------------
def run_leg(ref, inp, dtype, seed):
    t = lambda k: torch.from_numpy(inp[k].astype(np.float64 if inp[k].dtype.kind == "f" else inp[k].dtype)).to(
        dtype if inp[k].dtype.kind == "f" else torch.int64)
    leaf = {k: t(k).requires_grad_(True) for k in ("src_feats", "tgt_feats", "scores_overlap", "scores_saliency")}
    np.random.seed(seed)
    state0 = np.random.get_state()
    # `torch.zeros(n)` (:119-121) and `.float()` (:46, :50, :72, :75, :140) name float32: in the fp64 leg both mean float64
    torch.set_default_dtype(dtype)
    tensor_float = torch.Tensor.float
    torch.Tensor.float = lambda self: self.to(dtype)
    stats = ref.forward(t("src_pcd"), t("tgt_pcd"), leaf["src_feats"], leaf["tgt_feats"], t("correspondence"), t("rot"),
                        t("trans"), leaf["scores_overlap"], leaf["scores_saliency"])
    torch.set_default_dtype(torch.float32)
    torch.Tensor.float = tensor_float
    after = np.random.random_sample()
    np.random.set_state(state0)
    (stats["circle_loss"] + stats["overlap_loss"] + stats["saliency_loss"]).backward()
    out = {k: np.array(float(v), np.float64) for k, v in stats.items()}
    for k, v in leaf.items():
        out["grad_" + k] = v.grad.numpy().astype(np.float64)
    out["next_uniform"] = np.array(after)
    return out


def check_margins(name, inp, planted_tie):
    """The fp64 yardstick itself sits clear of every decision boundary (fp32 rounding of the quantities involved)."""
    from tests import predator_loss_oracle as O
    t = lambda k: torch.from_numpy(inp[k].astype(np.float64) if inp[k].dtype.kind == "f" else inp[k])
    keep = {}
    np.random.seed(0)
    O.forward(t("src_pcd"), t("tgt_pcd"), t("src_feats"), t("tgt_feats"), t("correspondence"), t("rot"), t("trans"),
              t("scores_overlap"), t("scores_saliency"), keep=keep)
    eps = 2.0 ** -23
    assert float((t("scores_overlap") - 0.5).abs().min()) > 4 * eps, name
    assert float((keep["saliency_pred"] - 0.5).abs().min()) > 4 * eps, name
    # a distance between two fp32 points: a few roundings at the magnitude of the larger coordinate of the pair
    sw = (t("src_pcd") @ t("rot").T + t("trans").T).abs().max(1)[0]
    tw = t("tgt_pcd").abs().max(1)[0]
    si, ti, corr = keep["src_idx"], keep["tgt_idx"], t("correspondence")
    mag_sal = torch.cat((torch.maximum(sw[si], tw[ti][keep["row_arg"]]), torch.maximum(tw[ti], sw[si][keep["col_arg"]])))
    assert bool(((keep["saliency_dist"] - KITTI["matchability_radius"]).abs() > 4 * eps * mag_sal).all()), name
    mag_c = torch.maximum(sw[corr[:, 0]], tw[corr[:, 1]])
    assert bool(((keep["c_dist"] - (KITTI["pos_radius"] - 0.001)).abs() > 4 * eps * mag_c).all()), name
    cd = keep["coords_dist"]
    # the P x P masks: the anchors' own coordinates bound the rounding of each entry
    ch = keep["choice"]
    sel = torch.nonzero(keep["c_dist"] < KITTI["pos_radius"] - 0.001).flatten()
    sel = sel if ch is None else sel[torch.as_tensor(np.asarray(ch))]
    mag_pp = torch.maximum(sw[corr[sel, 0]][:, None], tw[corr[sel, 1]][None, :])
    for r in (KITTI["pos_radius"], KITTI["safe_radius"]):
        assert bool(((cd - r).abs() > 4 * eps * mag_pp).all()), (name, r)
    exact = 0
    for top in (keep["scores"].topk(2, dim=1)[0].T, keep["scores"].topk(2, dim=0)[0]):
        gap = top[0] - top[1]
        assert int(((gap < 8 * eps) & (gap != 0)).sum()) == 0, (name, "a near tie that is not exact")
        exact += int((gap == 0).sum())
    assert (exact >= 1) if planted_tie else (exact == 0), (name, "exact ties", exact)
    return keep["n_filtered"]


def main():
    ref = reference_loss()
    out = {}
    info = {}
    for name, make, tie in (("kitti", case_kitti, False), ("short", case_short, True), ("cluster", case_cluster, False)):
        inp = make()
        n_f = check_margins(name, inp, tie)
        for k, v in inp.items():
            out[f"{name}/in/{k}"] = v.astype(np.int32) if k == "correspondence" else v
        for leg, dtype in (("fp64", torch.float64), ("fp32", torch.float32)):
            res = run_leg(ref, inp, dtype, seed=77)
            for k, v in res.items():
                if k in ("grad_src_feats", "grad_tgt_feats"):
                    rows = np.flatnonzero(np.abs(v).sum(1) > 0)
                    if leg == "fp64":
                        out[f"{name}/{leg}/{k}_rows"], out[f"{name}/{leg}/{k}"] = rows.astype(np.int32), v[rows]
                    else:                                      # the fp32 leg is there for scale: its distance from the yardstick
                        full = np.zeros_like(v)
                        full[out[f"{name}/fp64/{k}_rows"]] = out[f"{name}/fp64/{k}"]
                        out[f"{name}/{leg}/{k}_rel_l2_vs_fp64"] = np.array(np.linalg.norm(v - full) / np.linalg.norm(full))
                elif leg == "fp32" and k.startswith("grad_"):
                    g64 = out[f"{name}/fp64/{k}"]
                    out[f"{name}/{leg}/{k}_rel_l2_vs_fp64"] = np.array(np.linalg.norm(v - g64) / np.linalg.norm(g64))
                else:
                    out[f"{name}/{leg}/{k}"] = v
        # the draw of :157 as the reference made it (same seed, same count)
        np.random.seed(77)
        out[f"{name}/choice"] = (np.random.permutation(n_f)[:KITTI["max_points"]] if n_f > KITTI["max_points"]
                                 else np.arange(n_f)).astype(np.int64)
        out[f"{name}/n_filtered"] = np.array(n_f)
        info[name] = dict(n=(len(inp["src_pcd"]), len(inp["tgt_pcd"])), corr=len(inp["correspondence"]),
                          unique=(len(np.unique(inp["correspondence"][:, 0])), len(np.unique(inp["correspondence"][:, 1]))),
                          filtered=n_f, circle=float(out[f"{name}/fp64/circle_loss"]), recall=float(out[f"{name}/fp64/recall"]),
                          fp32_circle_err=abs(float(out[f"{name}/fp32/circle_loss"]) / float(out[f"{name}/fp64/circle_loss"]) - 1),
                          fp32_grad_err=float(out[f"{name}/fp32/grad_src_feats_rel_l2_vs_fp64"]))
    p, gt = case_bce()
    out["bce/in/prediction"], out["bce/in/gt"] = p, gt
    for leg, dtype in (("fp64", torch.float64), ("fp32", torch.float32)):
        x = torch.from_numpy(p.astype(np.float64)).to(dtype).requires_grad_(True)
        loss, prec, rec = ref.get_weighted_bce_loss(x, torch.from_numpy(gt.astype(np.float64)).to(dtype))
        loss.backward()
        out[f"bce/{leg}/loss"], out[f"bce/{leg}/precision"], out[f"bce/{leg}/recall"] = (np.array(float(v), np.float64)
                                                                                      for v in (loss, prec, rec))
        if leg == "fp64":
            out[f"bce/{leg}/grad"] = x.grad.numpy().astype(np.float64)
    path = os.path.join(HERE, "predator_loss_ref.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1_000_000, size
    print(f"wrote predator_loss_ref.npz ({size / 1e6:.2f} MB)")
    for k, v in info.items():
        print(k, v)


if __name__ == "__main__":
    sys.exit(main())
