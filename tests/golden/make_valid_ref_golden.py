"""Reference-pinned fixture for the matching half of a validation pair (tests/golden/valid_ref.npz).

Run in the build container only (needs /root/reference):   python tests/golden/make_valid_ref_golden.py

As tests/golden/make_fcgf_ref_golden.py does, the reference's source is parsed with `ast` and its own text is compiled
and executed here, nothing is re-typed and nothing but arrays is stored:

  find_corr, evaluate_hit_ratio, apply_transform   FCGF_APR/lib/complement_trainer.py:214-247   (methods, stub `self`)
  find_nn_gpu                                      FCGF_APR/lib/eval.py:18-48                   (function)
  est_quad_linear_robust + helpers                 FCGF_APR/util/transform_estimation.py:5-116  (functions)
  corr_dist, pdist                                 FCGF_APR/lib/metrics.py                      (imported)
  AverageMeter                                     FCGF_APR/lib/timer.py                        (imported)
  T_est = ... ; loss ... feat_match_ratio.update   FCGF_APR/lib/complement_trainer.py:557-571   (statements of
                                                   GenerativePairTrainer._valid_epoch, executed in order)

Input: ~3000 rows per side, ground truth of a few metres and degrees, features = a smooth function of the scene position
plus noise, so that roughly a third of the feature nearest neighbours are the true partner.  find_corr is called with a
subsample size below the row count so that its two draws happen (the trainer passes 5000 to clouds of ~14 k voxels).
The script checks what tests/test_valid_pair_gpu.py relies on: few correspondences within 1e-5 of the hit threshold, a
pose error above 0.5 degrees.
"""
import ast
import importlib.util
import os
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/FCGF_APR"
SEED, SUBSAMPLE, HIT_THRESH, NOISE = 20, 2000, 0.1, 0.4


def _tree(rel):
    src = open(os.path.join(REF, rel), encoding="utf-8").read()
    return src, ast.parse(src)


def _defs(rel, names, ns, cls=None):
    src, tree = _tree(rel)
    body = tree.body
    if cls is not None:
        body = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    found = {}
    for node in body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            found[node.name] = textwrap.dedent("\n".join(src.splitlines()[node.lineno - 1:node.end_lineno]))
    missing = set(names) - set(found)
    assert not missing, f"{rel}: {missing} not found"
    for name in names:
        exec(compile(found[name], f"{REF}/{rel}:{name}", "exec"), ns)
    return ns


def _import(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _valid_statements():
    """The statements of the pair loop of GenerativePairTrainer._valid_epoch from `T_est = ...` to
    `feat_match_ratio.update(...)`, dedented, in source order."""
    rel = "lib/complement_trainer.py"
    src, tree = _tree(rel)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "GenerativePairTrainer")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "_valid_epoch")
    loop = next(n for n in fn.body if isinstance(n, ast.For))
    texts = [ast.unparse(n) for n in loop.body]
    a = next(i for i, t in enumerate(texts) if t.startswith("T_est ="))
    b = next(i for i, t in enumerate(texts) if t.startswith("feat_match_ratio.update"))
    lines = src.splitlines()
    return [(textwrap.dedent("\n".join(lines[n.lineno - 1:n.end_lineno])), n.lineno) for n in loop.body[a:b + 1]]


def _rot(deg_xyz):
    a, b, g = np.deg2rad(deg_xyz)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def make_inputs(rng):
    """The second cloud is the scene moved by T_true plus 2 cm of noise; the stored ground truth is T_true times a small
    pose offset (0.7 degrees, 2 cm), as a dataset's GPS / INS ground truth is off: the fitted pose then differs from T_gt
    by a well-resolved angle and only the correspondences near the origin are hits."""
    n0, n1, n, c = 3000, 2900, 3400, 16
    scene = np.concatenate([rng.uniform(-12, 12, (n, 2)), rng.uniform(-2, 3, (n, 1))], 1)
    T_true = np.eye(4)
    T_true[:3, :3] = _rot([4.0, -2.5, 9.0])
    T_true[:3, 3] = [3.2, -1.4, 0.35]
    off = np.eye(4)
    off[:3, :3] = _rot([0.3, -0.2, 0.6])
    off[:3, 3] = [0.015, -0.01, 0.005]
    T = off @ T_true
    i0, i1 = rng.permutation(n)[:n0], rng.permutation(n)[:n1]
    xyz0 = scene[i0].astype(np.float32)
    xyz1 = (scene[i1] @ T_true[:3, :3].T + T_true[:3, 3] + rng.normal(0, 0.02, (n1, 3))).astype(np.float32)
    freq = rng.normal(0, 1.2, (3, c))
    phase = rng.uniform(0, 2 * np.pi, c)

    def feats(p):
        f = np.sin(p @ freq + phase) + rng.normal(0, NOISE, (len(p), c))
        return (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)

    return xyz0, xyz1, feats(scene[i0]), feats(scene[i1]), T.astype(np.float32), i0, i1


def main():
    rng = np.random.default_rng(SEED)
    xyz0, xyz1, F0, F1, T_gt, i0, i1 = make_inputs(rng)
    metrics = _import("lib/metrics.py", "ref_fcgf_metrics")
    timer = _import("lib/timer.py", "ref_fcgf_timer")
    te = _defs("util/transform_estimation.py",
               ["rot_x", "rot_y", "rot_z", "get_trans", "update_pcd", "build_linear_system", "solve_linear_system",
                "compute_weights", "est_quad_linear_robust"], {"torch": torch})
    ev = _defs("lib/eval.py", ["find_nn_gpu"], {"torch": torch, "np": np, "pdist": metrics.pdist})
    tr = _defs("lib/complement_trainer.py", ["find_corr", "apply_transform", "evaluate_hit_ratio"],
               {"np": np, "torch": torch, "find_nn_gpu": ev["find_nn_gpu"]}, cls="TwoStageTrainer")
    stub = types.SimpleNamespace(config=types.SimpleNamespace(nn_max_n=500, hit_ratio_thresh=HIT_THRESH))
    for name in ("find_corr", "apply_transform", "evaluate_hit_ratio"):
        setattr(stub, name, types.MethodType(tr[name], stub))
    t = torch.from_numpy
    np.random.seed(SEED)
    xyz0_corr, xyz1_corr = stub.find_corr(t(xyz0), t(xyz1), t(F0), t(F1), subsample_size=SUBSAMPLE)
    # the same two draws again, in the reference's order, and the NN on the sub-sampled features
    np.random.seed(SEED)
    inds0 = np.random.choice(len(F0), min(len(F0), SUBSAMPLE), replace=False)
    inds1 = np.random.choice(len(F1), min(len(F1), SUBSAMPLE), replace=False)
    nn = ev["find_nn_gpu"](t(F0[inds0]), t(F1[inds1]), nn_max_n=500).numpy()
    assert np.array_equal(xyz0_corr.numpy(), xyz0[inds0]) and np.array_equal(xyz1_corr.numpy(), xyz1[inds1[nn]])
    meters = {k: timer.AverageMeter() for k in ("loss_meter", "rte_meter", "rre_meter", "hit_ratio_meter", "feat_match_ratio")}
    ns = {"np": np, "torch": torch, "te": types.SimpleNamespace(est_quad_linear_robust=te["est_quad_linear_robust"]),
          "corr_dist": metrics.corr_dist, "self": stub, "xyz0": t(xyz0), "xyz1": t(xyz1), "T_gt": t(T_gt),
          "xyz0_corr": xyz0_corr, "xyz1_corr": xyz1_corr, **meters}
    for text, lineno in _valid_statements():
        exec(compile(text, f"{REF}/lib/complement_trainer.py:{lineno}", "exec"), ns)
    out = {"xyz0": xyz0, "xyz1": xyz1, "F0": F0, "F1": F1, "T_gt": T_gt, "seed": np.array(SEED),
           "subsample_size": np.array(SUBSAMPLE), "hit_thresh": np.array(HIT_THRESH), "inds0": inds0.astype(np.int64),
           "inds1": inds1.astype(np.int64), "nn": nn.astype(np.int64), "T_est": ns["T_est"].numpy(),
           "corr_dist": np.array(float(ns["loss"])), "rte": np.array(float(ns["rte"])), "rre": np.array(float(ns["rre"])),
           "hit_ratio": np.array(float(ns["hit_ratio"])), "feat_match": np.array(bool(meters["feat_match_ratio"].avg))}
    # what the GPU test relies on
    right = float(np.mean(i0[inds0] == i1[inds1[nn]]))
    p0, p1, Tg = xyz0[inds0].astype(np.float64), xyz1[inds1[nn]].astype(np.float64), T_gt.astype(np.float64)
    d = np.sqrt(((p0 @ Tg[:3, :3].T + Tg[:3, 3] - p1) ** 2).sum(1) + 1e-6)
    border = int((np.abs(d - HIT_THRESH) < 1e-5).sum())
    print(f"right NN {right:.3f}, borderline {border}, rre {np.degrees(float(ns['rre'])):.4f} deg, hit {float(ns['hit_ratio']):.4f}")
    assert border <= len(d) // 1000, border
    assert np.degrees(float(ns["rre"])) > 0.5, np.degrees(float(ns["rre"]))
    assert 0.2 < right < 0.5, right
    path = os.path.join(HERE, "valid_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote valid_ref.npz ({os.path.getsize(path) / 1e3:.0f} kB): right NN {right:.3f}, hit ratio {float(ns['hit_ratio']):.4f}, "
          f"borderline {border}, corr_dist {float(ns['loss']):.5f}, rte {float(ns['rte']):.5f} m, "
          f"rre {np.degrees(float(ns['rre'])):.4f} deg")


if __name__ == "__main__":
    sys.exit(main())
