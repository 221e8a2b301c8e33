"""Reference-pinned fixture of Predator_APR's mutual matching and inlier ratios: tests/golden/predator_mutual_ref.npz.

Run where the reference checkout is present:
    python tests/golden/make_predator_mutual_ref_golden.py

Same rule as make_predator_ref_golden.py: `mutual_selection`, `get_inlier_ratio`, `to_tensor` and `to_array`
(Predator_APR/lib/benchmark_utils.py:76-95, :227-295) are cut out of the reference's file with `ast`, compiled unchanged and
executed on seeded inputs, on the CPU: the name `torch` in the execution namespace is a proxy whose
`cuda.device_count()` answers 0, and where the installed NumPy has no `np.bool` the name `np` is a proxy that supplies the
alias.  The text is not edited.  Only numeric arrays are stored (allow_pickle=False).

Cases (descriptors: L2-normalised float32 rows, d = 32; about a third of the source rows have a planted true match: a
target row that is the source row plus noise, at the transformed position plus noise)
  odd      300 x 257: neither a multiple of 16 or 64 (partial tiles of the arg-max kernel, partial block of the scan)
  one      1 x 1,  row 1 x 40,  col 40 x 1
  ties     70 x 70 with three duplicated target rows and three duplicated source rows, each duplicate of a planted match:
           the tie rule (lowest index, np.argmax) decides on both axes
  pose     400 x 380 in a 20 m cube: the pair of the pair-list RANSAC test

Conditions (asserted here in float64 for EVERY row and column; a seed is kept only if the reference alone satisfies them)
  * outside the planted ties the best and the second-best score of every row and every column differ by >= 1e-4 (float32
    rounding of a 32-term unit-norm dot product stays below ~4e-6: no arithmetic flips an arg-max);
  * the planted ties are exact in the reference's own float32 score matrix;
  * no `wo` and no `w` distance lies within 1e-5 of the threshold.
"""
import ast
import os
import sys
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference/Predator_APR/lib/benchmark_utils.py"
NAMES = ("to_tensor", "to_array", "get_inlier_ratio", "mutual_selection")
THRESHOLD = 0.1
GAP = 1e-4
MARGIN = 1e-5


class _Cuda:
    def __getattr__(self, name):
        return getattr(torch.cuda, name)

    @staticmethod
    def device_count():
        return 0


class _TorchOnCpu:
    """`torch` for the reference's text: everything is torch's, `cuda.device_count()` answers 0."""
    cuda = _Cuda()

    def __getattr__(self, name):
        return getattr(torch, name)


class _NumpyWithBool:
    """`np` for the reference's text on a NumPy without the `np.bool` alias."""
    bool = bool

    def __getattr__(self, name):
        return getattr(np, name)


def reference_namespace():
    src = open(REF, encoding="utf-8").read()
    found = {n.name: textwrap.dedent("\n".join(src.splitlines()[n.lineno - 1:n.end_lineno]))
             for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in NAMES}
    assert set(found) == set(NAMES), set(NAMES) - set(found)
    ns = {"torch": _TorchOnCpu(), "np": np if hasattr(np, "bool") else _NumpyWithBool()}
    for name in NAMES:
        exec(compile(found[name], f"{REF}:{name}", "exec"), ns)
    return ns


def make_inputs(seed, n, m, extent, dup_tgt=0, dup_src=0):
    rng = np.random.default_rng(seed)
    unit = lambda f: (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)
    src_feat = unit(rng.standard_normal((n, 32)))
    tgt_feat = unit(rng.standard_normal((m, 32)))
    src = rng.uniform(-extent, extent, (n, 3)).astype(np.float32)
    tgt = rng.uniform(-extent, extent, (m, 3)).astype(np.float32)
    a, b = np.deg2rad(rng.uniform(-25, 25)), np.deg2rad(rng.uniform(-10, 10))
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    rot = (Rz @ Rx).astype(np.float32)
    trans = rng.uniform(-1, 1, (3, 1)).astype(np.float32)
    k = max(1, int(round(min(n, m) / 3)))
    pi, pj = np.sort(rng.choice(n, k, replace=False)), rng.choice(m, k, replace=False)
    tgt_feat[pj] = unit(src_feat[pi] + 0.03 * rng.standard_normal((k, 32)))
    tgt[pj] = (src[pi].astype(np.float64) @ rot.astype(np.float64).T + trans[:, 0] + rng.normal(0, 0.02, (k, 3))).astype(np.float32)
    planted = np.stack([pi, pj], 1).astype(np.int64)
    dups = []                                   # (axis, original, duplicate): axis 1 = target rows, 0 = source rows
    free_t = np.setdiff1d(np.arange(m), pj)
    free_s = np.setdiff1d(np.arange(n), pi)
    for d in range(dup_tgt):                    # a second target row with the descriptor of a planted partner
        j1, j2 = int(pj[d]), int(free_t[d])
        tgt_feat[j2] = tgt_feat[j1]
        dups.append((1, j1, j2))
    for d in range(dup_src):                    # a second source row with the descriptor of a planted source row
        i1, i2 = int(pi[k - 1 - d]), int(free_s[d])
        src_feat[i2] = src_feat[i1]
        dups.append((0, i1, i2))
    return dict(src_pcd=src, tgt_pcd=tgt, src_feat=src_feat, tgt_feat=tgt_feat, rot=rot, trans=trans, planted=planted,
                dups=np.array(dups, dtype=np.int64).reshape(-1, 3))


def top_two_gap(scores64, feat_other):
    """Per row of scores64: best minus the best among the columns whose descriptor differs from the winner's (the planted
    duplicates are bitwise copies); inf where there is no such column."""
    arg = scores64.argmax(1)
    same = (feat_other[None, :, :] == feat_other[arg][:, None, :]).all(2)
    rest = np.where(same, -np.inf, scores64)
    return scores64.max(1) - rest.max(1)


def conditions(c, res, scores32):
    """The three conditions of the docstring -> list of violations (empty: the case is kept)."""
    bad = []
    s64 = c["src_feat"].astype(np.float64) @ c["tgt_feat"].astype(np.float64).T
    if min(top_two_gap(s64, c["tgt_feat"]).min(), top_two_gap(s64.T, c["src_feat"]).min()) < GAP:
        bad.append("gap")
    for axis, a, b in c["dups"]:
        same = np.array_equal(scores32[:, a], scores32[:, b]) if axis == 1 else np.array_equal(scores32[a], scores32[b])
        if not same:
            bad.append("tie not exact")
    p = c["src_pcd"].astype(np.float64) @ c["rot"].astype(np.float64).T + c["trans"][:, 0].astype(np.float64)
    t = c["tgt_pcd"].astype(np.float64)
    d_wo = np.linalg.norm(p - t[s64.argmax(1)], axis=1)
    d_w = np.linalg.norm(p[res["row_sel"]] - t[res["col_sel"]], axis=1)
    if np.abs(d_wo - THRESHOLD).min() < MARGIN or np.abs(d_w - THRESHOLD).min() < MARGIN:
        bad.append("threshold margin")
    return bad


def run_reference(ns, c):
    out = ns["get_inlier_ratio"](c["src_pcd"], c["tgt_pcd"], c["src_feat"], c["tgt_feat"], c["rot"], c["trans"], THRESHOLD)
    scores = torch.matmul(torch.from_numpy(c["src_feat"]), torch.from_numpy(c["tgt_feat"]).transpose(0, 1))   # :199, :247
    mask = ns["mutual_selection"](scores[None, :, :])
    assert mask.dtype == np.bool_ and mask.shape == (1,) + tuple(scores.shape)
    row_sel, col_sel = np.where(mask[0])
    res = dict(mask=mask[0], row_sel=row_sel.astype(np.int64), col_sel=col_sel.astype(np.int64),
               dist_wo=out["wo"]["distance"], dist_w=out["w"]["distance"],
               ratio_wo=np.float32(out["wo"]["inlier_ratio"]), ratio_w=np.float32(out["w"]["inlier_ratio"]))
    assert res["dist_wo"].dtype == np.float32 and res["dist_w"].dtype == np.float32
    assert out["wo"]["inlier_ratio"].dtype == torch.float32 and out["wo"]["inlier_ratio"].dim() == 0
    return res, scores.numpy()


CASES = [("odd", 300, 257, 3.0, 0, 0), ("one", 1, 1, 3.0, 0, 0), ("row", 1, 40, 3.0, 0, 0), ("col", 40, 1, 3.0, 0, 0),
         ("ties", 70, 70, 3.0, 3, 3), ("pose", 400, 380, 10.0, 0, 0)]


def main():
    ns = reference_namespace()
    store = {"threshold": np.float32(THRESHOLD), "names": np.array([c[0] for c in CASES])}
    for name, n, m, extent, dt, ds in CASES:
        for seed in range(1000):
            c = make_inputs(seed, n, m, extent, dt, ds)
            res, scores32 = run_reference(ns, c)
            bad = conditions(c, res, scores32)
            if not bad:
                break
            print(f"{name}: seed {seed} rejected ({', '.join(bad)})")
        else:
            raise SystemExit(f"{name}: no seed satisfies the conditions")
        assert len(c["dups"]) == dt + ds
        print(f"{name}: seed {seed}, {len(res['row_sel'])} mutual pairs, ratio wo {float(res['ratio_wo']):.4f} "
              f"w {float(res['ratio_w']):.4f}")
        store[f"{name}.seed"] = np.int64(seed)
        for k, v in c.items():
            store[f"{name}.{k}"] = v
        for k, v in res.items():
            store[f"{name}.{k}"] = v
    path = os.path.join(HERE, "predator_mutual_ref.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
