"""Reference-pinned fixture of the two formulas around the multiway registration: tests/golden/multiway_ref.npz.

Run where the reference checkout is present:
    python tests/golden/make_multiway_ref_golden.py

Same rule as the other make_*_ref_golden.py scripts: the statements are cut out of the reference's file with `ast`, compiled
unchanged and executed on seeded inputs; the text is not edited and only numeric arrays are stored (allow_pickle=False).
  * `M = (self.velo2cam @ pos_source.T @ np.linalg.inv(pos_target.T) @ np.linalg.inv(self.velo2cam)).T`, the ICP init of
    pairwise_registration (FCGF_APR/lib/complement_data_loader.py:410-411, Predator_APR/datasets/kitti.py:199-200);
  * `listMs = [np.linalg.inv(listM_left[0]) @ listM_left[i] ...] + [... listM_right ...]`, the poses multiway_registration
    hands out (:508-509, kitti.py:297-298).
Both files are executed and must agree bit for bit.  Inputs: a KITTI-like velo2cam (a rotation that swaps the axes plus a
small offset), k + 1 = 4 odometry positions per side about a metre and a degree apart, and two lists of four rigid poses.
"""
import ast
import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REFS = ("/root/reference/FCGF_APR/lib/complement_data_loader.py", "/root/reference/Predator_APR/datasets/kitti.py")


def statement(path, function, target):
    """The source text of the LAST assignment to `target` directly in the body of the method `function`."""
    src = open(path, encoding="utf-8").read()
    lines = src.splitlines()
    found = None
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.FunctionDef) and node.name == function:
            for st in node.body:
                if isinstance(st, ast.Assign) and any(isinstance(t, ast.Name) and t.id == target for t in st.targets):
                    found = textwrap.dedent("\n".join(lines[st.lineno - 1:st.end_lineno]))
    assert found is not None, (path, function, target)
    return found


def rigid(rng, trans, deg):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    P = np.eye(4)
    P[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    P[:3, 3] = rng.normal(size=3) * trans
    return P


def main():
    rng = np.random.default_rng(16)
    velo2cam = np.eye(4)
    velo2cam[:3, :3] = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]) @ rigid(rng, 0.0, 0.8)[:3, :3]
    velo2cam[:3, 3] = [-0.004, -0.076, -0.272]
    pos = [np.eye(4)]
    for _ in range(6):
        pos.append(pos[-1] @ rigid(rng, 1.0, 1.5))
    pos = np.stack(pos)
    left = np.stack([rigid(rng, 2.0, 3.0) for _ in range(4)])
    right = np.stack([rigid(rng, 2.0, 3.0) for _ in range(4)])
    pairs = np.array([(s, t) for s in range(len(pos)) for t in range(len(pos)) if s != t], dtype=np.int64)
    results = []
    for path in REFS:
        init_src = statement(path, "pairwise_registration", "M")
        prod_src = statement(path, "multiway_registration", "listMs")
        holder = types.SimpleNamespace(velo2cam=velo2cam)
        inits = []
        for s, t in pairs:
            ns = {"np": np, "self": holder, "pos_source": pos[s], "pos_target": pos[t]}
            exec(compile(init_src, f"{path}:pairwise_registration", "exec"), ns)
            inits.append(ns["M"])
        ns = {"np": np, "listM_left": list(left), "listM_right": list(right)}
        exec(compile(prod_src, f"{path}:multiway_registration", "exec"), ns)
        results.append((np.stack(inits), np.stack(ns["listMs"])))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    path = os.path.join(HERE, "multiway_ref.npz")
    np.savez_compressed(path, velo2cam=velo2cam, pos=pos, pairs=pairs, inits=results[0][0], left=left, right=right,
                        products=results[0][1])
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
