"""Reference-pinned fixture of the host arithmetic and the NumPy draws of FCGF_APR's two test scripts:
tests/golden/fcgf_tester_ref.npz.

Run where the reference checkout is present:
    python tests/golden/make_fcgf_tester_ref_golden.py

Same rule as make_predator_tester_ref_golden.py: the pieces are cut out of the reference's files with `ast`, compiled
unchanged and executed on CPU tensors; the text is not edited.  From scripts/test_apr.py: `find_corr`, `evaluate_nn_dist`,
`apply_transform`, and of `main`'s per-pair loop the statement that forms `dist_gth` (:123) and the statements from
`rte = ...` to `list_rre.append(rre)` (:162-186); from scripts/test_fcgf.py: `random_sample`; from lib/eval.py:
`find_nn_gpu`; from lib/metrics.py: `pdist`; from lib/timer.py: `AverageMeter`.  `np` in `find_corr`'s and
`random_sample`'s namespace is a proxy whose `random.choice` / `random.permutation` are NumPy's and record what they
return.  Only numbers are stored (allow_pickle=False).

Summary cases (float32 poses in, the reference's meters and lists out)
  mix        8 pairs: successes, RTE-only, RRE-only and double failures
  threshold  pair 0's RTE is exactly 2.0 (strict <: a failure), pair 2's its lower float32 neighbour (a success; along z, where
             t_gt is 0 and the offset survives the addition), two clean ones
  nan        estimates bit-identical to their float32 ground truth for which the reference's own RRE statement returns NaN
             (found by a seeded search) beside one for which it returns 0: the NaN pairs are booked as failures
  allfail    3 pairs failing both flags: no meter but `success` is updated (avg 0; the reference has no `var` then: NaN)
  single     one successful pair

Draw cases (rows of the two clouds, subsample_size, n_points): per case both scripts' draws after `np.random.seed`, the
pair's `dists_nn` row, and one `np.random.random()` taken after the calls as a stream sentinel per script
  both       70, 64 rows, 50, 50: find_corr draws both sides; random_sample cuts both sides down
  none       40, 90 rows: find_corr does not draw (40 <= 50); random_sample pads side 0 (n < N) and cuts side 1
  equal      50, 50 rows: nothing is drawn at all
  short1     60, 30 rows: find_corr draws 50 of 60 and all 30 of 30 (a permutation); random_sample cuts side 0, pads side 1
"""
import ast
import logging
import os
import textwrap
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/FCGF_APR"
METERS = ("success", "rte", "rre")


def _function(path, name, cls=False):
    src = open(path, encoding="utf-8").read()
    kind = ast.ClassDef if cls else ast.FunctionDef
    fn = [n for n in ast.parse(src).body if isinstance(n, kind) and n.name == name][0]
    return textwrap.dedent("\n".join(src.splitlines()[fn.lineno - 1:fn.end_lineno]))


def _loop_statements():
    """-> (the `dist_gth = ...` statement, the statements `rte = ...` .. `list_rre.append(rre)`) of test_apr.py's main."""
    path = f"{REF}/scripts/test_apr.py"
    src = open(path, encoding="utf-8").read()
    main = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "main"][0]
    loop = [n for n in main.body if isinstance(n, ast.For)][0]
    target = lambda n: getattr(n.targets[0], "id", "") if isinstance(n, ast.Assign) else ""
    dist = [n for n in loop.body if target(n) == "dist_gth"][0]
    first = [i for i, n in enumerate(loop.body) if target(n) == "rte"][0]
    last = [i for i, n in enumerate(loop.body) if isinstance(n, ast.Expr) and isinstance(n.value, ast.Call)
            and getattr(n.value.func, "attr", "") == "append" and getattr(n.value.func.value, "id", "") == "list_rre"][0]
    lines = src.splitlines()
    cut = lambda a, b: textwrap.dedent("\n".join(lines[a.lineno - 1:b.end_lineno]))
    assert (dist.lineno, loop.body[first].lineno, loop.body[last].end_lineno) == (123, 162, 186)
    return cut(dist, dist), cut(loop.body[first], loop.body[last])


class _RecordingRandom:
    def __init__(self):
        self.drawn = []

    def choice(self, *a, **k):
        self.drawn.append(np.random.choice(*a, **k))
        return self.drawn[-1]

    def permutation(self, *a, **k):
        self.drawn.append(np.random.permutation(*a, **k))
        return self.drawn[-1]


class _NumpyRecordingDraws:
    """`np` for the reference's text: everything is NumPy's, `random` records what its two draw functions return."""

    def __init__(self):
        self.random = _RecordingRandom()

    def __getattr__(self, name):
        return getattr(np, name)


def reference_pieces():
    p = {"dist_gth": None}
    p["dist_gth"], p["tail"] = _loop_statements()
    p["meter"] = _function(f"{REF}/lib/timer.py", "AverageMeter", cls=True)
    p["corr"] = "\n\n".join([_function(f"{REF}/lib/metrics.py", "pdist"), _function(f"{REF}/lib/eval.py", "find_nn_gpu"),
                             _function(f"{REF}/scripts/test_apr.py", "find_corr"),
                             _function(f"{REF}/scripts/test_apr.py", "apply_transform"),
                             _function(f"{REF}/scripts/test_apr.py", "evaluate_nn_dist")])
    p["sample"] = _function(f"{REF}/scripts/test_fcgf.py", "random_sample")
    return p


def run_summary(p, T_est, T_gt, rte_thresh=2, rre_thresh=5):
    """The reference's statements per pair on float32 torch tensors, as the scripts hold them."""
    ns = {"np": np, "logging": logging.getLogger("fcgf_tester_ref")}
    exec(compile(p["meter"], f"{REF}/lib/timer.py:AverageMeter", "exec"), ns)
    M = ns["AverageMeter"]
    ns.update(success_meter=M(), rte_meter=M(), rre_meter=M(), dists_success=[], dists_fail=[], list_rte=[], list_rre=[],
              rte_thresh=rte_thresh, rre_thresh=rre_thresh)
    head = compile(p["dist_gth"], f"{REF}/scripts/test_apr.py:123", "exec")
    tail = compile(p["tail"], f"{REF}/scripts/test_apr.py:162-186", "exec")
    trans_gt = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for E, G in zip(T_est, T_gt):
            ns["T_ransac"], ns["T_gth"] = torch.from_numpy(E.copy()), torch.from_numpy(G.copy())
            exec(head, ns)
            trans_gt.append(ns["dist_gth"])
            exec(tail, ns)
    out = {}
    for name in METERS:
        m = ns[name + "_meter"]
        out[name] = np.array([m.sum, m.count, m.avg, getattr(m, "var", np.nan)], np.float64)
    f32 = lambda v: np.asarray(v, dtype=np.float32)
    out.update(dists_success=f32(ns["dists_success"]), dists_fail=f32(ns["dists_fail"]), list_rte=f32(ns["list_rte"]),
               list_rre=f32(ns["list_rre"]), dists=f32(trans_gt))
    assert all(np.asarray(v).dtype == np.float32 for v in ns["list_rte"] + ns["list_rre"] + trans_gt)
    return out


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def make_case(seed, rot_err_deg, trans_err, exact=False):
    """Ground truth like synth.make_pair's (5 .. 20 m along x, some yaw) in float32; the estimate of pair i is a rotation by
    rot_err_deg[i] about z in front of it with the translation moved by trans_err[i] along axis i % 3, rounded to float32.
    `exact`: identity rotations and whole-metre translations, so that float32(2.0) along x is an RTE of exactly 2.0."""
    rng = np.random.default_rng(seed)
    n = len(rot_err_deg)
    T_gt = np.stack([pose(np.eye(3) if exact else rot(2, rng.uniform(-15, 15)) @ rot(0, rng.uniform(-2, 2)),
                          [rng.uniform(5, 20), rng.uniform(-1, 1), rng.uniform(-0.2, 0.2)]) for _ in range(n)]).astype(np.float32)
    if exact:
        T_gt[:, :3, 3] = np.round(T_gt[:, :3, 3])
    T_est = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    for i in range(n):
        axis = np.zeros(3, np.float32)
        axis[i % 3] = 1
        T_est[i, :3, :3] = (rot(2, rot_err_deg[i]) @ T_gt[i, :3, :3].astype(np.float64)).astype(np.float32)
        T_est[i, :3, 3] = T_gt[i, :3, 3] + np.float32(trans_err[i]) * axis
    return T_est, T_gt


def nan_case(p, want=3):
    """Seeded search: float32 rotations R with arccos((trace(R^T R) - 1) / 2) NaN in the reference's own arithmetic."""
    rng = np.random.default_rng(7)
    found, zero = [], None
    while len(found) < want or zero is None:
        T = pose(rot(2, rng.uniform(-180, 180)) @ rot(1, rng.uniform(-90, 90)) @ rot(0, rng.uniform(-180, 180)),
                 [rng.uniform(5, 20), rng.uniform(-1, 1), rng.uniform(-0.2, 0.2)]).astype(np.float32)
        rre = run_summary(p, T[None], T[None])["list_rre"][0]
        if np.isnan(rre) and len(found) < want:
            found.append(T)
        elif rre == 0 and zero is None:
            zero = T
    T_gt = np.stack(found[:2] + [zero] + found[2:])
    return T_gt.copy(), T_gt


SUMMARY_CASES = {
    "mix": dict(seed=1, rot_err_deg=[0.3, 1.2, 7.5, 0.8, 40.0, 2.5, 4.9, 170.0], trans_err=[0.1, 0.5, 0.2, 3.0, 9.0, 1.9, 2.5, 0.05]),
    "threshold": dict(seed=2, rot_err_deg=[0.5, 0.2, 0.1, 0.4], trans_err=[2.0, 0.3, np.nextafter(np.float32(2.0), np.float32(0.0)), 0.1],
                      exact=True),
    "allfail": dict(seed=3, rot_err_deg=[12.0, 90.0, 6.0], trans_err=[2.5, 4.0, 30.0]),
    "single": dict(seed=4, rot_err_deg=[0.7], trans_err=[0.4]),
}

DRAW_CASES = {"both": (70, 64), "none": (40, 90), "equal": (50, 50), "short1": (60, 30)}
SUBSAMPLE, N_POINTS, CHANNELS = 50, 50, 8


def run_draws(p, name, n0, n1):
    rng = np.random.default_rng(sum(map(ord, name)))
    xyz0 = rng.uniform(-10, 10, (n0, 3)).astype(np.float32)
    T = pose(rot(2, 9.0) @ rot(0, 1.0), [7.0, -0.5, 0.1]).astype(np.float32)
    moved = xyz0.astype(np.float64) @ T[:3, :3].T.astype(np.float64) + T[:3, 3]
    xyz1 = (moved[rng.integers(0, n0, n1)] + rng.normal(0, 0.2, (n1, 3))).astype(np.float32)
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    F0, F1 = unit(rng.standard_normal((n0, CHANNELS))), unit(rng.standard_normal((n1, CHANNELS)))
    out = dict(xyz0=xyz0, xyz1=xyz1, F0=F0, F1=F1, T_gt=T, seed=np.int64(n0 * 1000 + n1))
    t = torch.from_numpy
    empty = np.zeros(0, np.int64)
    for script in ("apr", "fcgf"):
        proxy = _NumpyRecordingDraws()
        ns = {"np": proxy, "torch": torch}
        exec(compile(p["corr"], f"{REF}:find_corr", "exec"), ns)
        exec(compile(p["sample"], f"{REF}/scripts/test_fcgf.py:random_sample", "exec"), ns)
        np.random.seed(int(out["seed"]))
        c0, c1 = ns["find_corr"](t(xyz0), t(xyz1), t(F0), t(F1), subsample_size=SUBSAMPLE)
        dists = np.asarray(ns["evaluate_nn_dist"](c0, c1, t(T)), dtype=np.float32)
        drawn = list(proxy.random.drawn)
        assert len(drawn) == (2 if n0 > SUBSAMPLE else 0)
        inds0, inds1 = drawn if drawn else (empty, empty)
        # find_corr keeps its nearest-neighbour indices to itself: the same cut-out search on the same rows
        nn = ns["find_nn_gpu"](t(F0)[inds0] if drawn else t(F0), t(F1)[inds1] if drawn else t(F1), nn_max_n=500).numpy()
        assert np.array_equal(c1.numpy(), xyz1[inds1[nn]] if drawn else xyz1[nn])
        if script == "apr":
            out.update(inds0=inds0, inds1=inds1, nn=nn, dists_nn=dists)
        else:
            assert np.array_equal(out["inds0"], inds0) and np.array_equal(out["dists_nn"], dists)
            proxy.random.drawn.clear()
            a0, G0 = ns["random_sample"](xyz0, t(F0), N_POINTS)
            a1, G1 = ns["random_sample"](xyz1, t(F1), N_POINTS)
            ch = list(proxy.random.drawn)
            assert len(a0) == len(a1) == N_POINTS and len(ch) == (n0 != N_POINTS) + (n1 != N_POINTS)
            out["choice0"] = ch.pop(0)[:N_POINTS] if n0 != N_POINTS else empty
            out["choice1"] = ch.pop(0)[:N_POINTS] if n1 != N_POINTS else empty
            assert n0 == N_POINTS or np.array_equal(a0, xyz0[out["choice0"]])
            assert n1 == N_POINTS or (np.array_equal(a1, xyz1[out["choice1"]]) and np.array_equal(G1.numpy(), F1[out["choice1"]]))
        out["sentinel_" + script] = np.float64(np.random.random())
    return {k: np.asarray(v) for k, v in out.items()}


def main():
    p = reference_pieces()
    store = {"summary_names": np.array(list(SUMMARY_CASES) + ["nan"]), "draw_names": np.array(list(DRAW_CASES)),
             "draw_sizes": np.array([SUBSAMPLE, N_POINTS], np.int64)}
    cases = {}
    for name, spec in SUMMARY_CASES.items():
        spec = dict(spec)
        cases[name] = make_case(spec.pop("seed"), **spec)
    cases["nan"] = nan_case(p)
    for name, (T_est, T_gt) in cases.items():
        out = run_summary(p, T_est, T_gt)
        if name == "threshold":      # the case is what it says only if the reference itself sees exactly 2.0 m and fails it
            assert out["list_rte"][0] == 2.0 and out["list_rte"][2] < 2.0 and out["list_rte"][2] == np.nextafter(np.float32(2), np.float32(0))
            assert out["dists"][0] in out["dists_fail"] and out["dists"][2] in out["dists_success"]
            assert out["success"][0] == 3 and out["rte"][1] == 3 and out["rre"][1] == 4
        if name == "nan":
            assert T_est.tobytes() == T_gt.tobytes()
            nan = np.isnan(out["list_rre"])
            assert list(nan) == [True, True, False, True] and out["list_rre"][2] == 0
            assert out["success"][0] == 1 and out["success"][1] == 4 and len(out["dists_fail"]) == 3
            assert np.array_equal(out["dists_fail"], out["dists"][nan]) and (out["list_rte"] == 0).all()
        if name == "mix":
            ok_t, ok_r = out["list_rte"] < 2, out["list_rre"] < np.pi / 180 * 5
            assert (ok_t & ok_r).any() and (ok_t & ~ok_r).any() and (~ok_t & ok_r).any() and (~ok_t & ~ok_r).any()
        if name == "allfail":
            assert out["success"][0] == 0 and out["rte"][1] == 0 and out["rre"][1] == 0
        print(name, {k: out[k].tolist() for k in METERS}, "rte", out["list_rte"], "rre", out["list_rre"])
        store[f"{name}.T_est"], store[f"{name}.T_gt"] = T_est, T_gt
        for k, v in out.items():
            store[f"{name}.{k}"] = v
    for name, (n0, n1) in DRAW_CASES.items():
        out = run_draws(p, name, n0, n1)
        print(name, {k: (v.shape if v.ndim else v.item()) for k, v in out.items()})
        for k, v in out.items():
            store[f"draw.{name}.{k}"] = v
    path = os.path.join(HERE, "fcgf_tester_ref.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
