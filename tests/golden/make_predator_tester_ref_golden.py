"""Reference-pinned fixture of the arithmetic Predator_APR's tester runs after its per-pair loop:
tests/golden/predator_tester_ref.npz.

Run where the reference checkout is present:
    python tests/golden/make_predator_tester_ref_golden.py

Same rule as make_predator_ref_golden.py: the statements of `KITTITester.test` behind its `with torch.no_grad()` loop
(Predator_APR/lib/tester.py:104-137: from `tsfm_est = np.array(tsfm_est)` to the last `errors[...] = ...`) and
`get_angle_deviation` (lib/benchmark_utils.py:170-185) are cut out of the reference's files with `ast`, compiled unchanged
and executed on the inputs below.  The text is not edited; `np` in its namespace is a proxy whose `savez` / `save` keep
what the reference would write instead of writing it, `self` carries the two thresholds.  Only numbers are stored
(allow_pickle=False): the inputs (float64 estimates; float32 ground truth, as the tester collects it from tensors) and
the outputs.

Cases
  mix        8 pairs: successes, rotation-only, translation-only and double failures
  threshold  a pair whose translation error is exactly 2 m (strict <: a failure), one whose rotation error rounds past 5
             degrees from a matrix built at exactly 5 degrees and its neighbours on both sides, and two clean successes
  allfail    3 pairs failing both flags: recall 0, all six statistics NaN
  single     one successful pair
"""
import ast
import os
import textwrap
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_TESTER = "/root/reference/Predator_APR/lib/tester.py"
REF_BU = "/root/reference/Predator_APR/lib/benchmark_utils.py"
ERRORS = ("rot_mean", "rot_median", "trans_rmse", "trans_rmedse", "rot_std", "trans_std")


class _NumpyNoFiles:
    """`np` for the reference's text: everything is NumPy's, `savez` / `save` record their arguments."""

    def __init__(self):
        self.saved = {}

    def savez(self, path, **arrays):
        self.saved[os.path.basename(path)] = arrays

    def save(self, path, array):
        self.saved[os.path.basename(path)] = array

    def __getattr__(self, name):
        return getattr(np, name)


class _Self:
    snapshot_dir = "nowhere"

    def __init__(self, rot_threshold, trans_threshold):
        self.rot_threshold, self.trans_threshold = rot_threshold, trans_threshold


def reference_pieces():
    src = open(REF_BU, encoding="utf-8").read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "get_angle_deviation"][0]
    angle = textwrap.dedent("\n".join(src.splitlines()[fn.lineno - 1:fn.end_lineno]))
    src = open(REF_TESTER, encoding="utf-8").read()
    cls = [n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "KITTITester"][0]
    test = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "test"][0]
    loop = [i for i, n in enumerate(test.body) if isinstance(n, ast.With)][-1]
    tail = test.body[loop + 1:]
    first = [i for i, n in enumerate(tail) if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "tsfm_est"][0]
    last = [i for i, n in enumerate(tail) if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Subscript)
            and getattr(n.targets[0].value, "id", "") == "errors"][-1]
    lines = src.splitlines()[tail[first].lineno - 1:tail[last].end_lineno]
    return angle, textwrap.dedent("\n".join(lines))


def run_reference(pieces, tsfm_est, rot_gt, trans_gt, rot_threshold=5, trans_threshold=2):
    angle, tail = pieces
    proxy = _NumpyNoFiles()
    ns = {"np": proxy}
    exec(compile(angle, REF_BU + ":get_angle_deviation", "exec"), ns)
    ns.update(tsfm_est=[T for T in tsfm_est], rot_gt=[R for R in rot_gt], trans_gt=[t.reshape(3, 1) for t in trans_gt],
              self=_Self(rot_threshold, trans_threshold))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        exec(compile(tail, REF_TESTER + ":KITTITester.test", "exec"), ns)
    out = {"recall": np.float64(ns["precision"]), "errors": np.array([ns["errors"][k] for k in ERRORS], np.float64),
           "success_dists": np.asarray(proxy.saved["success_dists.npy"]), "fail_dists": np.asarray(proxy.saved["fail_dists.npy"])}
    for k, v in proxy.saved["results"].items():
        out["results_" + k] = np.asarray(v)
    return out


def rot_z(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def rot_x(deg):
    a = np.deg2rad(deg)
    return np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])


def make_case(seed, rot_err_deg, trans_err, exact=False):
    """Ground truth poses like synth.make_pair's (5 .. 20 m along x, a few degrees of yaw) in float32; the estimate of pair i
    is the float32 ground truth, widened, times a rotation by rot_err_deg[i] about z with the translation moved by
    trans_err[i] metres along axis i % 3.  `exact`: identity rotations and whole-metre translations as ground truth, so
    that an offset of 2.0 m is a translation error of exactly 2.0 and a rotation by 5 degrees meets no rounding of the
    ground truth's own."""
    rng = np.random.default_rng(seed)
    n = len(rot_err_deg)
    rot_gt = np.stack([np.eye(3) if exact else rot_z(rng.uniform(-15, 15)) @ rot_x(rng.uniform(-2, 2))
                       for _ in range(n)]).astype(np.float32)
    trans_gt = np.stack([[rng.uniform(5, 20), rng.uniform(-1, 1), rng.uniform(-0.2, 0.2)] for _ in range(n)]).astype(np.float32)
    if exact:
        trans_gt = np.round(trans_gt)
    tsfm = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        tsfm[i, :3, :3] = rot_z(rot_err_deg[i]) @ rot_gt[i].astype(np.float64)
        axis = np.zeros(3)
        axis[i % 3] = 1.0
        tsfm[i, :3, 3] = trans_gt[i].astype(np.float64) + trans_err[i] * axis
    return tsfm, rot_gt, trans_gt


CASES = {
    "mix": dict(seed=1, rot_err_deg=[0.3, 1.2, 7.5, 0.8, 40.0, 2.5, 4.9, 170.0], trans_err=[0.1, 0.5, 0.2, 3.0, 9.0, 1.9, 2.5, 0.05]),
    # pair 0: exactly 2.0 m along x; pair 5: the double below 2.0 along z (t_gt z = 0: the offset survives the addition)
    "threshold": dict(seed=2, rot_err_deg=[0.5, 5.0, 5.0 - 1e-9, 5.0 + 1e-9, 0.2, 0.1],
                      trans_err=[2.0, 0.1, 0.1, 0.1, 0.3, np.nextafter(2.0, 0.0)], exact=True),
    "allfail": dict(seed=3, rot_err_deg=[12.0, 90.0, 6.0], trans_err=[2.5, 4.0, 30.0]),
    "single": dict(seed=4, rot_err_deg=[0.7], trans_err=[0.4]),
}


def main():
    pieces = reference_pieces()
    store = {"names": np.array(list(CASES)), "error_keys": np.array(ERRORS)}
    for name, spec in CASES.items():
        spec = dict(spec)
        tsfm, rot_gt, trans_gt = make_case(spec.pop("seed"), **spec)
        out = run_reference(pieces, tsfm, rot_gt, trans_gt)
        if name == "threshold":      # the case is what it says only if the reference itself sees exactly 2.0 m and fails it
            err = np.linalg.norm(tsfm[:, :3, 3] - trans_gt, axis=-1)
            assert err[0] == 2.0 and err[5] < 2.0
            assert np.linalg.norm(trans_gt[0]) in out["fail_dists"] and np.linalg.norm(trans_gt[5]) in out["success_dists"]
        print(name, "recall", float(out["recall"]), dict(zip(ERRORS, out["errors"])), "success", out["success_dists"],
              "fail", out["fail_dists"])
        store[f"{name}.tsfm_est"], store[f"{name}.rot_gt"], store[f"{name}.trans_gt"] = tsfm, rot_gt, trans_gt
        for k, v in out.items():
            store[f"{name}.{k}"] = v
    path = os.path.join(HERE, "predator_tester_ref.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
