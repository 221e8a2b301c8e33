"""`apr_fcgf_test_pair` (csrc/fcgf_test.hip) against the float64 NumPy restatement of tests/fcgf_test_oracle.py on hand-made
inputs, and `dists` against the reference's own `dists_nn` rows (tests/golden/fcgf_tester_ref.npz).

Bars, derived.  Integer columns ([2], [4..7], [24], [26..28], [32..41]) are exact.  [0] RTE and [3] |t_gt| are bit-equal:
the header states the operation order and the restatement repeats it on the same doubles.  [1] RRE: its argument is formed
in the stated order too, but it is not a column, so its bit equality shows through the angle: NaN exactly when the
restatement's argument leaves [-1, 1], exactly 0 / pi where it is exactly 1 / -1, and otherwise the bar
tests/test_predator_test_epoch_gpu.py holds the same column to (`acos` may differ by an ulp or two between libraries and
d acos / dx = 1 / sin: 1e-9 degrees for angles >= 0.01 degrees), here in radians.  The two float32 shares [29], [30] are, as
there, the float32 quotient of the float64 restatement's counts, exactly: the inputs keep every float64 distance 1e-4 away
from the threshold, float32 arithmetic on coordinates below 32 m errs by ~1e-5.  The ten hit counts likewise: no float64
distance lies within 1e-4 of any of the ten thresholds (asserted on the restatement), so the counts must be equal, no
exemptions.  `dists` against the float32 restatement (every operation rounded, the kernel's order): 2 ulp; against the
reference's rows: the bar derived in tests/test_fcgf_tester_cpu.py.

Planted rows: per threshold T_k one row at 0.5 T_k and one at 1.5 T_k.  Where that offset itself comes within the margin of
another threshold (0.5 T_k for even k: T_{k/2}; 1.5 T_k for k = 2, 4, 6: T_{3k/2}) the margin assertion above could not
hold, so such a row sits at 0.45 T_k / 1.55 T_k instead.
"""
import os

import numpy as np
import pytest
import torch

from apr_amd import ops
from apr_amd._lib import AprHipError
from tests import fcgf_test_oracle as FO

pytestmark = pytest.mark.gpu

DIST_THR, MARGIN, EPS = 0.3, 1e-4, 2.0 ** -24
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 5000]
RAD = np.pi / 180
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcgf_tester_ref.npz")


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


def planted_offsets():
    out = []
    for k, t in enumerate(FO.HIT_LEVELS, 1):
        for f, g in ((0.5, 0.45), (1.5, 1.55)):
            d = np.sqrt((f * t) ** 2 + 1e-6)
            out.append(f * t if min(abs(d - u) for u in FO.HIT_LEVELS) > 10 * MARGIN else g * t)
    return out


def make_inputs(seed, m0, k0, with_sel, G32, T_est):
    """Clouds in a 20 m cube.  find_corr's side: injective `nn`, the matched target at the ground-truth image of its source
    plus an offset from a list of magnitudes (the planted rows first, as far as m0 goes).  RANSAC's side: its own clouds
    r0 / r1 and an injective `corr`, built the same way.  Rows whose float64 distance comes within 10 * MARGIN of a
    threshold are moved 3 m off."""
    rng = np.random.default_rng(seed)
    G = G32.astype(np.float64)
    m1 = m0 + 3
    n0, n1 = (m0 + 7, m1 + 5) if with_sel else (m0, m1)
    xyz0 = rng.uniform(-10, 10, (n0, 3)).astype(np.float32)
    xyz1 = rng.uniform(-10, 10, (n1, 3)).astype(np.float32)
    sel0 = rng.permutation(n0)[:m0].astype(np.int64) if with_sel else None
    sel1 = rng.permutation(n1)[:m1].astype(np.int64) if with_sel else None
    nn = rng.permutation(m1)[:m0].astype(np.int64)
    a, b, _ = FO.find_corr_rows(n0, n1, sel0, sel1, nn)
    unit = lambda n: (lambda u: u / np.linalg.norm(u, axis=1, keepdims=True))(rng.standard_normal((n, 3)))
    u = unit(m0)
    mag = rng.choice([0.02, 0.06, 0.13, 0.27, 0.44, 0.55, 0.85, 1.3, 3.0], m0)
    plant = planted_offsets()[:m0]
    mag[:len(plant)] = plant
    img = xyz0[a].astype(np.float64) @ G[:3, :3].T + G[:3, 3]
    xyz1[b] = (img + u * mag[:, None]).astype(np.float32)
    for _ in range(4):
        d = np.sqrt(np.linalg.norm(xyz0[a].astype(np.float64) @ G[:3, :3].T + G[:3, 3] - xyz1[b], axis=1) ** 2 + 1e-6)
        close = (np.abs(d[:, None] - np.array(FO.HIT_LEVELS)) < 10 * MARGIN).any(1)
        if not close.any():
            break
        xyz1[b[close]] = (img[close] + 3.0 * u[close]).astype(np.float32)
    k1 = k0 + 3
    r0 = rng.uniform(-10, 10, (k0, 3)).astype(np.float32)
    r1 = rng.uniform(-10, 10, (k1, 3)).astype(np.float32)
    corr = rng.permutation(k1)[:k0].astype(np.int64)
    v = unit(k0)
    img = r0.astype(np.float64) @ G[:3, :3].T + G[:3, 3]
    r1[corr] = (img + v * rng.choice([0.02, 0.06, 0.2, 0.5, 3.0], k0)[:, None]).astype(np.float32)
    for _ in range(4):
        close = np.zeros(k0, bool)
        for T in (G, T_est.astype(np.float32).astype(np.float64)):
            d = np.linalg.norm(r0.astype(np.float64) @ T[:3, :3].T + T[:3, 3] - r1[corr], axis=1)
            close |= np.abs(d - DIST_THR) < 10 * MARGIN
        if not close.any():
            break
        r1[corr[close]] = (img[close] + 3.0 * v[close]).astype(np.float32)
    return dict(xyz0=xyz0, xyz1=xyz1, sel0=sel0, sel1=sel1, nn=nn, r0=r0, r1=r1, corr=corr)


def run_kernel(dev, inp, G32, raw, max_iter=4000000, slots=3, slot=1, want_dists=True, **kw):
    rec = torch.zeros((slots, ops.FTEST_RECORD_FLOATS), dtype=torch.float64, device=dev)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    m0 = len(inp["nn"])
    dists = torch.full((m0,), -1.0, dtype=torch.float32, device=dev) if want_dists else None
    ops.fcgf_test_pair(up(inp["xyz0"]), up(inp["xyz1"]), up(inp["nn"]), up(inp["r0"]), up(inp["r1"]), up(inp["corr"]), up(G32),
                       up(raw), rec, slot, sel0=up(inp["sel0"]), sel1=up(inp["sel1"]), distance_threshold=DIST_THR,
                       max_iter=max_iter, dists=dists, **kw)
    r = rec.cpu().numpy()
    assert not r[[k for k in range(slots) if k != slot]].any()            # the other slots are untouched
    return r[slot], (dists.cpu().numpy() if want_dists else None)


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_record(r, dists, inp, G32, T_est, raw, total_valid=777, max_iter=4000000):
    w = FO.restate(inp["xyz0"], inp["xyz1"], inp["sel0"], inp["sel1"], inp["nn"], inp["r0"], inp["r1"], inp["corr"], G32, T_est,
                   total_valid, max_iter)
    k0 = len(inp["r0"])
    # the margins the exact bars rest on, on the restatement
    assert (np.abs(w["d_nn"][:, None] - np.array(FO.HIT_LEVELS)) > MARGIN).all()
    assert (np.abs(w["d_est"] - DIST_THR) > MARGIN).all() and (np.abs(w["d_gt"] - DIST_THR) > MARGIN).all()
    print(f"m0 {w['m0']} k0 {k0}: rte {r[0]!r} ({w['rte']!r}) rre {r[1]!r} ({w['rre']!r}) hits {r[32:42].astype(int).tolist()}")
    assert np.float64(r[ops.FTEST_RTE]).tobytes() == np.float64(w["rte"]).tobytes()
    assert np.float64(r[ops.FTEST_DIST]).tobytes() == np.float64(w["dist"]).tobytes()
    if not -1.0 <= w["arg"] <= 1.0:
        assert np.isnan(r[ops.FTEST_RRE]) and np.isnan(w["rre"])
    elif abs(w["arg"]) == 1.0:
        assert r[ops.FTEST_RRE] == w["rre"] and w["rre"] in (0.0, np.pi)
    elif w["rre"] >= 0.01 * RAD:
        assert abs(r[ops.FTEST_RRE] - w["rre"]) < 1e-9 * RAD, (r[ops.FTEST_RRE], w["rre"])
    else:                                            # below 0.01 degrees 1 / sin outgrows the bar: both are that small
        assert 0 <= r[ops.FTEST_RRE] < 0.01 * RAD
    assert r[ops.FTEST_SUCCESS] == w["ok"]
    assert (r[ops.FTEST_M0], r[ops.FTEST_K0], r[ops.FTEST_K1], r[ops.FTEST_BAD]) == (w["m0"], w["k0"], w["k1"], w["bad"])
    assert r[ops.FTEST_T:ops.FTEST_T + 16].tobytes() == w["T"].reshape(16).tobytes()
    T, info = ops.ransac_decode(raw, k0)
    assert r[ops.FTEST_INLIERS] == info["inliers"] and r[ops.FTEST_N_VALID] == info["n_valid"] == total_valid
    assert r[ops.FTEST_BEST_ITERATION] == info["best_iteration"]
    assert np.float64(r[ops.FTEST_RMSE]).tobytes() == np.float64(info["rmse"]).tobytes()
    assert r[ops.FTEST_OVERFLOW] == w["overflow"]
    n_est, n_gt = int((w["d_est"] < DIST_THR).sum()), int((w["d_gt"] < DIST_THR).sum())
    assert r[ops.FTEST_INLIER_EST] == float(np.float32(n_est) / np.float32(k0)), (r[ops.FTEST_INLIER_EST], n_est, k0)
    assert r[ops.FTEST_INLIER_GT] == float(np.float32(n_gt) / np.float32(k0)), (r[ops.FTEST_INLIER_GT], n_gt, k0)
    assert r[ops.FTEST_HITS:ops.FTEST_HITS + 10].tolist() == [float(h) for h in w["hits"]]
    assert r[31] == 0 and not r[42:].any()
    if dists is not None:
        assert ulps(dists, w["d32"]).max() <= 2, ulps(dists, w["d32"]).max()
    return w


GT32 = pose(rot(2, 11.0) @ rot(0, 1.5), [7.5, -0.4, 0.1]).astype(np.float32)
EST = pose(rot(2, 1.3) @ rot(0, -0.4) @ GT32[:3, :3].astype(np.float64), GT32[:3, 3].astype(np.float64) + [0.11, -0.07, 0.02])


@pytest.mark.parametrize("with_sel", [False, True])
@pytest.mark.parametrize("m0,k0", list(zip(SIZES, SIZES[3:] + SIZES[:3])))
def test_record_of_a_generic_pose_at_every_block_edge(dev, m0, k0, with_sel):
    inp = make_inputs(m0 * 2 + with_sel, m0, k0, with_sel, GT32, EST)
    raw = FO.pack_raw(EST, inliers=max(1, k0 // 2))
    r, dists = run_kernel(dev, inp, GT32, raw)
    w = check_record(r, dists, inp, GT32, EST, raw)
    assert w["ok"] == 1.0
    if m0 >= 63:
        hits = np.array(w["hits"])
        assert (np.diff(hits) > 0).all() and hits[0] > 0 and hits[-1] < m0      # every threshold separates some rows
        assert 0 < r[ops.FTEST_INLIER_EST] < 1 or k0 == 1
    again, dists2 = run_kernel(dev, inp, GT32, raw)
    assert again.tobytes() == r.tobytes() and dists2.tobytes() == dists.tobytes()
    no_dists, _ = run_kernel(dev, inp, GT32, raw, want_dists=False)
    assert no_dists.tobytes() == r.tobytes()


def test_two_runs_give_equal_records_on_the_device(dev):
    inp = make_inputs(77, 1025, 5000, True, GT32, EST)
    raw = FO.pack_raw(EST)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    recs = [torch.zeros((1, ops.FTEST_RECORD_FLOATS), dtype=torch.float64, device=dev) for _ in range(2)]
    for rec in recs:
        ops.fcgf_test_pair(up(inp["xyz0"]), up(inp["xyz1"]), up(inp["nn"]), up(inp["r0"]), up(inp["r1"]), up(inp["corr"]),
                           up(GT32), up(raw), rec, 0, sel0=up(inp["sel0"]), sel1=up(inp["sel1"]), distance_threshold=DIST_THR)
    assert torch.equal(recs[0], recs[1]) and recs[0].any()


def _nan_pose():
    g = np.load(GOLD, allow_pickle=False)
    return g["nan.T_gt"][0]


HALF = np.diag([-1.0, -1.0, 1.0])
POSES = {
    # name: (T_gt float32, T_est float64, success)
    "generic": lambda: (GT32, EST, 1.0),
    # the reference's own float32 statement gives NaN for this pose against itself; the record's double arithmetic need not
    "nan": lambda: (_nan_pose(), _nan_pose().astype(np.float64), None),
    "exactly_2_m": lambda: (pose(np.eye(3), [6.0, 1.0, 0.0]).astype(np.float32), pose(rot(2, 0.5), [8.0, 1.0, 0.0]), 0.0),
    "below_2_m": lambda: (pose(np.eye(3), [6.0, 1.0, 0.0]).astype(np.float32),
                          pose(rot(2, 0.5), [6.0, 1.0, float(np.nextafter(np.float32(2), np.float32(0)))]), 1.0),
    "half_turn": lambda: (pose(np.eye(3), [6.0, 1.0, 0.0]).astype(np.float32), pose(HALF, [6.0, 1.0, 0.0]), 0.0),
    "past_one": lambda: (pose(np.eye(3), [6.0, 1.0, 0.0]).astype(np.float32), pose(np.eye(3) * (1.0 + 2.0 ** -20), [6.0, 1.0, 0.0]), 0.0),
}


@pytest.mark.parametrize("name", list(POSES))
def test_record_at_the_edges_of_the_angle_and_the_thresholds(dev, name):
    G32, T_est, ok = POSES[name]()
    inp = make_inputs(5, 65, 70, True, G32, T_est)
    raw = FO.pack_raw(T_est)
    r, dists = run_kernel(dev, inp, G32, raw)
    w = check_record(r, dists, inp, G32, T_est, raw)
    if ok is not None:
        assert w["ok"] == ok
    if name == "nan":
        assert r[ops.FTEST_RTE] == 0.0 and (np.isnan(r[ops.FTEST_RRE]) or r[ops.FTEST_RRE] < 1e-3)
        assert r[ops.FTEST_SUCCESS] == (0.0 if np.isnan(r[ops.FTEST_RRE]) else 1.0)
    if name == "exactly_2_m":
        assert r[ops.FTEST_RTE] == 2.0 and r[ops.FTEST_SUCCESS] == 0.0
    if name == "below_2_m":
        assert r[ops.FTEST_RTE] == float(np.nextafter(np.float32(2), np.float32(0))) and r[ops.FTEST_SUCCESS] == 1.0
    if name == "half_turn":
        assert r[ops.FTEST_RRE] == np.pi
    if name == "past_one":
        assert w["arg"] > 1.0 and np.isnan(r[ops.FTEST_RRE]) and r[ops.FTEST_SUCCESS] == 0.0      # unclipped: a failure


@pytest.mark.parametrize("total_valid,max_iter,flag", [(2 ** 20, 4000000, 0.0), (2 ** 20 + 1, 4000000, 1.0),
                                                       (2 ** 21, 2 ** 20, 0.0), (2 ** 21, 2 ** 20 + 1, 1.0)])
def test_the_overflow_column(dev, total_valid, max_iter, flag):
    """Set only when BOTH total_valid and max_iter exceed 2^20: of total_valid = 2^20 and 2^20 + 1 under 4 M iterations the
    second, of max_iter = 2^20 and 2^20 + 1 under 2^21 valid hypotheses the second."""
    inp = make_inputs(6, 65, 64, False, GT32, EST)
    raw = FO.pack_raw(EST, total_valid=total_valid)
    r, dists = run_kernel(dev, inp, GT32, raw, max_iter=max_iter)
    check_record(r, dists, inp, GT32, EST, raw, total_valid=total_valid, max_iter=max_iter)
    assert r[ops.FTEST_OVERFLOW] == flag


def test_out_of_range_entries_read_row_0_and_are_counted(dev):
    inp = make_inputs(9, 200, 210, True, GT32, GT32.astype(np.float64))
    G = GT32.astype(np.float64)
    inp["sel0"][[3, 50]] = [-1, len(inp["xyz0"])]
    inp["nn"][[7, 60]] = [len(inp["sel1"]), -5]
    inp["sel1"][inp["nn"][100]] = 2 ** 40
    inp["corr"][[3, 77, 199]] = [-1, len(inp["r1"]), 2 ** 40]
    # row 0 of each target cloud: far from every threshold whatever reads it
    inp["xyz1"][0] = [40.0, 40.0, 40.0]
    inp["r1"][0] = (inp["r0"][3].astype(np.float64) @ G[:3, :3].T + G[:3, 3]).astype(np.float32)      # row 3 now reads an inlier
    a, b, bad = FO.find_corr_rows(len(inp["xyz0"]), len(inp["xyz1"]), inp["sel0"], inp["sel1"], inp["nn"])
    assert bad == 5 and a[3] == 0 and a[50] == 0 and b[100] == 0
    # rows that now read source row 0 must keep the margin too: move their targets far off
    inp["xyz1"][b[[3, 50]]] = [-40.0, -40.0, -40.0]
    raw = FO.pack_raw(GT32.astype(np.float64))
    r, dists = run_kernel(dev, inp, GT32, raw)
    w = check_record(r, dists, inp, GT32, GT32.astype(np.float64), raw)
    assert w["bad"] == 8 and r[ops.FTEST_BAD] == 8 and w["d_gt"][3] < 1e-5


def test_dists_meet_the_references_rows(dev):
    g = np.load(GOLD, allow_pickle=False)
    for name in g["draw_names"]:
        f = lambda k: g[f"draw.{name}.{k}"]
        sel = len(f("inds0")) > 0
        inp = dict(xyz0=f("xyz0"), xyz1=f("xyz1"), sel0=f("inds0") if sel else None, sel1=f("inds1") if sel else None, nn=f("nn"),
                   r0=f("xyz0"), r1=f("xyz1"), corr=np.zeros(len(f("xyz0")), np.int64))
        r, dists = run_kernel(dev, inp, f("T_gt"), FO.pack_raw(f("T_gt").astype(np.float64)))
        want = f("dists_nn")
        bound = 16 * EPS * (np.abs(f("xyz0")).max() * 3 + np.abs(f("T_gt")[:3, 3]).max())
        print(name, "max |dists - reference|", np.abs(dists - want).max(), "bound", bound)
        assert dists.shape == want.shape and np.abs(dists.astype(np.float64) - want).max() <= bound
        assert r[ops.FTEST_HITS:ops.FTEST_HITS + 10].tolist() == [float((dists.astype(np.float64) < t).sum()) for t in FO.HIT_LEVELS]
        assert r[ops.FTEST_M0] == len(want) and r[ops.FTEST_BAD] == 0


def test_argument_checks_raise_before_a_launch(dev):
    lib = ops._lib_()
    rec = torch.zeros((2, ops.FTEST_RECORD_FLOATS), dtype=torch.float64, device=dev)
    x = torch.zeros((4, 3), device=dev)
    idx = torch.zeros(4, dtype=torch.int64, device=dev)
    T = torch.eye(4, device=dev)
    raw = torch.from_numpy(FO.pack_raw(np.eye(4))).to(dev)
    odd = torch.zeros(200, dtype=torch.uint8, device=dev)[4:]
    p = ops.ptr
    dflt = dict(xyz0=p(x), n0=4, sel0=None, sel1=None, m0=4, m1=4, nn=p(idx), r0=p(x), k0=4, corr=p(idx), T=p(T), raw=p(raw),
                thr=0.3, it=1000, rec=p(rec), slot=0)

    def call(**o):
        a = dict(dflt, **o)
        return lib.apr_fcgf_test_pair(a["xyz0"], a["n0"], p(x), 4, a["sel0"], a["sel1"], a["m0"], a["m1"], a["nn"], a["r0"], a["k0"],
                                      p(x), 4, a["corr"], a["T"], a["raw"], a["thr"], 2.0, 5.0, a["it"], None, a["rec"], 2, a["slot"],
                                      None)

    ops.check(call())
    torch.cuda.synchronize()
    assert rec[0].any() and not rec[1].any()
    rec.zero_()
    for bad in (dict(xyz0=None), dict(nn=None), dict(r0=None), dict(corr=None), dict(T=None), dict(raw=None), dict(rec=None),
                dict(m0=0), dict(k0=0), dict(m0=2 ** 24, sel0=p(idx)), dict(k0=2 ** 24), dict(m0=3), dict(m1=3), dict(n0=0),
                dict(slot=2), dict(slot=-1), dict(raw=p(odd)), dict(thr=0.0), dict(it=0)):
        with pytest.raises(AprHipError):
            ops.check(call(**bad))
    with pytest.raises(AprHipError):
        ops.fcgf_test_pair(x, x, idx, x, x, idx, T, raw, rec, 2)
    with pytest.raises(AprHipError):
        ops.fcgf_test_pair(x, x, idx[:3], x, x, idx, T, raw, rec, 0)
    with pytest.raises(AprHipError):
        ops.fcgf_test_pair(x, x, idx, x, x, idx[:3], T, raw, rec, 0)
    with pytest.raises(AprHipError):
        ops.fcgf_test_pair(x, x, idx, x, x, idx, T, raw[:100], rec, 0)
    with pytest.raises(AprHipError):
        ops.fcgf_test_pair(x, x, idx, x, x, idx, T, raw, rec, 0, dists=torch.zeros(3, device=dev))
    with pytest.raises(AprHipError):
        ops.fcgf_test_pair(x.cpu(), x, idx, x, x, idx, T, raw, rec, 0)
    sb = int(lib.apr_ransac_scratch_bytes(4, 1000))
    scratch = torch.zeros(sb, dtype=torch.uint8, device=dev)
    out = torch.zeros(136, dtype=torch.uint8, device=dev)
    rargs = lambda **o: [o.get("x", p(x)), o.get("n0", 4), p(x), 4, o.get("corr", p(idx)), o.get("d", 0.3), 0.9, o.get("it", 1000), 0,
                         o.get("scratch", p(scratch)), o.get("sb", sb), o.get("raw", p(out)), None]
    for bad in (dict(x=None), dict(corr=None), dict(raw=None), dict(scratch=None), dict(n0=0), dict(it=0), dict(it=2 ** 31),
                dict(d=0.0), dict(sb=sb - 1)):
        with pytest.raises(AprHipError):
            ops.check(lib.apr_ransac_pose_async(*rargs(**bad)))
    with pytest.raises(AprHipError):
        ops.ransac_pose_async(x, x, idx[:3], 0.3)
    torch.cuda.synchronize()
    assert not rec.any() and not out.any()
