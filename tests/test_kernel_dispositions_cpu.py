"""Kernel-point dispositions for any (num_kernel_points, fixed): apr_amd/predator/kernels/kernel_points.py against the
reference's own results (tests/golden/kernel_dispositions.npz, written by tests/golden/make_kernel_dispositions_golden.py).

The restated descent reproduces the reference's raw dispositions to 1e-11 (the reference's own sensitivity to a one-ulp change
of every initial draw is <= 1.4e-14 over these four cases: a margin of about 1000).  Measured on the build machine: the
largest |restatement - reference| over the four cases is exactly 0.0, and load_kernels gives the golden's bits.
"""
import os

import numpy as np
import pytest

from apr_amd.predator.kernels import kernel_points as KP

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "kernel_dispositions.npz"))
CASES = [(4, "verticals"), (7, "center"), (13, "none"), (16, "center")]
IDS = [f"{k}-{f}" for k, f in CASES]


@pytest.fixture(autouse=True)
def fresh(monkeypatch):
    """every test starts with an empty memo and no disposition directory, and leaves the global RNG as it found it"""
    monkeypatch.setattr(KP, "_MEMO", {})
    monkeypatch.delenv(KP.DISPOSITION_DIR_ENV, raising=False)
    state = np.random.get_state()
    yield
    np.random.set_state(state)


@pytest.fixture(scope="module")
def made():
    """(K, fixed) -> (load_kernels(1.5, ..) under seed 3 from an empty memo, the raw disposition it made, the RNG state after):
    one descent per case, shared"""
    out = {}
    state = np.random.get_state()
    saved = KP._MEMO
    try:
        for K, fixed in CASES:
            KP._MEMO = {}
            np.random.seed(3)
            lk = KP.load_kernels(1.5, K, 3, fixed)
            out[(K, fixed)] = (lk, KP._MEMO[(K, fixed)].copy(), np.random.get_state())
    finally:
        KP._MEMO = saved
        np.random.set_state(state)
    return out


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _ulp_diff(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return float((np.abs(a.astype(np.float64) - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))).max())


@pytest.mark.parametrize("K,fixed", CASES, ids=IDS)
def test_restated_descent_reproduces_the_reference(made, K, fixed):
    lk, raw, _ = made[(K, fixed)]
    ref = GOLD[f"raw/{K}_{fixed}"]
    assert raw.dtype == np.float64 and raw.shape == ref.shape == (K, 3)
    err = float(np.abs(raw - ref).max())
    print(f"({K}, {fixed}): max |restatement - reference| = {err:.3g}")
    assert err <= 1e-11
    assert lk.dtype == np.float32 and lk.shape == (K, 3)
    u = _ulp_diff(lk, GOLD[f"lk/{K}_{fixed}"])
    print(f"({K}, {fixed}): load_kernels vs the reference, float32 ulps: {u:.3g}")
    assert u <= 1.0


@pytest.mark.parametrize("K,fixed", CASES, ids=IDS)
def test_invariants(made, K, fixed):
    _, raw, _ = made[(K, fixed)]
    if fixed in ("center", "verticals"):
        assert not raw[0].any(), "the centre point is not exactly 0"
    if fixed == "verticals":
        # points 1 and 2 START at +-2/3 on the z axis; the descent zeroes their x / y gradient only, so they stay exactly on
        # the axis and slide along it, as in the reference (its candidate 0 ends at +0.65325 / -0.65325 after scaling)
        assert not raw[1, :2].any() and not raw[2, :2].any(), "points 1 and 2 left the z axis"
        assert raw[1, 2] > 0 > raw[2, 2]


@pytest.mark.parametrize("K,fixed", [(4, "verticals"), (7, "center"), (5, "none")], ids=str)
def test_mean_norm_is_the_ratio(K, fixed):
    """The reference rescales ALL candidates by one factor, ratio / mean |x| over every candidate's points 1..: that mean is
    0.66 to 1e-9 (a single candidate's need not be)."""
    np.random.seed(3)
    pts, _ = KP.kernel_point_optimization(1.0, K, num_kernels=100, fixed=fixed)
    assert abs(np.linalg.norm(pts[:, 1:], axis=-1).mean() - 0.66) <= 1e-9


def test_verticals_stay_on_the_axis_and_rows_after_the_stop_are_zero():
    np.random.seed(5)
    pts, norms = KP.kernel_point_optimization(1.0, 4, num_kernels=3, fixed="verticals")
    assert pts.shape == (3, 4, 3) and norms.shape == (10000, 3)
    assert not pts[:, 0].any() and not pts[:, 1:3, :2].any()
    assert (pts[:, 1, 2] > 0).all() and (pts[:, 2, 2] < 0).all()
    stop = int((norms.max(1) > 0).sum())
    assert 0 < stop < 10000 and not norms[stop:].any(), "rows after the stop are not zero"


def test_generator_shapes_and_global_stop():
    np.random.seed(1)
    pts, norms = KP.kernel_point_optimization(2.0, 5, num_kernels=4, fixed="none", ratio=0.5)
    assert pts.shape == (4, 5, 3) and norms.shape == (10000, 4)
    r = np.linalg.norm(pts, axis=-1)
    assert abs(r[:, 1:].mean() - 2.0 * 0.5) <= 1e-9          # one scale for all kernels: the mean over every kernel's points 1..
    live = (norms > 0).sum(0)
    assert (live == live[0]).all(), "the kernels did not stop together"


def _parent_load_kernels(radius):
    """load_kernels of the parent commit for (15, 'center'), restated"""
    pts = np.load(KP._TABLE)
    theta = np.random.rand() * 2 * np.pi
    c, s = np.cos(theta), np.sin(theta)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float32)
    pts = pts + np.random.normal(scale=0.01, size=pts.shape)
    return np.matmul(radius * pts, R).astype(np.float32)


def test_15_center_keeps_its_bits_and_its_draws():
    np.random.seed(11)
    want = _parent_load_kernels(1.25)
    after = np.random.get_state()
    np.random.seed(11)
    got = KP.load_kernels(1.25, 15, 3, "center")
    assert got.tobytes() == want.tobytes()
    assert _same_state(np.random.get_state(), after), "(15, 'center') consumed other draws than the parent"
    assert (15, "center") not in KP._MEMO


def test_memo_and_draw_accounting(made):
    K, fixed = 7, "center"
    lk, raw, after_first = made[(K, fixed)]
    KP._MEMO[(K, fixed)] = raw.copy()
    # a later call: no descent, the rotation and the noise alone (1 + 21 draws), from whatever state the RNG is in
    np.random.seed(3)
    theta = np.random.rand() * 2 * np.pi
    noise = np.random.normal(scale=0.01, size=(K, 3))
    after = np.random.get_state()
    c, s = np.cos(theta), np.sin(theta)
    want = np.matmul(1.5 * (raw + noise), np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float32)).astype(np.float32)
    np.random.seed(3)
    got = KP.load_kernels(1.5, K, 3, fixed)
    assert got.tobytes() == want.tobytes() and _same_state(np.random.get_state(), after)
    assert got.tobytes() != lk.tobytes(), "the first call's draws include the generator's"
    assert not _same_state(after, after_first)
    assert np.array_equal(KP._MEMO[(K, fixed)], raw), "load_kernels changed the memo"


def test_disposition_directory(tmp_path, monkeypatch, made):
    K, fixed = 4, "verticals"
    lk, raw, after_first = made[(K, fixed)]
    folder = tmp_path / "disp"
    monkeypatch.setenv(KP.DISPOSITION_DIR_ENV, str(folder))
    cwd = tmp_path / "cwd"
    cwd.mkdir()
    monkeypatch.chdir(cwd)
    pkg_before = sorted(os.listdir(os.path.dirname(KP._TABLE)))
    np.random.seed(3)
    first = KP.load_kernels(1.5, K, 3, fixed)
    assert first.tobytes() == lk.tobytes() and _same_state(np.random.get_state(), after_first)
    path = folder / f"k_{K:03d}_{fixed}_3D.npy"
    assert [p.name for p in folder.iterdir()] == [path.name]
    assert np.array_equal(np.load(path), raw)
    assert not list(cwd.iterdir()) and sorted(os.listdir(os.path.dirname(KP._TABLE))) == pkg_before
    # a later process: an empty memo, the file at hand -> no descent
    KP._MEMO.clear()
    np.random.seed(3)
    second = KP.load_kernels(1.5, K, 3, fixed)
    after_second = np.random.get_state()
    np.random.seed(3)
    np.random.rand()
    np.random.normal(scale=0.01, size=(K, 3))
    assert _same_state(after_second, np.random.get_state()), "reading the file consumed other draws than rotation and noise"
    assert second.tobytes() != first.tobytes() and np.array_equal(KP._MEMO[(K, fixed)], raw)
    # (15, 'center') writes nothing
    KP.load_kernels(1.0, 15, 3, "center")
    assert [p.name for p in folder.iterdir()] == [path.name]


def test_refusals():
    state = np.random.get_state()
    for kw, exc in ((dict(dimension=2), NotImplementedError), (dict(num_kpoints=31), NotImplementedError),
                    (dict(lloyd=True), NotImplementedError), (dict(num_kpoints=1), ValueError),
                    (dict(num_kpoints=0), ValueError), (dict(num_kpoints=3, fixed="verticals"), ValueError),
                    (dict(num_kpoints=2, fixed="verticals"), ValueError), (dict(fixed="vertical"), ValueError),
                    (dict(fixed="centre"), ValueError), (dict(num_kpoints=15, fixed="center", lloyd=True), NotImplementedError),
                    (dict(num_kpoints=15, fixed="center", dimension=2), NotImplementedError)):
        args = dict(radius=1.0, num_kpoints=7, dimension=3, fixed="center")
        args.update(kw)
        with pytest.raises(exc):
            KP.load_kernels(**args)
    assert _same_state(np.random.get_state(), state), "a refused call drew from the RNG"
    assert not KP._MEMO


def test_small_counts_build():
    """the smallest counts the generator takes: 2 ('none', 'center') and 4 ('verticals')"""
    np.random.seed(2)
    for K, fixed in ((2, "none"), (2, "center"), (4, "verticals")):
        pts = KP.load_kernels(1.0, K, 3, fixed)
        assert pts.shape == (K, 3) and np.isfinite(pts).all()


def test_set_disposition_feeds_load_kernels_without_a_descent():
    pts = np.random.default_rng(0).uniform(-0.6, 0.6, (9, 3))
    KP.set_disposition(9, "none", pts)
    np.random.seed(4)
    got = KP.load_kernels(2.0, 9, 3, "none")
    np.random.seed(4)
    theta = np.random.rand() * 2 * np.pi
    noise = np.random.normal(scale=0.01, size=(9, 3))
    c, s = np.cos(theta), np.sin(theta)
    want = np.matmul(2.0 * (pts + noise), np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float32)).astype(np.float32)
    assert got.tobytes() == want.tobytes()
    for bad in ((15, "center", np.zeros((15, 3))), (9, "centre", pts), (8, "none", pts), (9, "none", pts * np.nan)):
        with pytest.raises(ValueError):
            KP.set_disposition(*bad)
