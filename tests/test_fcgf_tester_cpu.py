"""The host half of FCGF_APR's tester epoch (apr_amd/fcgf/lib/tester.py) against tests/golden/fcgf_tester_ref.npz, which
holds what the reference's own text gives (make_fcgf_tester_ref_golden.py): `test_summary` value for value, the NumPy draws
index for index with the stream left at the reference's sentinel, `fmr_table` on hand-made counts, and the float32
restatement of `evaluate_nn_dist` (tests/fcgf_test_oracle.py) against the reference's `dists_nn` rows.

Bar of the last: the reference moves a point with torch's matmul, whose summation order is not stated; three products of
magnitude <= xmax each rounded, two additions and the translation: 6 roundings of 2^-24 relative to at most
3 xmax + |t|, and d sqrt(s + 1e-6) / d dx <= 1 per component, so 16 * 2^-24 * (3 xmax + |t|) absolute covers it.
"""
import os

import numpy as np
import pytest

from apr_amd import ops
from apr_amd.fcgf.lib import tester as FT
from tests import fcgf_test_oracle as FO

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcgf_tester_ref.npz")
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD, allow_pickle=False)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", ["mix", "threshold", "nan", "allfail", "single"])
def test_summary_equals_the_reference_value_for_value(gold, name):
    assert name in list(gold["summary_names"])
    T_est, T_gt = gold[f"{name}.T_est"], gold[f"{name}.T_gt"]
    assert T_est.dtype == np.float32 and T_gt.dtype == np.float32
    out = FT.test_summary(T_est, T_gt)
    for key in ("list_rte", "list_rre", "dists_success", "dists_fail", "dists"):
        assert out[key].dtype == np.float32 and _same(out[key], gold[f"{name}.{key}"]), (key, out[key], gold[f"{name}.{key}"])
    assert _same(out["rtes"], out["list_rte"]) and _same(out["rres"], out["list_rre"])
    assert out["T_est"].tobytes() == T_est.tobytes() and out["T_gt"].tobytes() == T_gt.tobytes()
    s, t, r = gold[f"{name}.success"], gold[f"{name}.rte"], gold[f"{name}.rre"]      # sum, count, avg, var
    assert (out["success_sum"], out["success_count"], out["recall"]) == (s[0], s[1], s[2])
    assert _same(np.float64(out["rte_avg"]), t[2]) and _same(np.float64(out["rte_var"]), t[3])
    assert _same(np.float64(out["rre_avg"]), r[2]) and _same(np.float64(out["rre_var"]), r[3])
    if name == "nan":
        assert T_est.tobytes() == T_gt.tobytes() and np.isnan(out["list_rre"]).sum() == 3 and out["recall"] == 0.25
    if name == "threshold":
        assert out["list_rte"][0] == 2.0 and out["list_rte"][2] < 2.0 and out["success_sum"] == 3
    if name == "allfail":
        assert out["rte_avg"] == 0 and np.isnan(out["rte_var"]) and out["recall"] == 0


def test_summary_refuses_nothing_and_mismatched_inputs():
    with pytest.raises(ValueError):
        FT.test_summary(np.zeros((0, 4, 4), np.float32), np.zeros((0, 4, 4), np.float32))
    with pytest.raises(ValueError):
        FT.test_summary(np.zeros((2, 4, 4), np.float32), np.zeros((3, 4, 4), np.float32))


def test_fmr_table_on_hand_made_counts():
    rec = np.zeros((3, ops.FTEST_RECORD_FLOATS))
    rec[:, ops.FTEST_M0] = [100, 40, 5000]                               # m0 differs between the pairs
    rec[0, ops.FTEST_HITS:ops.FTEST_HITS + 10] = [0, 1, 2, 3, 5, 8, 10, 11, 50, 100]
    rec[1, ops.FTEST_HITS:ops.FTEST_HITS + 10] = [0, 0, 1, 2, 2, 4, 4, 4, 4, 40]
    rec[2, ops.FTEST_HITS:ops.FTEST_HITS + 10] = [50, 51, 100, 150, 250, 251, 500, 501, 4999, 5000]
    out = FT.fmr_table(rec)
    hr, fmrs = out["hit_ratios"], out["fmrs"]
    assert hr.shape == (10, 3) and fmrs.shape == (10, 10)
    assert list(hr[:, 0]) == [c / 100 for c in (0, 1, 2, 3, 5, 8, 10, 11, 50, 100)]
    assert list(hr[:, 1]) == [c / 40 for c in (0, 0, 1, 2, 2, 4, 4, 4, 4, 40)]
    assert hr[0, 2] == 50 / 5000 and hr[9].tolist() == [1.0, 1.0, 1.0]
    # fmrs[j][k]: share of pairs with hit_ratios[k] > (j + 1) * 0.01, strictly; 50 / 5000 == 0.01 is not above tao_2 = 0.01
    assert fmrs[0].tolist() == [0.0, 1 / 3, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    # tao_2 = 0.05: 5 / 100 and 2 / 40 and 250 / 5000 are 0.05, not above it
    assert fmrs[4].tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    # tao_2 = 0.1 (the double 10 * 0.01): 10 / 100, 4 / 40, 500 / 5000 are 0.1
    assert 10 * 0.01 == 0.1 and fmrs[9].tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2 / 3, 2 / 3, 1.0]
    # the reference's commented-out block on a rectangular dists_nn gives the same two tables
    rng = np.random.default_rng(0)
    dists_nn = rng.uniform(0, 1.2, (4, 50))
    rec = np.zeros((4, ops.FTEST_RECORD_FLOATS))
    rec[:, ops.FTEST_M0] = 50
    rec[:, ops.FTEST_HITS:ops.FTEST_HITS + 10] = np.stack([(dists_nn < k * 0.1).sum(1) for k in range(1, 11)], 1)
    want_hr = np.stack([np.mean((dists_nn < k * 0.1).astype(float), axis=1) for k in range(1, 11)])
    want_fmr = np.stack([np.mean((want_hr > j * 0.01).astype(float), axis=1) for j in range(1, 11)])
    out = FT.fmr_table(rec)
    assert np.array_equal(out["hit_ratios"], want_hr) and np.array_equal(out["fmrs"], want_fmr)
    with pytest.raises(ValueError):
        FT.fmr_table(np.zeros((0, ops.FTEST_RECORD_FLOATS)))


def test_records_summary_reads_the_pose_columns(gold):
    T_est, T_gt = gold["mix.T_est"], gold["mix.T_gt"]
    rec = np.zeros((len(T_est), ops.FTEST_RECORD_FLOATS))
    rec[:, ops.FTEST_T:ops.FTEST_T + 16] = T_est.reshape(-1, 16).astype(np.float64)
    rec[:, ops.FTEST_M0] = 10
    out = FT.records_summary(rec, T_gt)
    want = FT.test_summary(T_est, T_gt)
    assert out["recall"] == want["recall"] and _same(out["list_rre"], want["list_rre"]) and out["hit_ratios"].shape == (10, len(T_est))


@pytest.mark.parametrize("variant", ["apr", "fcgf"])
@pytest.mark.parametrize("name", ["both", "none", "equal", "short1"])
def test_host_draws_are_the_references_and_leave_the_stream_where_it_does(gold, name, variant):
    g = lambda k: gold[f"draw.{name}.{k}"]
    sub, npts = (int(v) for v in gold["draw_sizes"])
    n0, n1 = len(g("xyz0")), len(g("xyz1"))
    for rng in (None, np.random.RandomState(int(g("seed")))):
        np.random.seed(int(g("seed")))
        h = FT.host_draws(n0, n1, variant, sub, npts, rng)
        sentinel = (np.random if rng is None else rng).random()
        for key in ("inds0", "inds1") + (("choice0", "choice1") if variant == "fcgf" else ()):
            want = g(key)
            if len(want) == 0:
                assert h[key] is None, key
            else:
                assert h[key].dtype == np.int64 and np.array_equal(h[key], want), key
        if variant == "apr":
            assert h["choice0"] is None and h["choice1"] is None
        assert sentinel == float(g("sentinel_" + variant))
    drew = dict(both=(True, True, True), none=(False, True, True), equal=(False, False, False), short1=(True, True, True))[name]
    assert (len(g("inds0")) > 0, len(g("choice0")) > 0, len(g("choice1")) > 0) == drew
    with pytest.raises(ValueError):
        FT.host_draws(n0, n1, "other")


@pytest.mark.parametrize("name", ["both", "none", "equal", "short1"])
def test_the_float32_restatement_of_evaluate_nn_dist_meets_the_references_rows(gold, name):
    g = lambda k: gold[f"draw.{name}.{k}"]
    xyz0, xyz1, T = g("xyz0"), g("xyz1"), g("T_gt")
    sel0, sel1 = (g("inds0"), g("inds1")) if len(g("inds0")) else (None, None)
    a, b, bad = FO.find_corr_rows(len(xyz0), len(xyz1), sel0, sel1, g("nn"))
    d32 = FO.dists_f32(xyz0, xyz1, a, b, T)
    want = g("dists_nn")
    assert bad == 0 and d32.dtype == np.float32 and d32.shape == want.shape
    bound = 16 * EPS * (np.abs(xyz0).max() * 3 + np.abs(T[:3, 3]).max())
    print(name, "max |d32 - reference|", np.abs(d32 - want).max(), "bound", bound)
    assert np.abs(d32.astype(np.float64) - want).max() <= bound


def test_ransac_encode_is_the_inverse_of_decode(lib):
    rng = np.random.default_rng(5)
    for inliers, it, tv in ((37, 4242, 777), (1, 0, 1), (4999, 3999999, 2 ** 21), (0, -1, 0)):
        err2 = float(rng.uniform(0, 3)) if inliers else 0.0
        T = np.eye(4)
        T[:3] = rng.standard_normal((3, 4))
        raw = FO.pack_raw(T, it=it, inliers=inliers if it >= 0 else -1, err2=err2, total_valid=tv)
        T_dec, info = ops.ransac_decode(raw, 5000)
        again = ops.ransac_encode(T_dec, info)
        T2, info2 = ops.ransac_decode(again, 5000)
        assert T2.tobytes() == T_dec.tobytes() and info2 == info
