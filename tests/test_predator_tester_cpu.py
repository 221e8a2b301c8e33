"""Host halves of the Predator validation pass and tester epoch, no GPU: `tester.test_summary` against the reference's own
statements (tests/golden/predator_tester_ref.npz, made by tests/golden/make_predator_tester_ref_golden.py from
Predator_APR/lib/tester.py:104-137), `validation.saliency_weight` at its threshold, `validation.reduce_records` against
np.mean."""
import os

import numpy as np
import pytest

from apr_amd import ops
from apr_amd.predator.lib import tester as PT
from apr_amd.predator.lib import validation as PV

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "predator_tester_ref.npz"), allow_pickle=False)
ERRORS = tuple(str(k) for k in G["error_keys"])


def _case(name):
    T = G[f"{name}.tsfm_est"]
    return T[:, :3, :3], T[:, :3, 3], G[f"{name}.rot_gt"], G[f"{name}.trans_gt"]


def test_fixture_holds_the_four_cases():
    assert {"mix", "threshold", "allfail", "single"} <= set(str(n) for n in G["names"])
    assert ERRORS == ("rot_mean", "rot_median", "trans_rmse", "trans_rmedse", "rot_std", "trans_std")


@pytest.mark.parametrize("name", ["mix", "threshold", "allfail", "single"])
def test_summary_equals_the_reference_statements(name):
    rot_est, trans_est, rot_gt, trans_gt = _case(name)
    s = PT.test_summary(rot_est, trans_est, rot_gt, trans_gt)
    assert s["recall"] == G[f"{name}.recall"]
    got = np.array([s["errors"][k] for k in ERRORS], np.float64)
    assert np.array_equal(got, G[f"{name}.errors"], equal_nan=True), (got, G[f"{name}.errors"])
    for k in ("success_dists", "fail_dists"):
        assert s[k].dtype == G[f"{name}.{k}"].dtype and np.array_equal(s[k], G[f"{name}.{k}"]), k
    for k in ("rot_est", "rot_gt", "trans_est", "trans_gt"):
        assert np.array_equal(s[k], G[f"{name}.results_{k}"]), k
    # the [B, 3, 1] ground truth of the tester's own list gives the same
    s3 = PT.test_summary(rot_est, trans_est, rot_gt, trans_gt[:, :, None])
    assert s3["recall"] == s["recall"] and np.array_equal(s3["fail_dists"], s["fail_dists"])


def test_the_cases_are_what_they_are_named_for():
    rot_est, trans_est, rot_gt, trans_gt = _case("threshold")
    s = PT.test_summary(rot_est, trans_est, rot_gt, trans_gt)
    assert s["translation_errors"][0] == 2.0 and s["r_deviation"][0] < 5            # exactly 2 m: strict <, a failure
    assert np.linalg.norm(trans_gt[0]) in s["fail_dists"]
    assert s["translation_errors"][5] < 2.0 and np.linalg.norm(trans_gt[5]) in s["success_dists"]
    assert s["r_deviation"][2] < 5 < s["r_deviation"][3]
    s = PT.test_summary(*_case("allfail"))
    assert s["recall"] == 0 and all(np.isnan(s["errors"][k]) for k in ERRORS) and len(s["success_dists"]) == 0
    s = PT.test_summary(*_case("single"))
    assert s["recall"] == 1 and len(s["success_dists"]) == 1 and s["errors"]["rot_std"] == 0
    # the quirk: rotation statistics over flag_1 alone, translation statistics over flag_2 alone
    rot_est, trans_est, rot_gt, trans_gt = _case("mix")
    s = PT.test_summary(rot_est, trans_est, rot_gt, trans_gt)
    f1, f2 = s["r_deviation"] < 5, s["translation_errors"] < 2
    assert (f1 & ~f2).any() and (f2 & ~f1).any()
    assert s["errors"]["rot_mean"] == round(np.mean(s["r_deviation"][f1]), 3)
    assert s["errors"]["trans_rmse"] == round(np.mean(s["translation_errors"][f2]), 3)


def test_records_summary_reads_the_pose_columns():
    rot_est, trans_est, rot_gt, trans_gt = _case("mix")
    rec = np.zeros((len(rot_est), ops.PTEST_RECORD_FLOATS))
    T = np.tile(np.eye(4), (len(rot_est), 1, 1))
    T[:, :3, :3], T[:, :3, 3] = rot_est, trans_est
    rec[:, ops.PTEST_T:ops.PTEST_T + 16] = T.reshape(-1, 16)
    a, b = PT.records_summary(rec, rot_gt, trans_gt), PT.test_summary(rot_est, trans_est, rot_gt, trans_gt)
    assert a["recall"] == b["recall"] and a["errors"] == b["errors"]


def test_record_entry_points_reject_bad_arguments_before_any_launch(lib):
    """NULL pointers, empty clouds, a slot outside the buffer: APR_CHECK_ARG answers on the host, no GPU needed."""
    one = 8          # any non-NULL address: a rejected call dereferences nothing
    ok = [one, 4, one, 4, one, one, one, one, 0.3, 0.1, 5.0, 2.0, one, 2, 0, None]
    for pos, bad, word in ((0, None, b"NULL"), (7, None, b"NULL"), (12, None, b"NULL"), (1, 0, b"ns"), (3, 0, b"nt"),
                           (14, 2, b"slot"), (14, -1, b"slot"), (7, 12, b"aligned")):
        args = list(ok)
        args[pos] = bad
        assert lib.apr_predator_test_pair(*args) == -1 and word in lib.apr_last_error(), (pos, lib.apr_last_error())
    ok = [one] * 8 + [10, 10, one, 2, 0, None]
    for pos, bad, word in ((0, None, b"NULL"), (3, None, b"NULL"), (10, None, b"NULL"), (8, 0, b"n_src"), (12, 2, b"slot")):
        args = list(ok)
        args[pos] = bad
        assert lib.apr_predator_valid_record(*args) == -1 and word in lib.apr_last_error(), (pos, lib.apr_last_error())
    assert ops.PVALID_RECORD_FLOATS == 16 and ops.PTEST_RECORD_FLOATS == 32


def test_saliency_weight_switches_strictly_above_0_3():
    assert PV.saliency_weight(0.3) == 0.0
    assert PV.saliency_weight(np.nextafter(0.3, 1.0)) == 1.0
    assert PV.saliency_weight(0.0) == 0.0 and PV.saliency_weight(1.0) == 1.0
    assert PV.saliency_weight(float("nan")) == 0.0


def test_reduce_records_is_the_float64_mean_of_the_float32_columns():
    rng = np.random.default_rng(0)
    rec = rng.uniform(0, 3, (5, ops.PVALID_RECORD_FLOATS)).astype(np.float32)
    out = PV.reduce_records(rec)
    assert out["pairs"] == 5 and set(out) == set(PV.KEYS) | {"pairs"} and len(PV.KEYS) == 10
    for i, k in enumerate(PV.KEYS):
        assert out[k] == float(np.mean(rec[:, i].astype(np.float64))), k
    assert PV.KEYS[:8] == ("circle_loss", "recall", "overlap_loss", "overlap_recall", "overlap_precision", "saliency_loss",
                           "saliency_recall", "saliency_precision") and PV.KEYS[8:] == ("chamfer_loss", "regularization_loss")
    rec[2, ops.PVALID_CHAMFER] = np.nan                     # NaN stays NaN, in its own column only
    out = PV.reduce_records(rec)
    assert np.isnan(out["chamfer_loss"]) and not np.isnan(out["regularization_loss"])
    with pytest.raises(ValueError):
        PV.reduce_records(np.zeros((0, ops.PVALID_RECORD_FLOATS), np.float32))
