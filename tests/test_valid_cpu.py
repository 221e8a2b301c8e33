"""Host-side halves of the validation pass (no GPU): the epoch reduction of a hand-made record buffer, the seeds of the
train-then-validate run, and the no-synchronisation rule of the library entry."""
import os
import re

import numpy as np
import pytest

from apr_amd import ops
from apr_amd.fcgf.lib.learned import pair_seeds
from apr_amd.fcgf.lib.validation import GenerativePairValidStep, reduce_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _records():
    r = np.zeros((4, ops.VALID_RECORD_FLOATS), np.float32)
    #        corr_dist  rte   rre      hit_ratio          n_corr
    r[0, :5] = [0.50, 1.00, 0.10, np.float32(0.05), 5000]        # exactly at the feature-match threshold: not matched
    r[1, :5] = [0.25, 3.00, np.nan, np.float32(0.0502), 5000]    # NaN angle: skipped by the rre mean only
    r[2, :5] = [1.00, 0.50, 0.30, 0.0, 5000]
    r[3, :5] = [0.75, 0.10, 0.20, 0.40, 5000]
    r[:, ops.VALID_CHAMFER] = [2.0, 4.0, 6.0, 8.0]
    r[:, ops.VALID_REG] = [1.0, 2.0, 3.0, 4.0]
    return r


def test_epoch_reduction_of_a_hand_made_record_buffer():
    out = reduce_records(_records(), 0.5)
    assert set(out) == {"loss", "rre", "rte", "feat_match_ratio", "hit_ratio", "chamfer_distance", "regularize_loss"}
    # two updates per pair: corr_dist, then chamfer + regulariser * strength
    second = [2.0 + 0.5, 4.0 + 1.0, 6.0 + 1.5, 8.0 + 2.0]
    assert out["loss"] == pytest.approx((0.5 + 0.25 + 1.0 + 0.75 + sum(second)) / 8, rel=1e-7)
    assert out["rre"] == pytest.approx((0.1 + 0.3 + 0.2) / 3, rel=1e-6)              # three pairs, not four
    assert out["rte"] == pytest.approx(4.6 / 4, rel=1e-6)
    assert out["feat_match_ratio"] == 0.5                                           # 0.0502 and 0.40; 0.05 itself is not above 0.05
    assert out["hit_ratio"] == pytest.approx((0.05 + 0.0502 + 0.4) / 4, rel=1e-6)
    assert out["chamfer_distance"] == 5.0 and out["regularize_loss"] == 2.5


def test_epoch_reduction_edge_cases():
    r = _records()
    r[:, ops.VALID_RRE] = np.nan
    assert reduce_records(r, 0.5)["rre"] == 0.0                                     # an AverageMeter nobody updated
    r[2, ops.VALID_N_CORR] = -3                                                     # the kernel met 3 indices out of range
    with pytest.raises(ValueError):
        reduce_records(r, 0.5)
    with pytest.raises(ValueError):
        reduce_records(np.zeros((0, ops.VALID_RECORD_FLOATS), np.float32), 0.5)


def test_train_and_held_out_seeds_are_disjoint():
    seen = set()
    for seed in (0, 1, 2):
        tr, va = pair_seeds(32, 32, seed)
        assert len(tr) == 32 and len(va) == 32 and not set(tr) & set(va)
        assert not seen & (set(tr) | set(va))                                       # nor shared between runs of different seeds
        seen |= set(tr) | set(va)
    with pytest.raises(ValueError):
        pair_seeds(0, 4)


def test_subsample_draws_follow_find_corr():
    step = GenerativePairValidStep(None, None, subsample_size=50)
    np.random.seed(4)
    a0, a1 = step.draw_subsample(300, 40)
    np.random.seed(4)
    b0 = np.random.choice(300, 50, replace=False)
    b1 = np.random.choice(40, 40, replace=False)                                    # a target smaller than the subsample: a permutation
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1)
    assert step.draw_subsample(50, 400) == (None, None)                             # len(F0) > subsample_size decides alone
    with pytest.raises(NotImplementedError):
        GenerativePairValidStep(None, None, symmetric=True)


def test_valid_entry_does_not_synchronise_and_shares_the_irls_code():
    src = lambda name: open(os.path.join(ROOT, "apr_amd", "csrc", name)).read()
    valid = re.sub(r"//.*", "", src("valid.hip"))
    assert not re.search(r"hip(Stream|Device)Synchronize|hipMemcpy", valid)
    assert "irls_run(" in valid and '#include "irls.h"' in src("valid.hip")
    ransac = src("ransac.hip")
    assert '#include "irls.h"' in ransac and "irls_run(" in ransac and "void solve6" not in ransac


def test_valid_entry_rejects_bad_arguments_without_a_gpu(lib):
    assert lib.apr_valid_pair_scratch_bytes(0) == 0 and lib.apr_valid_pair_scratch_bytes(5000) >= 5000 * 40
    one = 1      # non-NULL stand-ins: rejected before any launch
    rc = lib.apr_valid_pair(one, 10, one, 10, None, None, 8, 10, one, one, 0.1, one, 4, 0, one, 1 << 20, None)
    assert rc == -1 and b"sel0 == NULL" in lib.apr_last_error()
    rc = lib.apr_valid_pair(one, 10, one, 10, None, None, 10, 10, one, one, 0.1, one, 4, 4, one, 1 << 20, None)
    assert rc == -1 and b"slot" in lib.apr_last_error()
    rc = lib.apr_valid_pair(one, 10, one, 10, None, None, 10, 10, one, one, 0.1, one, 4, 0, one, 16, None)
    assert rc == -1 and b"scratch" in lib.apr_last_error()
