"""CPU side of the ICP pose refinement (csrc/icp.hip): the C ABI's exports and argument checks, and the host restatement
(tests/icp_oracle.py) against a planted motion and against itself in its two arithmetic variants."""
import ctypes as C

import numpy as np
import pytest

from tests import icp_oracle as O


def test_library_exports_the_icp_entry_points(lib):
    from apr_amd import _lib
    assert "apr_icp_batch" in _lib.PROTOTYPES and "apr_icp_scratch_bytes" in _lib.PROTOTYPES
    assert lib.apr_icp_batch is not None and lib.apr_icp_scratch_bytes is not None


def test_scratch_size_grows_with_every_argument(lib):
    base = lib.apr_icp_scratch_bytes(100000, 100000, 1)
    assert base > 0
    assert lib.apr_icp_scratch_bytes(400000, 100000, 1) > base
    assert lib.apr_icp_scratch_bytes(100000, 400000, 1) > base
    assert lib.apr_icp_scratch_bytes(100000, 100000, 64) > base


def _call(lib, src_off, tgt_off, nb, max_dist=0.2, max_iteration=5, top=None):
    """apr_icp_batch with dummy (never dereferenced) device pointers: only the argument checks may run."""
    so = np.asarray(src_off, dtype=np.int64)
    to = np.asarray(tgt_off, dtype=np.int64)
    top = None if top is None else np.asarray(top, dtype=np.int32)
    dummy = C.c_void_p(256)
    return lib.apr_icp_batch(dummy, so.ctypes.data_as(C.c_void_p), dummy, to.ctypes.data_as(C.c_void_p), len(to) - 1,
                             None if top is None else top.ctypes.data_as(C.c_void_p), nb, dummy, max_dist, max_iteration,
                             1e-6, 1e-6, dummy, None, dummy, 1 << 40, None)


@pytest.mark.parametrize("kind", ["no_problem", "empty_source", "zero_max_dist", "negative_max_dist", "negative_iterations"])
def test_bad_arguments_are_rejected_before_any_launch(lib, kind):
    rc = {"no_problem": lambda: _call(lib, [0], [0, 10], 0),
          "empty_source": lambda: _call(lib, [0, 0], [0, 10], 1),
          "zero_max_dist": lambda: _call(lib, [0, 10], [0, 10], 1, max_dist=0.0),
          "negative_max_dist": lambda: _call(lib, [0, 10], [0, 10], 1, max_dist=-0.2),
          "negative_iterations": lambda: _call(lib, [0, 10], [0, 10], 1, max_iteration=-1)}[kind]()
    assert rc == -1                                             # APR_EINVAL
    assert b"apr_icp_batch" in lib.apr_last_error()


@pytest.mark.parametrize("kind", ["65_problems", "65_segments", "segment_past_the_end", "negative_segment", "empty_segment",
                                  "empty_source_in_the_middle", "default_mapping_needs_one_segment_each"])
def test_batch_layout_is_checked_before_any_launch(lib, kind):
    """The limits of the problem and segment tables.  The device pointers are dummies and this machine has no GPU: -1 can
    only come from a check on the host that ran before the first HIP call."""
    ten = lambda k: list(range(0, 10 * k + 1, 10))
    rc = {"65_problems": lambda: _call(lib, ten(65), [0, 10], 65, top=[0] * 65),
          "65_segments": lambda: _call(lib, ten(3), ten(65), 3, top=[0, 64, 1]),
          "segment_past_the_end": lambda: _call(lib, ten(3), ten(2), 3, top=[0, 2, 1]),
          "negative_segment": lambda: _call(lib, ten(3), ten(2), 3, top=[0, -1, 1]),
          "empty_segment": lambda: _call(lib, ten(2), [0, 10, 10, 20], 2, top=[0, 2]),
          "empty_source_in_the_middle": lambda: _call(lib, [0, 10, 10, 20], ten(3), 3),
          "default_mapping_needs_one_segment_each": lambda: _call(lib, ten(3), ten(2), 3)}[kind]()
    assert rc == -1
    assert b"apr_icp_batch" in lib.apr_last_error()


def test_oracle_recovers_a_planted_motion_on_a_noise_free_cloud():
    rng = np.random.default_rng(0)
    tgt = rng.uniform(-10.0, 10.0, size=(3000, 3))              # ~1 m between neighbours: a 5 cm motion keeps every match
    P = O.perturbation(0.05, 1.0, seed=5)
    src = (tgt - P[:3, 3]) @ P[:3, :3]                          # P src = tgt
    r = O.icp(src, tgt, None, 0.5, 50, fp32_round=False)
    assert r["fitness"] == 1.0 and r["n_corr"] == len(src)
    assert np.abs(r["T"] - P).max() < 1e-9 and r["rmse"] < 1e-9
    assert np.array_equal(r["corr"], np.arange(len(src)))


def test_oracle_ties_bound_and_empty_cases():
    tgt = np.array([[1.0, 0, 0], [-1.0, 0, 0], [5.0, 0, 0], [5.0, 0, 0], [9.5, 0, 0]], dtype=np.float32)
    src = np.array([[0.0, 0, 0], [5.0, 0.25, 0], [9.0, 0, 0], [20.0, 0, 0]], dtype=np.float32)
    for fp32 in (True, False):
        r = O.icp(src, tgt, None, 0.5, 0, fp32_round=fp32)
        # equidistant targets and duplicates -> the smallest row; d^2 == max_dist^2 is no correspondence
        assert r["corr"].tolist() == [-1, 2, -1, -1] and r["iterations"] == 0
        assert r["fitness"] == 0.25 and abs(r["rmse"] - 0.25) < 1e-12
    r = O.icp(src, tgt, None, 1.5, 0)
    assert r["corr"].tolist() == [0, 2, 4, -1]
    r = O.icp(src + np.float32(100.0), tgt, None, 0.5, 7)
    assert r["n_corr"] == 0 and r["rmse"] == 0.0 and r["iterations"] == 1 and np.array_equal(r["T"], np.eye(4))


@pytest.mark.parametrize("trans_m,rot_deg", [(0.05, 0.2), (0.15, 0.5)])
def test_oracle_variants_stop_after_the_same_number_of_iterations(trans_m, rot_deg):
    """The cases of tests/test_icp_gpu.py::test_converged_run: with the reference's criteria (1e-6 / 1e-6 / 200) the
    float32-rounded and the all-float64 restatement must stop at the same iteration and at the same pose, else the GPU
    test's iteration equality would rest on rounding luck.  (At 0.3 m / 1 deg they do not -- 59 against 73 iterations --
    which is why that case is not asserted anywhere: DESIGN section 15.)"""
    from scipy.spatial import cKDTree
    src, tgt = O.icp_case(trans_m, rot_deg)
    tree = cKDTree(tgt.astype(np.float64))
    a = O.icp(src, tgt, None, 0.2, 200, fp32_round=True, tree=tree)
    b = O.icp(src, tgt, None, 0.2, 200, fp32_round=False, tree=tree)
    rte, rre = O.pose_error(a["T"], b["T"])
    print(f"iterations {a['iterations']} / {b['iterations']}, pose difference {rte:.2e} m / {rre:.2e} deg, "
          f"correspondences {a['n_corr']} / {b['n_corr']}")
    assert 1 < a["iterations"] < 200
    assert a["iterations"] == b["iterations"]
    assert rte < 1e-6 and rre < 1e-4                            # arccos near 1 resolves ~1e-5 deg at best


def _variants_agree(src, tgt, max_dist=0.2, max_iteration=60, rel_fitness=1e-6, rel_rmse=1e-6, init=None):
    """Both arithmetic variants of the restatement on one input: the same iteration count, the same correspondence count,
    identical partners, poses less than 1e-6 m apart.  Exact equality of the kernel's partners with the float32 variant is
    asserted on the GPU only for inputs that pass this: the kernel differs from the float32 variant (Horn against SVD,
    summation order) by far less than the two variants differ from each other.  -> the float32 variant's result."""
    a = O.icp(src, tgt, init, max_dist, max_iteration, rel_fitness, rel_rmse, fp32_round=True)
    b = O.icp(src, tgt, init, max_dist, max_iteration, rel_fitness, rel_rmse, fp32_round=False)
    rte, _ = O.pose_error(a["T"], b["T"])
    assert a["iterations"] == b["iterations"] and a["n_corr"] == b["n_corr"]
    assert np.array_equal(a["corr"], b["corr"])
    assert rte < 1e-6
    return a


def test_ragged_batch_fixture_is_stable_under_rounding():
    tgts, srcs, top = O.ragged_batch()
    assert len({len(t) for t in tgts}) == 3 and [len(s) for s in srcs] == [1, 255, 256, 257, 513, 600, 64, 300]
    assert all(700 <= len(t) <= 3000 for t in tgts) and sorted(set(top)) == [0, 1, 2] and top != sorted(top)
    for t in tgts:                                               # coordinates of both signs on every axis
        assert (t.min(0) < 0).all() and (t.max(0) > 0).all()
    its = [_variants_agree(s, tgts[k])["iterations"] for s, k in zip(srcs, top)]
    print("iterations:", its)
    # the host looks at the flags after rounds 8, 16, 24, ...: problems that stop in the first, second and third chunk
    assert min(its) < 8 and any(9 <= i <= 15 for i in its) and max(its) >= 16 and max(its) < 60


def test_full_batch_fixture_is_stable_under_rounding():
    tgts, srcs = O.full_batch()
    assert len(tgts) == len(srcs) == 64
    assert all(200 <= len(t) <= 400 for t in tgts) and all(40 <= len(s) <= 300 for s in srcs)
    assert len({len(t) for t in tgts}) > 32 and len({len(s) for s in srcs}) > 32
    assert len({(len(s), len(t)) for s, t in zip(srcs, tgts)}) == 64
    its = [_variants_agree(s, t)["iterations"] for s, t in zip(srcs, tgts)]
    assert 1 <= min(its) and max(its) < 60 and len(set(its)) > 1


def test_chunk_fixtures_are_stable_under_rounding():
    tgt = O.chunk_target()
    fixed, batch = O.chunk_sources()
    assert len(fixed) == 600
    for k in (1, 7, 8, 9, 15, 16, 17):
        assert _variants_agree(fixed, tgt, 0.2, k, 0.0, 0.0)["iterations"] == k
    its = [_variants_agree(s, tgt, 0.2, 200)["iterations"] for s in batch]
    print("iterations:", its)
    assert its[0] < 8 and 9 <= its[1] <= 15 and 16 <= its[2] < 200
