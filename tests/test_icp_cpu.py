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


def _call(lib, src_off, tgt_off, nb, max_dist=0.2, max_iteration=5):
    """apr_icp_batch with dummy (never dereferenced) device pointers: only the argument checks may run."""
    so = np.asarray(src_off, dtype=np.int64)
    to = np.asarray(tgt_off, dtype=np.int64)
    dummy = C.c_void_p(256)
    return lib.apr_icp_batch(dummy, so.ctypes.data_as(C.c_void_p), dummy, to.ctypes.data_as(C.c_void_p), len(to) - 1, None,
                             nb, dummy, max_dist, max_iteration, 1e-6, 1e-6, dummy, None, dummy, 1 << 40, None)


@pytest.mark.parametrize("kind", ["no_problem", "empty_source", "zero_max_dist", "negative_max_dist", "negative_iterations"])
def test_bad_arguments_are_rejected_before_any_launch(lib, kind):
    rc = {"no_problem": lambda: _call(lib, [0], [0, 10], 0),
          "empty_source": lambda: _call(lib, [0, 0], [0, 10], 1),
          "zero_max_dist": lambda: _call(lib, [0, 10], [0, 10], 1, max_dist=0.0),
          "negative_max_dist": lambda: _call(lib, [0, 10], [0, 10], 1, max_dist=-0.2),
          "negative_iterations": lambda: _call(lib, [0, 10], [0, 10], 1, max_iteration=-1)}[kind]()
    assert rc == -1                                             # APR_EINVAL
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
