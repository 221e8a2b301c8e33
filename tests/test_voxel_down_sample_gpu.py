"""apr_voxel_down_sample (apr_amd/csrc/voxel.hip) against the float64 oracle of tests/voxel_oracle.py: every output array
bit for bit, no tolerance.  The cases are tests/voxel_cases.py's; tests/test_voxel_oracle_cpu.py shows on the CPU that each
of them tells a wrong implementation (fp32 indices, fp32 sums, no half voxel, reversed sums) from the right one."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_cases as VC  # noqa: E402
import voxel_oracle as VO  # noqa: E402
from apr_amd import _lib, ops, synth  # noqa: E402
from apr_amd.fcgf import registration  # noqa: E402

pytestmark = pytest.mark.gpu
ALL = ops.VOXEL_OUTPUTS


def _run(c, dev, want=ALL):
    got, lens = ops.voxel_down_sample(torch.from_numpy(c["points"]).to(dev), c["lengths"], c["voxel"], want=want)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    got["lengths"] = lens
    return got


def _check(c, dev):
    want = VO.voxel_down_sample(c["points"], c["lengths"], c["voxel"])
    got = _run(c, dev)
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k
    return got


@pytest.mark.parametrize("voxel", [0.3, 0.5])
def test_boundary_rows(dev, voxel):
    _check(VC.boundary_rows(voxel), dev)


def test_order_sensitive_sums(dev):
    _check(VC.order_sensitive(), dev)


def test_crowded_voxels_at_every_internal_capacity(dev):
    """voxel.hip: kVoxStage = 341 (rows staged per round by the wave kernel), kVoxWaveCap = 1024 (rows a wave sorts; more
    go to the workgroup kernel), kVoxBigStage = 1024 (its rows per round), kVoxBigLds = 8192 (rows it sorts in LDS; more
    are sorted in global memory).  VC.CROWDED_COUNTS holds each, one below and one above (or its double and one above)."""
    assert (VC.K_VOX_STAGE, VC.K_VOX_WAVE_CAP, VC.K_VOX_BIG_STAGE, VC.K_VOX_BIG_LDS) == (341, 1024, 1024, 8192)
    got = _check(VC.crowded(), dev)
    assert sorted(got["count"].tolist()) == sorted((1,) + VC.CROWDED_COUNTS)


@pytest.mark.parametrize("name", list(VC.shapes()))
def test_shapes(dev, name):
    _check(VC.shapes()[name], dev)


def test_a_cloud_gives_the_same_bits_alone_and_in_a_batch_and_run_to_run(dev):
    c = VC.shapes()["twice_in_a_batch"]
    a = _run(c, dev)
    n0, n1, n2 = a["lengths"]
    alone = _run(VC.case(c["points"][:300], [300], c["voxel"]), dev)
    for k in ("centroid", "centroid32", "count", "index", "first"):
        assert np.array_equal(a[k][:n0], alone[k]), k
        if k != "first":
            assert np.array_equal(a[k][n0 + n1:], alone[k]), k
    assert np.array_equal(a["first"][n0 + n1:], alone["first"] + 817)
    b = _run(c, dev)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_any_output_may_be_left_out(dev):
    c = VC.shapes()["batch_of_three"]
    full = _run(c, dev)
    for k in ALL:
        got = _run(c, dev, want=(k,))
        assert set(got) == {k, "lengths"} and np.array_equal(got[k], full[k]) and np.array_equal(got["lengths"], full["lengths"])
    assert np.array_equal(_run(c, dev, want=())["lengths"], full["lengths"])


def test_public_mirror_returns_the_float64_centroids(dev):
    c = VC.shapes()["n257"]
    want = VO.voxel_down_sample(c["points"], c["lengths"], c["voxel"])["centroid"]
    got = registration.voxel_down_sample(c["points"], c["voxel"])
    assert got.dtype == torch.float64 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)


@pytest.fixture(scope="module")
def scans():
    return synth.make_small_frame(0), synth.make_frame(0)


def test_small_frame(dev, scans):
    assert len(scans[0]) == 19750
    _check(VC.case(scans[0], [len(scans[0])], 0.3), dev)


def test_full_size_scan(dev, scans):
    assert len(scans[1]) > 100000
    _check(VC.case(scans[1], [len(scans[1])], 0.3), dev)


def test_errors(dev):
    far = torch.tensor([[0, 0, 0], [1500, 0, 0]], dtype=torch.float32, device=dev)
    with pytest.raises(_lib.AprHipError, match="error -3"):
        ops.voxel_down_sample(far, [2], 0.01)
    ops.voxel_down_sample(far, [2], 0.0115)
    bad = torch.tensor([[0, 0, 0], [float("nan"), 0, 0], [1, 1, 1]], dtype=torch.float32, device=dev)
    with pytest.raises(_lib.AprHipError, match="error -3"):
        ops.voxel_down_sample(bad, [3], 0.3)
    with pytest.raises(_lib.AprHipError, match="error -3"):
        ops.voxel_down_sample(torch.full((2, 3), float("inf"), device=dev), [2], 0.3)
    ok = torch.zeros((4, 3), device=dev)
    for lens, voxel in (([4], 0.0), ([4], -1.0), ([3], 0.3), ([4, 0], 0.3), ([1] * 65, 0.3)):
        with pytest.raises(_lib.AprHipError, match="error -1"):
            ops.voxel_down_sample(ok if len(lens) < 65 else torch.zeros((65, 3), device=dev), lens, voxel)
    # the device is still sound
    _check(VC.shapes()["n63"], dev)
