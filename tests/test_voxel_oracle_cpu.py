"""The cases of tests/test_voxel_down_sample_gpu.py keep their teeth: each is paired with a mutant oracle -- a plausible wrong
implementation -- and must tell it from the right one.  Runs on the CPU; the oracle is tests/voxel_oracle.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_cases as VC  # noqa: E402
import voxel_oracle as VO  # noqa: E402

PAIRS = [
    ("boundary_0.3", lambda: VC.boundary_rows(0.3), "fp32_index"),
    ("boundary_0.3", lambda: VC.boundary_rows(0.3), "no_half_voxel"),
    ("boundary_0.5", lambda: VC.boundary_rows(0.5), "no_half_voxel"),
    ("order_sensitive", VC.order_sensitive, "reversed_sums"),
    ("order_sensitive", VC.order_sensitive, "fp32_sums"),
    ("crowded", VC.crowded, "reversed_sums"),
    ("crowded", VC.crowded, "fp32_sums"),
]


def run(c, **kw):
    return VO.voxel_down_sample(c["points"], c["lengths"], c["voxel"], **kw)


@pytest.mark.parametrize("name,make,mutant", PAIRS, ids=[f"{n}-{m}" for n, _, m in PAIRS])
def test_case_tells_the_mutant_from_the_oracle(name, make, mutant):
    c = make()
    assert VO.differs(run(c), run(c, **VO.MUTANTS[mutant]))


def test_boundary_rows_sit_on_the_voxel_faces():
    """voxel 0.5: the rows are exactly origin + k * 0.5, so row 3k-1 (below) belongs to voxel k-1 and rows 3k, 3k+1 to k;
    voxel 0.3: fp32 index arithmetic files some rows in other voxels."""
    c = VC.boundary_rows(0.5)
    lo = np.float64(np.float32(-37.123))
    x = c["points"][1:601, 0].astype(np.float64).reshape(200, 3)
    assert np.array_equal(x[:, 1], lo - 0.25 + 0.5 * np.arange(1, 201))
    r = run(c)
    assert r["count"][0] == 1 + 3          # the corner row and the three rows just below the first face
    c3 = VC.boundary_rows(0.3)
    a, b = run(c3), run(c3, index_dtype=np.float32)
    assert not np.array_equal(a["count"], b["count"]) or not np.array_equal(a["index"], b["index"])


def test_reversed_order_moves_a_centroid_by_one_rounding():
    c = VC.order_sensitive()
    a, b = run(c), run(c, reverse=True)
    d = np.abs(a["centroid"] - b["centroid"]).max()
    assert 0 < d < 1e-16


def test_crowded_counts_are_the_named_capacities():
    r = run(VC.crowded())
    assert sorted(r["count"].tolist()) == sorted((1,) + VC.CROWDED_COUNTS)


@pytest.mark.parametrize("name", ["n1", "n63", "n65", "n257", "one_voxel", "batch_of_three", "twice_in_a_batch", "shuffled"])
def test_vectorised_oracle_is_the_dict_loop(name):
    c = VC.shapes()[name]
    assert not VO.differs(run(c), VO.voxel_down_sample_dict(c["points"], c["lengths"], c["voxel"]))


def test_dict_loop_on_the_order_sensitive_case():
    c = VC.order_sensitive()
    assert not VO.differs(run(c), VO.voxel_down_sample_dict(c["points"], c["lengths"], c["voxel"]))


def test_batch_structure():
    s = VC.shapes()
    r = run(s["twice_in_a_batch"])
    n0, n1, n2 = r["lengths"]
    assert n0 == n2
    for k in ("centroid", "centroid32", "count", "index"):
        assert np.array_equal(r[k][:n0], r[k][n0 + n1:])
    assert np.array_equal(r["first"][:n0] + 817, r["first"][n0 + n1:])
    one = run(s["one_voxel"])
    assert one["lengths"].tolist() == [1] and one["count"].tolist() == [100] and one["first"].tolist() == [0]
    sh = run(s["shuffled"])
    assert (np.diff(sh["first"]) > 0).all()


def test_range_errors():
    far = np.array([[0, 0, 0], [1500, 0, 0]], np.float32)
    with pytest.raises(VO.VoxelRangeError):
        VO.voxel_down_sample(far, [2], 0.01)
    VO.voxel_down_sample(far, [2], 0.0115)      # 1500 / 0.0115 = 130 435 <= 131 071
    bad = np.array([[0, 0, 0], [np.nan, 0, 0]], np.float32)
    with pytest.raises(VO.VoxelRangeError):
        VO.voxel_down_sample(bad, [2], 0.3)
