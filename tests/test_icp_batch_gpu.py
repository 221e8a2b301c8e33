"""The batch layout of apr_icp_batch (csrc/icp.hip) against the host restatement (tests/icp_oracle.py): ragged batches over
several target segments, the default problem -> segment mapping at the 64-problem limit, the chunked rounds, the search
grid's geometry and its cell range.

Partners are compared EXACTLY with the float32-rounded variant of the restatement.  That is a condition, not a measurement:
tests/test_icp_cpu.py asserts for these very inputs that the float32-rounded and the all-float64 variant stop at the same
iteration with identical partners, and those two differ from each other by far more than the kernel differs from the
float32 variant (Horn against SVD, summation order: last bits of T)."""
import functools
import time

import numpy as np
import pytest
import torch

from tests import icp_oracle as O

pytestmark = pytest.mark.gpu

BAR_M, BAR_DEG = 1e-3, 1e-3


def _batch(dev, srcs, tgts, top, max_dist=0.2, max_iteration=60, rel_fitness=1e-6, rel_rmse=1e-6):
    """-> (records float64 [nb, 20] on the device, corr int32 on the device, source offsets)."""
    from apr_amd import ops
    s = torch.from_numpy(np.concatenate(srcs)).to(dev)
    t = torch.from_numpy(np.concatenate(tgts)).to(dev)
    so = np.concatenate([[0], np.cumsum([len(x) for x in srcs])])
    to = np.concatenate([[0], np.cumsum([len(x) for x in tgts])])
    rec, corr = ops.icp_batch(s, so, t, to, np.tile(np.eye(4), (len(srcs), 1, 1)), max_dist, max_iteration, rel_fitness,
                              rel_rmse, tgt_of_problem=top, want_corr=True)
    return rec, corr, so


def _single(dev, src, tgt, **kw):
    rec, corr, _ = _batch(dev, [src], [tgt], None, **kw)
    return rec[0], corr


@functools.lru_cache(maxsize=None)
def _want(case, i, max_iteration=60, thresholds=1e-6):
    """The float32-rounded oracle on problem i of a fixture, computed once per session."""
    if case == "ragged":
        tgts, srcs, top = O.ragged_batch()
        src, tgt = srcs[i], tgts[top[i]]
    elif case == "full":
        tgts, srcs = O.full_batch()
        src, tgt = srcs[i], tgts[i]
    elif case == "chunk_fixed":
        src, tgt = O.chunk_sources()[0], O.chunk_target()
    else:
        src, tgt = O.chunk_sources()[1][i], O.chunk_target()
    return O.icp(src, tgt, None, 0.2, max_iteration, thresholds, thresholds, fp32_round=True)


def _assert_record(rec_row, corr_slice, want, what):
    """iterations, n_corr, fitness and the partners exactly; rmse to 1e-6 relative; the pose inside the project's bar."""
    r = rec_row.cpu().numpy()
    corr = corr_slice.cpu().numpy().astype(np.int64)
    rte, rre = O.pose_error(r[:16].reshape(4, 4), want["T"])
    rows = int((corr != want["corr"]).sum())
    print(f"{what}: iterations {int(r[19])} / {want['iterations']}, correspondences {int(r[18])} / {want['n_corr']}, {rows} rows "
          f"differ, pose difference {rte:.2e} m / {rre:.2e} deg, rmse {r[17]:.9f} / {want['rmse']:.9f}")
    assert int(r[19]) == want["iterations"], what
    assert int(r[18]) == want["n_corr"] and r[16] == want["fitness"], what
    assert np.array_equal(corr, want["corr"]), what
    assert abs(r[17] - want["rmse"]) <= 1e-6 * want["rmse"], what
    assert rte < BAR_M and rre < BAR_DEG, what
    assert np.isfinite(r).all(), what


def test_ragged_batch_over_three_targets(dev):
    """Eight problems of 1, 255, 256, 257, 513, 600, 64 and 300 rows on three segments of 3000, 700 and 1900 rows named in
    the order [2, 0, 2, 1, 0, 1, 2, 0]: the problem -> workgroup table, the per-segment origin and key, and the rebasing of
    corr.  The oracle stops after 2, 4, 5, 4, 6, 6, 12 and 17 iterations: inside the first, second and third chunk."""
    t0 = time.perf_counter()
    tgts, srcs, top = O.ragged_batch()
    rec, corr, off = _batch(dev, srcs, tgts, top)
    for i in range(len(srcs)):
        _assert_record(rec[i], corr[off[i]:off[i + 1]], _want("ragged", i), f"problem {i}")
    # alone on its own segment: the same bits
    for i in range(len(srcs)):
        rec_1, corr_1 = _single(dev, srcs[i], tgts[top[i]])
        assert torch.equal(rec_1, rec[i]) and torch.equal(corr_1, corr[off[i]:off[i + 1]]), f"problem {i} alone"
    # the same problems in another order: the same bits per problem
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    rec_p, corr_p, off_p = _batch(dev, [srcs[j] for j in perm], tgts, [top[j] for j in perm])
    for k, j in enumerate(perm):
        assert torch.equal(rec_p[k], rec[j]), f"problem {j} at position {k}"
        assert torch.equal(corr_p[off_p[k]:off_p[k + 1]], corr[off[j]:off[j + 1]]), f"problem {j} at position {k}"
    print(f"wall time {time.perf_counter() - t0:.2f} s")


def test_no_partner_leaks_from_another_segment(dev):
    """Segment 1 is segment 0 moved by 5 cm: a search that ignored the segment in the cell key or the origin would find
    most partners in the wrong one.  The same source on either segment must see its own segment only.  The source is built
    from the cloud halfway between the two (not from segment 0, as the issue words it): built on segment 0, 7 of 400 rows
    would leak one way at max_iteration 0; halfway, more than 20 rows would leak in each direction, which is asserted."""
    t0 = time.perf_counter()
    seg0 = O.box_cloud(1500, 700)
    seg1 = np.ascontiguousarray((seg0.astype(np.float64) + 0.05).astype(np.float32))
    # the source lies between the two: over the union its rows would find their partners in either segment
    src = O.box_source(np.ascontiguousarray((seg0.astype(np.float64) + 0.025).astype(np.float32)), 400, 0, 701)
    both = np.concatenate([seg0, seg1])
    for max_iteration in (0, 5):
        want = [O.icp(src, t, None, 0.2, max_iteration, 0.0, 0.0, fp32_round=True) for t in (seg0, seg1)]
        union = O.icp(src, both, None, 0.2, max_iteration, 0.0, 0.0, fp32_round=True)["corr"]
        # a leak would show: over the union, each problem would pick partners from the other segment
        leak0 = int((union >= len(seg0)).sum())
        leak1 = int(((union >= 0) & (union < len(seg0))).sum())
        print(f"max_iteration {max_iteration}: over the union {leak0} / {leak1} of {len(src)} rows would take a partner from "
              "the other segment")
        assert leak0 > 20 and leak1 > 20
        assert not np.array_equal(union, want[0]["corr"]) and not np.array_equal(union - len(seg0), want[1]["corr"])
        rec, corr, off = _batch(dev, [src, src], [seg0, seg1], [0, 1], max_iteration=max_iteration, rel_fitness=0.0,
                                rel_rmse=0.0)
        for i in range(2):
            r = rec[i].cpu().numpy()
            got = corr[off[i]:off[i + 1]].cpu().numpy().astype(np.int64)
            assert np.array_equal(got, want[i]["corr"])
            assert int(r[18]) == want[i]["n_corr"] and r[16] == want[i]["fitness"] and int(r[19]) == max_iteration
    print(f"wall time {time.perf_counter() - t0:.2f} s")


def test_default_mapping_at_the_problem_limit(dev):
    """64 problems on 64 segments without tgt_of_problem (problem i -> segment i), every length different."""
    t0 = time.perf_counter()
    tgts, srcs = O.full_batch()
    rec, corr, off = _batch(dev, srcs, tgts, None)
    for i in range(64):
        _assert_record(rec[i], corr[off[i]:off[i + 1]], _want("full", i), f"problem {i}")
    for i in (0, 31, 63):
        rec_1, corr_1 = _single(dev, srcs[i], tgts[i])
        assert torch.equal(rec_1, rec[i]) and torch.equal(corr_1, corr[off[i]:off[i + 1]]), f"problem {i} alone"
    print(f"wall time {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("kind", ["65_problems", "65_segments", "segment_out_of_range", "empty_source", "empty_segment"])
def test_batch_limits_are_refused(dev, kind):
    """Argument checks on the host (tests/test_icp_cpu.py shows with dummy pointers that they run before any launch)."""
    from apr_amd import _lib
    tgts, srcs = O.full_batch(3)
    empty = np.zeros((0, 3), dtype=np.float32)
    srcs_, tgts_, top = {"65_problems": ([srcs[0]] * 65, tgts[:1], [0] * 65),
                         "65_segments": (srcs, [tgts[0]] * 65, [0, 64, 1]),
                         "segment_out_of_range": (srcs, tgts, [0, 3, 1]),
                         "empty_source": ([srcs[0], empty, srcs[2]], tgts, None),
                         "empty_segment": (srcs, [tgts[0], empty, tgts[2]], [0, 2, 0])}[kind]
    with pytest.raises(_lib.AprHipError, match="apr_icp_batch"):
        _batch(dev, srcs_, tgts_, top)


def test_fixed_round_counts_across_the_chunk_boundaries(dev):
    """Both thresholds 0: exactly max_iteration iterations, for counts on either side of the chunks of 8 rounds."""
    t0 = time.perf_counter()
    tgt = O.chunk_target()
    src, _ = O.chunk_sources()
    recs = {}
    for k in (1, 7, 8, 9, 15, 16, 17):
        rec, corr = _single(dev, src, tgt, max_iteration=k, rel_fitness=0.0, rel_rmse=0.0)
        _assert_record(rec, corr, _want("chunk_fixed", 0, k, 0.0), f"max_iteration {k}")
        assert int(rec[19]) == k
        recs[k] = rec
    for k in (7, 8, 15, 16):                                    # the extra round ran
        assert not torch.equal(recs[k], recs[k + 1])
    print(f"wall time {time.perf_counter() - t0:.2f} s")


def test_problems_that_stop_in_different_chunks(dev):
    """Three problems on one target that the oracle stops after 3, 10 and 19 iterations: the first is finished when the host
    first looks at the flags, the third runs on after the second look."""
    t0 = time.perf_counter()
    tgt = O.chunk_target()
    _, srcs = O.chunk_sources()
    want = [_want("chunk_batch", i, 200) for i in range(3)]
    assert want[0]["iterations"] < 8 and 9 <= want[1]["iterations"] <= 15 and want[2]["iterations"] >= 16
    rec, corr, off = _batch(dev, srcs, [tgt], [0, 0, 0], max_iteration=200)
    for i in range(3):
        _assert_record(rec[i], corr[off[i]:off[i + 1]], want[i], f"problem {i}")
        rec_1, corr_1 = _single(dev, srcs[i], tgt, max_iteration=200)
        assert torch.equal(rec_1, rec[i]) and torch.equal(corr_1, corr[off[i]:off[i + 1]]), f"problem {i} alone"
    print(f"wall time {time.perf_counter() - t0:.2f} s")


def _brute_partners(p, tgt, max_dist):
    """float32 arg-min over ALL targets, the kernel's d^2 and tie rule."""
    d = p[:, None, :].astype(np.float32) - tgt[None, :, :].astype(np.float32)
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == np.float32
    row = d2.argmin(1)                                          # the first minimum = the smallest row
    r = np.float32(max_dist)
    return np.where(d2[np.arange(len(p)), row] < r * r, row, -1)


@pytest.mark.parametrize("name", ["one_cell", "far", "outside", "cell_faces"])
def test_grid_geometry(dev, name):
    t0 = time.perf_counter()
    src, tgt, max_dist = O.geometry_cases()[name]
    for max_iteration in (0, 5):
        want = O.icp(src, tgt, None, max_dist, max_iteration, 0.0, 0.0, fp32_round=True)
        rec, corr = _single(dev, src, tgt, max_dist=max_dist, max_iteration=max_iteration, rel_fitness=0.0, rel_rmse=0.0)
        r = rec.cpu().numpy()
        got = corr.cpu().numpy().astype(np.int64)
        T = r[:16].reshape(4, 4)
        # the pose where the cloud is (at 2 km from the origin a pose's translation is mostly lever arm)
        moved = np.abs(O.transform(T, src, False) - O.transform(want["T"], src, False)).max()
        print(f"{name}, max_iteration {max_iteration}: correspondences {int(r[18])} / {want['n_corr']}, "
              f"{int((got != want['corr']).sum())} rows differ, source rows moved {moved:.2e} m apart")
        assert np.array_equal(got, want["corr"])
        assert int(r[18]) == want["n_corr"] and r[16] == want["fitness"] and int(r[19]) == max_iteration
        assert np.isfinite(r).all() and moved < BAR_M
        if max_iteration == 0:
            assert np.array_equal(got, _brute_partners(src, tgt, max_dist))
        if name == "one_cell":
            assert (got >= 0).all()
            assert np.array_equal(got, _brute_partners(O.transform(T, src, True), tgt, max_dist))
        if name == "outside":
            assert (got[-8:] == -1).all() and int(r[18]) > 200
        if name == "cell_faces":
            assert (got >= 0).all()
    print(f"wall time {time.perf_counter() - t0:.2f} s")


def test_target_beyond_the_cell_range_is_refused(dev):
    """Two clusters of targets 150 m apart at max_dist = 1 mm need 1.5e5 cells along x, beyond the 2^17 the packed cell key
    holds; 45 m apart they need 4.5e4, inside the key but beyond the index up to which the 1 % widening of the cell covers
    the float32 rounding of the cell coordinate.  Both must be refused, never answered with partners
    missing or taken from an aliased cell.  30 m apart (3.1e4 cells) the answer is the oracle's."""
    from apr_amd import _lib
    t0 = time.perf_counter()
    for gap in (150.0, 45.0):
        src, tgt = O.range_case(gap)
        want = O.icp(src, tgt, None, O.RANGE_MAX_DIST, 0, fp32_round=True)
        assert np.array_equal(want["corr"], np.arange(400))     # the oracle pairs every row
        for max_iteration in (0, 5):
            with pytest.raises(_lib.AprHipError, match="cell range"):
                _single(dev, src, tgt, max_dist=O.RANGE_MAX_DIST, max_iteration=max_iteration)
    src, tgt = O.range_case(30.0)
    assert (tgt.max(0) - tgt.min(0)).max() / (np.float32(O.RANGE_MAX_DIST) * np.float32(1.01)) < 2 ** 15
    for max_iteration in (0, 5):
        want = O.icp(src, tgt, None, O.RANGE_MAX_DIST, max_iteration, 0.0, 0.0, fp32_round=True)
        rec, corr = _single(dev, src, tgt, max_dist=O.RANGE_MAX_DIST, max_iteration=max_iteration, rel_fitness=0.0,
                            rel_rmse=0.0)
        r = rec.cpu().numpy()
        assert np.array_equal(corr.cpu().numpy().astype(np.int64), want["corr"]) and (want["corr"] == np.arange(400)).all()
        assert int(r[18]) == 400 and r[16] == 1.0 and int(r[19]) == max_iteration and np.isfinite(r).all()
    # the refused call leaves the library usable
    rec, _ = _single(dev, src, tgt, max_dist=O.RANGE_MAX_DIST, max_iteration=0)
    assert int(rec[18]) == 400
    print(f"wall time {time.perf_counter() - t0:.2f} s")
