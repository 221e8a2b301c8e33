"""Grid subsample, radius neighbours and kNN (apr_amd/csrc/points.hip) against the numpy oracle of tests/points_oracle.py at
the kernels' own edges (tests/points_cases.py; their conditions are asserted on the host by test_points_oracle_cpu.py).
Every comparison is exact -- the kNN band aside -- and every synchronisation-free or regrid route must equal its
synchronous twin.  Nothing here needs oracle/_ref."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import points_cases as PC  # noqa: E402
import points_oracle as O  # noqa: E402
from apr_amd import _lib  # noqa: E402
from apr_amd.predator import point_ops  # noqa: E402

pytestmark = pytest.mark.gpu
CANARY = 0x5A5A5A5A


# ------------------------------------------------------------------------------------------------- grid subsample
def _check_subsample(c, dev):
    pts = torch.from_numpy(c["points"]).to(dev)
    feats = None if c["features"] is None else torch.from_numpy(c["features"]).to(dev)
    want = O.grid_subsample(c["points"], c["lengths"], c["dl"], c["features"])
    got = point_ops.grid_subsample(pts, c["lengths"], c["dl"], feats)
    gf = got[2].cpu().numpy() if feats is not None else None
    assert got[1].dtype == np.int32 and len(got[0]) == int(got[1].sum())
    # lengths per cloud and canonical rows per cloud segment: a row filed under the wrong cloud fails either
    O.assert_subsample_equal(got[0].cpu().numpy(), got[1], want[0], want[1], gf, want[3] if feats is not None else None)
    twin = point_ops.grid_subsample_async(pts, c["lengths"], c["dl"], feats).finish()
    assert len(twin) == len(got) and np.array_equal(twin[1], got[1]) and twin[1].dtype == np.int32
    assert torch.equal(twin[0], got[0])
    if feats is not None:
        assert torch.equal(twin[2], got[2])


@pytest.mark.parametrize("name", list(PC.subsample_cases()))
def test_subsample_cell_populations(dev, name):
    _check_subsample(PC.subsample_cases()[name](), dev)


@pytest.mark.parametrize("n", PC.CELL_COUNTS)
def test_subsample_one_point_per_cell(dev, n):
    _check_subsample(PC.one_point_per_cell(n), dev)


def test_subsample_64_clouds_pass_and_65_are_refused(dev):
    _check_subsample(PC.many_clouds(PC.MAX_CLOUDS), dev)
    c = PC.many_clouds(PC.MAX_CLOUDS + 1)
    pts = torch.from_numpy(c["points"]).to(dev)
    with pytest.raises(_lib.AprHipError):
        point_ops.grid_subsample(pts, c["lengths"], c["dl"])
    with pytest.raises(_lib.AprHipError):
        point_ops.grid_subsample_async(pts, c["lengths"], c["dl"])


# ----------------------------------------------------------------------------------------------- radius neighbours
def _lens(c):
    if "q_lengths" in c:
        return c["q_lengths"], c["s_lengths"]
    return np.array([len(c["queries"])], np.int32), np.array([len(c["supports"])], np.int32)


def _flags(dev, n):
    """n flag pairs inside a canary buffer -> (flags [n, 2], the whole buffer)."""
    buf = torch.full((n * 2 + 64,), CANARY, dtype=torch.int32, device=dev)
    return buf[32:32 + 2 * n].view(n, 2), buf


def _check_radius(c, dev, limit=0):
    """The synchronous table against the oracle, entry for entry; the synchronisation-free table, the grid-keeping one and
    the one that searches the kept grid against the synchronous one; the largest count in the flag word."""
    q, s = torch.from_numpy(c["queries"]).to(dev), torch.from_numpy(c["supports"]).to(dev)
    ql, sl = _lens(c)
    want, counts = O.radius_neighbors(c["queries"], c["supports"], ql, sl, c["radius"], limit=limit)
    got = point_ops.radius_neighbors(q, s, ql, sl, c["radius"], limit=limit)
    assert got.dtype == torch.int32
    O.assert_table_equal(got.cpu().numpy(), want)
    lim = limit if limit > 0 else int(counts.max()) + 3          # above the largest count: finish cuts the padding back
    flags, buf = _flags(dev, 3)
    grid = point_ops.SearchGrid()
    tabs = [point_ops.radius_neighbors_async(q, s, ql, sl, c["radius"], lim, flags[0]),
            point_ops.radius_neighbors_async(q, s, ql, sl, c["radius"], lim, flags[1], keep_grid=grid)]
    assert grid.scratch is not None
    with O.counted_calls(_lib.load(), "apr_radius_neighbors_regrid_async") as regrid:
        tabs.append(point_ops.radius_neighbors_async(q, s, ql, sl, c["radius"], lim, flags[2], grid=grid))
    assert regrid.n == 1                                         # the kept grid was searched, not built again
    done = point_ops.finish_radius_tables(tabs, flags)
    for t in done:
        assert t.shape == got.shape and torch.equal(t, got)
    host = buf.cpu().numpy()
    assert (host[:32] == CANARY).all() and (host[38:] == CANARY).all()
    assert host[32:38].reshape(3, 2).tolist() == [[int(counts.max()), 0]] * 3
    return got.cpu().numpy(), want, counts


def test_radius_straddling_pairs_are_found(dev):
    """Pairs whose cells differ by 2 in a grid of edge r while the float32 d2 is below r^2: lost by a 3^3 probe on such a
    grid, found on the grid of edge 1.01 r."""
    cases = PC.straddling_case()
    assert sum(len(c["pairs"]) for c in cases) >= 3
    for c in cases:
        got, want, _ = _check_radius(c, dev)
        for qi, sj, _ in c["pairs"]:
            assert sj in got[qi], (c["radius"], qi, sj)


@pytest.mark.parametrize("limit", [1, 48, 1024])
def test_radius_hit_buffer_limits(dev, limit):
    c = PC.hit_buffer_case()
    got, want, counts = _check_radius(c, dev, limit)
    assert got.shape[1] == limit and counts[:4].tolist() == [1023, 1024, 1025, 2600]


def test_radius_hit_buffer_exactly_full(dev):
    """1023 and 1024 hits fit the rank buffer: the full width is ranked without a limit."""
    got, want, counts = _check_radius(PC.hit_buffer_case(counts=(1023, 1024)), dev)
    assert got.shape[1] == PC.HIT_CAP


def test_radius_more_columns_than_the_hit_buffer_raise(dev):
    c = PC.hit_buffer_case()
    q, s = torch.from_numpy(c["queries"]).to(dev), torch.from_numpy(c["supports"]).to(dev)
    ql, sl = _lens(c)
    for limit in (PC.HIT_CAP + 1, 0):
        with pytest.raises(_lib.AprHipError):
            point_ops.radius_neighbors(q, s, ql, sl, c["radius"], limit=limit)
    flags, _ = _flags(dev, 1)
    tab = point_ops.radius_neighbors_async(q, s, ql, sl, c["radius"], PC.HIT_CAP + 1, flags[0])
    with pytest.raises(_lib.AprHipError):
        point_ops.finish_radius_tables([tab], flags)


@pytest.mark.parametrize("total", [64, 256, 257])
@pytest.mark.parametrize("nq", [1, 3, 4, 5])
def test_radius_row_and_candidate_shapes(dev, total, nq):
    _check_radius(PC.candidate_case(total, nq), dev)
    _check_radius(PC.candidate_case(total, nq), dev, limit=7)


def test_radius_queries_outside_the_supports_box(dev):
    got, want, counts = _check_radius(PC.outside_box_case(), dev)
    assert (counts[-5:] == 0).all()


def test_radius_no_neighbour_at_all_gives_width_zero(dev):
    got, _, _ = _check_radius(PC.no_neighbour_case(), dev)
    assert got.shape == (9, 0)


@pytest.mark.parametrize("nb", [3, 5])
def test_radius_ragged_clouds_and_twin_clouds_stay_apart(dev, nb):
    c = PC.ragged_clouds_case(nb)
    got, _, _ = _check_radius(c, dev)
    _check_radius(c, dev, limit=5)
    qs, ss = np.concatenate([[0], np.cumsum(c["q_lengths"])]), np.concatenate([[0], np.cumsum(c["s_lengths"])])
    for b in range(nb):
        t = got[qs[b]:qs[b + 1]]
        real = t[t != len(c["supports"])]
        assert (real >= ss[b]).all() and (real < ss[b + 1]).all()


def test_radius_grid_beyond_the_margin_fails_loudly_on_every_route(dev):
    """Supports over more cells than the grid's 1 % margin covers: an error on the synchronous call, a raised flag on the
    synchronisation-free and the regrid routes -- never a table."""
    c = PC.grid_range_case()
    q, s = torch.from_numpy(c["queries"]).to(dev), torch.from_numpy(c["supports"]).to(dev)
    ql, sl = _lens(c)
    with pytest.raises(_lib.AprHipError):
        point_ops.radius_neighbors(q, s, ql, sl, c["radius"])
    with pytest.raises(_lib.AprHipError):
        point_ops.radius_neighbors(q, s, ql, sl, c["radius"], limit=4)
    flags, _ = _flags(dev, 2)
    grid = point_ops.SearchGrid()
    t0 = point_ops.radius_neighbors_async(q, s, ql, sl, c["radius"], 4, flags[0], keep_grid=grid)
    with O.counted_calls(_lib.load(), "apr_radius_neighbors_regrid_async") as regrid:
        t1 = point_ops.radius_neighbors_async(q, s, ql, sl, c["radius"], 4, flags[1], grid=grid)
    assert regrid.n == 1                                         # the status is the one the earlier build left
    torch.cuda.synchronize()
    assert flags.cpu()[:, 1].tolist() == [19, 19]
    for t, f in ((t0, flags[0:1]), (t1, flags[1:2])):
        with pytest.raises(_lib.AprHipError):
            point_ops.finish_radius_tables([t], f)
    # the same supports at a radius whose grid is in range: a table again
    c2 = dict(c, radius=0.02)
    _check_radius(c2, dev)


def test_radius_direct_call_writes_its_table_and_flags_only(dev):
    """apr_radius_neighbors_async, then apr_radius_neighbors_regrid_async on the scratch it left, each with its table and
    its flag words carved out of canary buffers."""
    c = PC.candidate_case(257, 5)
    lib = _lib.load()
    q, s = torch.from_numpy(c["queries"]).to(dev), torch.from_numpy(c["supports"]).to(dev)
    nq, ns, lim = len(c["queries"]), len(c["supports"]), 9
    ql, sl = _lens(c)
    sb = int(lib.apr_radius_scratch_bytes(nq, ns))
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
    want, counts = O.radius_neighbors(c["queries"], c["supports"], ql, sl, c["radius"], limit=lim)
    for entry in (lib.apr_radius_neighbors_async, lib.apr_radius_neighbors_regrid_async):
        buf = torch.full((nq * lim + 512,), CANARY, dtype=torch.int32, device=dev)
        out = buf[256:256 + nq * lim]
        flags, fbuf = _flags(dev, 1)
        _lib.check(entry(_lib.ptr(q), nq, _lib.ptr(s), ns, ql.ctypes.data_as(C.c_void_p), sl.ctypes.data_as(C.c_void_p), 1,
                         float(c["radius"]), lim, _lib.ptr(out), lim, _lib.ptr(flags), _lib.ptr(scratch), sb, _lib.stream()))
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:256] == CANARY).all() and (host[256 + nq * lim:] == CANARY).all()
        O.assert_table_equal(host[256:256 + nq * lim].reshape(nq, lim), want)
        fh = fbuf.cpu().numpy()
        assert fh[32:34].tolist() == [int(counts.max()), 0] and (np.delete(fh, [32, 33]) == CANARY).all()


# ------------------------------------------------------------------------------------------------------------ kNN
@pytest.mark.parametrize("n", PC.KNN_N)
def test_knn_exact_on_lattices(dev, n):
    p = PC.knn_lattice(n)
    t = torch.from_numpy(p).to(dev)
    for k, skip in PC.KNN_K:
        O.assert_knn_exact(point_ops.knn(t, k, skip_first=skip).cpu().numpy(), p, k, skip)


def test_knn_k_plus_skip_of_17_is_refused(dev):
    t = torch.from_numpy(PC.knn_lattice(65)).to(dev)
    with pytest.raises(_lib.AprHipError):
        point_ops.knn(t, 16, skip_first=True)
    with pytest.raises(_lib.AprHipError):
        point_ops.knn(t, 17, skip_first=False)


@pytest.mark.parametrize("n,seed,half", PC.KNN_UNIFORM)
def test_knn_banded_on_uniform_clouds(dev, n, seed, half):
    p = PC.knn_uniform(n, seed, half)
    t = torch.from_numpy(p).to(dev)
    for k, skip in ((10, True), (16, False), (15, True)):
        O.knn_banded(point_ops.knn(t, k, skip_first=skip).cpu().numpy(), p, k, skip)
