"""Voxelisation, map builds, kernel maps, pyramids, fills and packs (apr_amd/csrc/hash.hip, apr_voxel_pyramid in encoder.hip)
against the numpy oracle of tests/hash_oracle.py at the kernels' own edges (tests/hash_cases.py; every planted fact is
asserted on the host by test_hash_oracle_cpu.py).  Everything is an integer (the representative points are copies of input
floats) and every comparison is array_equal over whole arrays.  Nothing here needs oracle/_ref."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hash_cases as HC  # noqa: E402
import hash_oracle as O  # noqa: E402
from apr_amd import ops  # noqa: E402
from apr_amd._lib import AprHipError  # noqa: E402
from apr_amd.MinkowskiEngine.core import CoordinateManager  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A
MAP_CASES = HC.map_cases()
KMAP_CASES = HC.kernel_map_cases()
RAISING = [n for n, d in MAP_CASES.items() if "oor" in d]
CLEAN = [n for n in MAP_CASES if n not in RAISING]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _eq(t, want):
    got = t.cpu().numpy()
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def _n_dev(n_live, dev):
    return None if n_live is None else torch.tensor([n_live], dtype=torch.int32, device=dev)


def _build(d, dev):
    """An unfinalised build of a map case and what the device holds: -> (map, coords[:n], first[:n], n, status, counts)."""
    n = len(d["rows"])
    offsets = [0, n // 3, n // 3, n - 1, n]                      # an empty segment and a segment of one row
    m = ops.build_map(_t(d["rows"], dev), d["floor_to"], n_in_dev=_n_dev(d["n_live"], dev), want_first=True)
    counts = ops.segment_counts(m, torch.tensor(offsets, dtype=torch.int64, device=dev))
    n_out, status = int(m.n_dev.item()), int(m.status.item())
    return m, m.coords[:n_out], m.first[:n_out], n_out, status, counts, offsets


def _check_build(d, dev):
    want_rows, want_first, want_status = O.build_map(d["rows"], d["floor_to"], d["n_live"])
    m, rows, first, n_out, status, counts, offsets = _build(d, dev)
    assert n_out == len(want_rows) and status == want_status
    assert _eq(rows, want_rows) and _eq(first, want_first)
    assert _eq(counts, O.segment_counts(want_first, offsets))
    return m, want_rows


def _map(rows, dev):
    """A finalised map over unique rows: its rows are the input rows, in order."""
    m = ops.build_map(_t(rows, dev))
    ops.finalize_maps([m])
    assert m.n == len(rows) and _eq(m.coords, np.ascontiguousarray(rows, np.int32))
    return m


def _generic(out_map, in_map, ks, scale, n_out_dev=None, nbr=None):
    """apr_kernel_map itself (ops.kernel_map sends same-level 5^3 / 7^3 maps to the symmetric kernel)."""
    nbr = torch.empty((out_map.n, ks ** 3), dtype=torch.int32, device=out_map.coords.device) if nbr is None else nbr
    ops.check(ops._lib_().apr_kernel_map(ops.ptr(out_map.coords), out_map.n, ops.ptr(n_out_dev), ops.ptr(in_map.keys), ops.ptr(in_map.vals),
                                        in_map.cap, ks, scale, ops.ptr(nbr), ops.stream()))
    return nbr


def _same(m, ks, scale):
    """apr_kernel_map_same itself, into a table full of a sentinel: it must write every entry."""
    nbr = torch.full((m.n, ks ** 3), SENTINEL, dtype=torch.int32, device=m.coords.device)
    ops.check(ops._lib_().apr_kernel_map_same(ops.ptr(m.coords), m.n, ops.ptr(m.keys), ops.ptr(m.vals), m.cap, ks, scale, ops.ptr(nbr),
                                             ops.stream()))
    return nbr


# ------------------------------------------------------------------------------------------------- voxelisation
@pytest.mark.parametrize("vs", HC.VOXEL_SIZES)
def test_voxelize_planted_values(dev, vs):
    v = HC.voxel_values(vs)
    xyz = np.concatenate([v["inside"], v["outside"]])
    t = _t(xyz, dev)
    assert _eq(ops.voxelize(t, vs, 5), O.voxelize(xyz, vs, 5))
    cuts = [0, 7, 7, 64, len(xyz)]                               # an empty frame, a frame that ends on a wave boundary
    want = O.voxelize(xyz, vs, np.repeat(np.arange(4), np.diff(cuts)))
    assert _eq(ops.voxelize_segments(t, vs, torch.tensor(cuts, dtype=torch.int64, device=dev)), want)
    coords, offs_dev, offs = ops.voxelize_frames([t[a:b] for a, b in zip(cuts, cuts[1:])], vs)
    assert _eq(coords, want) and offs == cuts and offs_dev.tolist() == cuts
    # the in-range rows build; each first out-of-range value, on each axis, is reported
    inside = O.voxelize(v["inside"], vs, 0)
    m = ops.build_map(ops.voxelize(_t(v["inside"], dev), vs, 0), want_first=True)
    ops.finalize_maps([m])
    want_rows, want_first, status = O.build_map(inside)
    assert status == 0 and _eq(m.coords, want_rows) and _eq(m.first, want_first)
    for row in v["outside"]:
        m = ops.build_map(ops.voxelize(_t(np.concatenate([v["inside"], row[None]]), dev), vs, 0))
        with pytest.raises(AprHipError):
            ops.finalize_maps([m])


# ------------------------------------------------------------------------------------------------- map build
@pytest.mark.parametrize("name", CLEAN)
def test_map_build_row_patterns(dev, name):
    d = MAP_CASES[name]
    m, want_rows = _check_build(d, dev)
    ops.finalize_maps([m])                                        # garbage past n_live does not raise
    assert m.n == len(want_rows) and _eq(m.coords, want_rows)


@pytest.mark.parametrize("name", RAISING)
def test_map_build_reports_an_out_of_range_live_row(dev, name):
    m, _ = _check_build(MAP_CASES[name], dev)                     # the in-range rows still form the oracle's map
    with pytest.raises(AprHipError):
        ops.finalize_maps([m])


def test_map_build_scan_takes_a_second_trip(dev):
    _check_build(HC.scan_two_trips(), dev)


def test_map_build_of_no_rows(dev):
    m = ops.build_map(torch.zeros((0, 4), dtype=torch.int32, device=dev), want_first=True)
    assert int(m.n_dev.item()) == 0 and int(m.status.item()) == 0
    assert bool((m.keys == HC.EMPTY).all())


# ------------------------------------------------------------------------------------------------- probe wrap
def test_probe_chain_wraps_from_the_last_slot_to_slot_0(dev):
    d = HC.probe_wrap()
    rows = d["rows"]
    m = _map(rows, dev)
    assert m.cap == d["cap"] == 1024
    occupied = m.keys.cpu().numpy() != HC.EMPTY
    assert int(occupied.sum()) == len(rows)
    assert bool(occupied[1020:].all()) and bool(occupied[:36].all())      # one unbroken chain through slot 1023 into slot 0
    for ks in (3, 5, 7):
        want = O.kernel_map(rows, rows, ks, 1)
        assert _eq(_generic(m, m, ks, 1), want), ks
        assert _eq(_same(m, ks, 1), want), ks
    coarse, _, _ = O.build_map(rows, floor_to=2)
    cm = _map(coarse, dev)
    assert _eq(_generic(cm, m, 3, 1), O.kernel_map(coarse, rows, 3, 1))


# ------------------------------------------------------------------------------------------------- kernel maps
@pytest.mark.parametrize("name", [n for n, c in KMAP_CASES.items() if c["kind"] == "same"])
def test_same_level_kernel_maps(dev, name):
    c = KMAP_CASES[name]
    m = _map(c["rows"], dev)
    want = O.kernel_map(c["rows"], c["rows"], c["ks"], c["scale"])
    assert _eq(_generic(m, m, c["ks"], c["scale"]), want)
    assert _eq(_same(m, c["ks"], c["scale"]), want)
    assert _eq(ops.kernel_map(m, m, c["ks"], c["scale"]), want)
    assert _eq(ops.kernel_map(m, copy.copy(m), c["ks"], c["scale"]), want)


def _two_levels(c, dev):
    fine = _map(c["rows"], dev)
    coarse_rows, _, status = O.build_map(c["rows"], floor_to=2 * c["scale"])
    coarse = ops.build_map(fine.coords, floor_to=2 * c["scale"])
    ops.finalize_maps([coarse])
    assert status == 0 and _eq(coarse.coords, coarse_rows)
    return fine, coarse, coarse_rows


@pytest.mark.parametrize("name", [n for n, c in KMAP_CASES.items() if c["kind"] == "strided"])
def test_strided_kernel_maps(dev, name):
    c = KMAP_CASES[name]
    fine, coarse, coarse_rows = _two_levels(c, dev)
    want = O.kernel_map(coarse_rows, c["rows"], c["ks"], c["scale"])
    assert _eq(_generic(coarse, fine, c["ks"], c["scale"]), want)
    assert _eq(ops.kernel_map(coarse, fine, c["ks"], c["scale"]), want)


@pytest.mark.parametrize("name", [n for n, c in KMAP_CASES.items() if c["kind"] == "transposed"])
def test_transposed_kernel_maps(dev, name):
    c = KMAP_CASES[name]
    fine, coarse, coarse_rows = _two_levels(c, dev)
    want = O.kernel_map(c["rows"], coarse_rows, c["ks"], -c["scale"])
    fwd = O.kernel_map(coarse_rows, c["rows"], c["ks"], c["scale"])
    assert np.array_equal(want, O.transpose_map(fwd, len(c["rows"])))
    assert _eq(_generic(fine, coarse, c["ks"], -c["scale"]), want)      # the negative-scale probe
    forward = _generic(coarse, fine, c["ks"], c["scale"])
    assert _eq(forward, fwd)                                            # checked on the host before the scatter reads it
    assert _eq(ops.kernel_map_transpose(forward, fine.n), want)


@pytest.mark.parametrize("name", ["strided_1_to_2", "transposed_2_to_1", "strided_faces", "transposed_faces", "two_batches"])
def test_coordinate_manager_transposed_maps(dev, name):
    rows = KMAP_CASES[name]["rows"]
    lv = {1: rows}
    for ts in (2, 4):
        lv[ts] = O.build_map(lv[ts // 2], floor_to=ts)[0]
    cm = CoordinateManager(_t(rows, dev))
    cm.build_pyramid([2, 4])
    for ts in (1, 2, 4):
        assert _eq(cm.get_map(ts).coords, lv[ts])
    # the forward tables first: the transpose scatters through their entries, so a wrong one must fail here, on the host
    assert _eq(cm.kernel_map(1, 2, 3), O.kernel_map(lv[2], lv[1], 3, 1))
    assert _eq(cm.kernel_map(2, 4, 3), O.kernel_map(lv[4], lv[2], 3, 2))
    assert _eq(cm.kernel_map(1, 1, 5), O.kernel_map(lv[1], lv[1], 5, 1))
    # 2:1 strides: the transpose of the forward table; 4:1: the negative-scale probe into the coarse table
    assert _eq(cm.kernel_map(2, 1, 3, True), O.transpose_map(O.kernel_map(lv[2], lv[1], 3, 1), len(rows)))
    assert _eq(cm.kernel_map(4, 2, 3, True), O.transpose_map(O.kernel_map(lv[4], lv[2], 3, 2), len(lv[2])))
    assert _eq(cm.kernel_map(4, 1, 3, True), O.kernel_map(lv[1], lv[4], 3, -1))


@pytest.mark.parametrize("name,live", [("k3_n257", 128), ("k3_n257", 0), ("k7_n255", 254), ("range_faces_k5", 7)])
def test_kernel_map_device_row_count(dev, name, live):
    c = KMAP_CASES[name]
    m = _map(c["rows"], dev)
    nbr = torch.full((m.n, c["ks"] ** 3), SENTINEL, dtype=torch.int32, device=dev)
    _generic(m, m, c["ks"], c["scale"], n_out_dev=_n_dev(live, dev), nbr=nbr)
    want = O.kernel_map(c["rows"], c["rows"], c["ks"], c["scale"])
    want[live:] = SENTINEL                                        # rows past the device count are not written
    assert _eq(nbr, want)


@pytest.mark.parametrize("name", [n for n, c in KMAP_CASES.items() if c.get("occ")])
def test_kernel_map_through_the_occupancy_bitmap(dev, name):
    c = KMAP_CASES[name]
    rows, ks = c["rows"], c["ks"]
    fine = _map(rows, dev)
    bbox = ops.coords_bbox(fine.coords).tolist()
    assert bbox == O.bbox(rows) and ops.occ_conv_supported(bbox, ks, 8)
    keep = []
    ops.occ_conv(fine.coords, fine.n, bbox, ks, torch.ones((ks ** 3, 8), dtype=torch.float32, device=dev), keep=keep)
    assert keep[0][3] == fine.n and keep[0][4] == fine.coords.data_ptr()      # kernel_map_occ takes the bitmap path
    assert _eq(ops.kernel_map_occ(fine, fine, ks, 1, keep[0]), O.kernel_map(rows, rows, ks, 1))
    coarse_rows, _, _ = O.build_map(rows, floor_to=2)
    coarse = _map(coarse_rows, dev)
    assert _eq(ops.kernel_map_occ(coarse, fine, 3, 1, keep[0]), O.kernel_map(coarse_rows, rows, 3, 1))


def test_kernel_maps_of_zero_rows(dev):
    empty = ops.build_map(torch.zeros((0, 4), dtype=torch.int32, device=dev))
    ops.finalize_maps([empty])
    rows = KMAP_CASES["k3_n257"]["rows"]
    m = _map(rows, dev)
    assert empty.n == 0 and tuple(_generic(empty, m, 3, 1).shape) == (0, 27) and tuple(ops.kernel_map(empty, empty, 5, 1).shape) == (0, 125)
    assert _eq(_generic(m, empty, 3, 1), O.kernel_map(rows, np.zeros((0, 4), np.int32), 3, 1))      # every probe misses an empty table


def test_generic_kernel_past_its_grid_cap(dev):
    c = HC.big_generic()
    m = _map(c["rows"], dev)
    assert m.n * 343 > 65536 * 256
    assert _eq(_generic(m, m, 7, 1), O.kernel_map(c["rows"], c["rows"], 7, 1))


def test_symmetric_kernel_and_its_fill_past_their_grid_caps(dev):
    c = HC.big_sym()
    m = _map(c["rows"], dev)
    assert m.n * 172 > 65536 * 256 and m.n * 171 > 16384 * 256
    assert _eq(_same(m, 7, 1), O.kernel_map(c["rows"], c["rows"], 7, 1))


# ------------------------------------------------------------------------------------------------- transpose
@pytest.mark.parametrize("name", list(HC.transpose_cases()))
def test_map_transpose_both_entry_points(dev, name):
    d = HC.transpose_cases()[name]
    nbr, n_in = _t(d["nbr"], dev), d["n_in"]
    want = O.transpose_map(d["nbr"], n_in)
    assert _eq(ops.kernel_map_transpose(nbr, n_in), want)
    table = ops.fill_bytes(torch.empty((n_in, nbr.shape[1]), dtype=torch.int32, device=dev), 0xFF)
    assert _eq(ops.kernel_map_transpose(nbr, n_in, prefilled=table), want)


# ------------------------------------------------------------------------------------------------- pyramids
# (CoordinateManager.kernel_map arguments, the oracle's table over the levels lv); the forward (4, 8) table comes before its
# transpose, which scatters through it
PYRAMID_MAPS = (((1, 1, 3, False), lambda lv: O.kernel_map(lv[1], lv[1], 3, 1)),
                ((1, 2, 3, False), lambda lv: O.kernel_map(lv[2], lv[1], 3, 1)),
                ((4, 8, 3, False), lambda lv: O.kernel_map(lv[8], lv[4], 3, 4)),
                ((8, 4, 3, True), lambda lv: O.transpose_map(O.kernel_map(lv[8], lv[4], 3, 4), len(lv[4]))))


def _check_pyramid(cm, counts, bbox, pts, first, p):
    for ts in (1, 2, 4, 8):
        assert cm.size(ts) == len(p["rows"][ts]) and _eq(cm.get_map(ts).coords, p["rows"][ts]), ts
    assert [int(v) for v in counts] == p["counts"].tolist()
    assert [int(v) for v in bbox] == p["bbox"]
    assert _eq(first, p["first"])
    assert _eq(pts, p["pts"])
    for key, want in PYRAMID_MAPS:
        assert _eq(cm.kernel_map(*key), want(p["rows"])), key


def _tensor_front_end(clouds, vs):
    """Tensor by tensor: apr_voxelize_frames, apr_map_build x 4 (x 5 with the compact table), apr_segment_counts,
    apr_coords_bbox, apr_gather_frame_points."""
    coords, offs_dev, offs = ops.voxelize_frames(clouds, vs)
    m = ops.build_map(coords, want_first=True)
    pts = ops.gather_frame_points(clouds, m)
    counts, bbox = ops.segment_counts(m, offs_dev), ops.coords_bbox(coords)
    cm = CoordinateManager(base_map=m)
    counts, bbox = cm.build_pyramid([2, 4, 8], extras=(counts, bbox))
    return cm, counts, bbox, pts[:len(m.first)], m.first, offs


def _one_call_front_end(clouds, vs):
    vp = ops.VoxelPyramid(clouds, vs)
    maps, counts, bbox, pts, first, counters = vp.finish()
    return CoordinateManager.from_maps(maps, counters), counts, bbox, pts, first, vp


@pytest.mark.parametrize("name", list(HC.frame_cases()))
def test_build_pyramid_equals_the_oracle(dev, name):
    d = HC.frame_cases()[name]
    p = O.pyramid(d["clouds"], d["vs"])
    cm, counts, bbox, pts, first, offs = _tensor_front_end([_t(x, dev) for x in d["clouds"]], d["vs"])
    assert offs == p["offsets"]
    _check_pyramid(cm, counts, bbox, pts, first, p)


@pytest.mark.parametrize("name", list(HC.frame_cases()))
def test_voxel_pyramid_equals_the_oracle(dev, name):
    d = HC.frame_cases()[name]
    p = O.pyramid(d["clouds"], d["vs"])
    cm, counts, bbox, pts, first, vp = _one_call_front_end([_t(x, dev) for x in d["clouds"]], d["vs"])
    assert vp.offsets == p["offsets"] and vp.py.compact == 0
    _check_pyramid(cm, counts, bbox, pts, first, p)


def test_compact_table_holds_exactly_its_rows(dev):
    """R distinct voxels in a table of R rows: the compact table is used, by both front ends."""
    d = HC.compact_case(False)
    p = O.pyramid(d["clouds"], d["vs"])
    assert len(p["rows"][1]) == d["R"]
    clouds = [_t(x, dev) for x in d["clouds"]]
    cm, counts, bbox, pts, first, vp = _one_call_front_end(clouds, d["vs"])
    assert vp.py.compact == 1 and vp.py.compact_rows == d["R"]
    _check_pyramid(cm, counts, bbox, pts, first, p)
    cm, counts, bbox, pts, first, _ = _tensor_front_end(clouds, d["vs"])
    assert cm._dedup is not None and cm._compact_rows == d["R"] and cm.get_map(1).cap == 2 * d["R"]
    _check_pyramid(cm, counts, bbox, pts, first, p)


def test_compact_table_one_row_short_is_a_fallback(dev):
    """R + 1 distinct voxels: apr_voxel_pyramid reports it (finish() is None), CoordinateManager rebuilds over the big table;
    never a truncated pyramid."""
    d = HC.compact_case(True)
    p = O.pyramid(d["clouds"], d["vs"])
    assert len(p["rows"][1]) == d["R"] + 1
    clouds = [_t(x, dev) for x in d["clouds"]]
    vp = ops.VoxelPyramid(clouds, d["vs"])
    assert vp.py.compact == 1 and vp.py.compact_rows == d["R"]
    assert vp.finish() is None
    cm, counts, bbox, pts, first, _ = _tensor_front_end(clouds, d["vs"])
    assert cm._dedup is None
    _check_pyramid(cm, counts, bbox, pts, first, p)


# ------------------------------------------------------------------------------------------------- fills and packs
def _filled(buf, lo, hi, inside, outside):
    h = buf.cpu().numpy()
    return bool((h[:lo] == outside).all()) and bool((h[lo:hi] == inside).all()) and bool((h[hi:] == outside).all())


def test_fill_bytes_every_phase_and_short_length(dev):
    G = HC.FILL_GUARD
    base = torch.empty(2 * G + 16 + max(HC.FILL_LENGTHS), dtype=torch.uint8, device=dev)
    assert base.data_ptr() % 16 == 0
    for phase in HC.FILL_PHASES:
        for n in HC.FILL_LENGTHS:
            base.fill_(0xA5)
            # the library call itself: an empty torch slice has no address, and a length of 0 must still touch nothing
            ops.check(ops._lib_().apr_fill_bytes(C.c_void_p(base.data_ptr() + G + phase), 0x3C, n, ops.stream()))
            assert _filled(base, G + phase, G + phase + n, 0x3C, 0xA5), (phase, n)


@pytest.mark.parametrize("n,phase", [(HC.FILL_LONG[0], 3), (HC.FILL_LONG[1], 9)])
def test_fill_bytes_past_its_grid(dev, n, phase):
    G = HC.FILL_GUARD
    base = torch.full((2 * G + 16 + n,), 0xA5, dtype=torch.uint8, device=dev)
    t = base[G + phase:G + phase + n]
    assert t.data_ptr() % 16 == phase
    ops.fill_bytes(t, 0xFF)
    assert bool((t == 0xFF).all()) and bool((base[:G + phase] == 0xA5).all()) and bool((base[G + phase + n:] == 0xA5).all())


def test_pack_i32_past_its_grid(dev):
    G = HC.FILL_GUARD
    rng = np.random.default_rng(3)
    parts = [_t(rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32), dev)
             for n in (3, HC.PACK_LONG_SOURCE, 0, HC.PACK_GRID_WORDS, 1, HC.PACK_GRID_WORDS + 1)]
    zbuf = torch.full((2 * G + HC.PACK_LONG_ZERO,), 7, dtype=torch.int32, device=dev)
    zero = zbuf[G:G + HC.PACK_LONG_ZERO]
    packed = ops.pack_i32(parts, zero=zero)
    assert torch.equal(packed, torch.cat(parts))
    assert bool((zero == 0).all()) and bool((zbuf[:G] == 7).all()) and bool((zbuf[G + HC.PACK_LONG_ZERO:] == 7).all())
    # no sources, only a block to clear
    zbuf.fill_(7)
    assert ops.pack_i32([], zero=zero).numel() == 0
    assert bool((zero == 0).all()) and bool((zbuf[:G] == 7).all()) and bool((zbuf[G + HC.PACK_LONG_ZERO:] == 7).all())
