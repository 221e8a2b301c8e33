"""The hashing oracle (tests/hash_oracle.py) and the planted inputs (tests/hash_cases.py) on the host: every case holds the
fact it claims, the oracle equals a brute-force dict implementation on every small case and oracle/me_oracle.py on a synthetic
frame, and me_oracle's kernel map no longer aliases across the range edge."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hash_cases as HC  # noqa: E402
import hash_oracle as O  # noqa: E402
from apr_amd import synth  # noqa: E402
from oracle import me_oracle as OME  # noqa: E402

F32 = np.float32
LO, HI = O.AXIS_LO, O.AXIS_HI


# ------------------------------------------------------------------------------------------------- brute force
def _floor_to(v, m):
    return v if m <= 0 else (v // m) * m          # Python's // floors


def brute_build(rows, floor_to=0, n_live=None):
    seen, out, first, status = {}, [], [], 0
    n = len(rows) if n_live is None else min(n_live, len(rows))
    for i in range(n):
        b, x, y, z = (int(v) for v in rows[i])
        r = (b, _floor_to(x, floor_to), _floor_to(y, floor_to), _floor_to(z, floor_to))
        if not (0 <= r[0] < 1023 and all(LO <= v < HI for v in r[1:])):
            status = 1
            continue
        if r not in seen:
            seen[r] = len(out)
            out.append(r)
            first.append(i)
    return np.array(out, np.int32).reshape(-1, 4), np.array(first, np.int64), status


def brute_kernel_map(out_rows, in_rows, ks, scale):
    table = {tuple(int(v) for v in r): i for i, r in enumerate(in_rows)}
    h = ks // 2
    nbr = np.full((len(out_rows), ks ** 3), -1, np.int32)
    for j, r in enumerate(out_rows):
        b, x, y, z = (int(v) for v in r)
        o = 0
        for oz in range(-h, h + 1):
            for oy in range(-h, h + 1):
                for ox in range(-h, h + 1):
                    q = (x + ox * scale, y + oy * scale, z + oz * scale)
                    if all(LO <= v < HI for v in q) and 0 <= b < 1023:
                        nbr[j, o] = table.get((b,) + q, -1)
                    o += 1
    return nbr


def _levels(c):
    """(out rows, in rows, signed scale) of a kernel-map case."""
    fine = c["rows"]
    if c["kind"] == "same":
        return fine, fine, c["scale"]
    coarse, _, st = O.build_map(fine, floor_to=2 * c["scale"])
    assert st == 0
    return (coarse, fine, c["scale"]) if c["kind"] == "strided" else (fine, coarse, -c["scale"])


# ------------------------------------------------------------------------------------------------- voxelisation values
@pytest.mark.parametrize("vs", HC.VOXEL_SIZES)
def test_voxel_values_hold_their_facts(vs):
    v = HC.voxel_values(vs)
    tiny = np.finfo(F32).tiny
    q = v["denormal"] / F32(vs)
    assert bool(((q < 0) & (np.abs(q) < tiny)).all()) and bool((np.floor(q) == -1).all())
    pin, pout, nin, nout = v["edges"]
    fl = lambda x: float(np.floor(F32(x) / F32(vs)))      # noqa: E731
    assert fl(pin) == HI - 1 and fl(pout) == HI and np.nextafter(pin, F32(np.inf)) == pout
    assert fl(nin) == LO and fl(nout) == LO - 1 and np.nextafter(nin, F32(-np.inf)) == nout
    rows = O.voxelize(v["inside"], vs, 0)
    assert bool(O.in_range(rows).all())
    col = v["inside"][:, 0]
    assert any(np.signbit(x) and x == 0 for x in col) and any(not np.signbit(x) and x == 0 for x in col)
    assert pin in col and nin in col
    out = O.voxelize(v["outside"], vs, 0)
    assert not bool(O.in_range(out).any()) and len(out) == 6
    assert sorted(set(out[:, 1:][(out[:, 1:] >= HI) | (out[:, 1:] < LO)].tolist())) == [LO - 1, HI]
    # the planted multiples straddle voxel faces: a float32 step changes the voxel
    x = col[:, None]
    step = np.floor(np.nextafter(x, F32(np.inf)) / F32(vs)) != np.floor(np.nextafter(x, F32(-np.inf)) / F32(vs))
    assert int(step.sum()) >= 20
    # -0.0 voxelises to 0 and the negative denormal to -1
    assert O.voxelize(np.array([[-0.0, 0.0, -1e-45]], F32), vs, 3).tolist() == [[3, 0, 0, -1]]


# ------------------------------------------------------------------------------------------------- map-build patterns
def _run_ok(rows, start, length):
    run = rows[start:start + length]
    return bool((run == run[0]).all()) and (start == 0 or not (rows[start - 1] == run[0]).all()) and \
        (start + length == len(rows) or not (rows[start + length] == run[0]).all())


def test_map_cases_hold_their_facts():
    c = HC.map_cases()
    for n in (1, 63, 64, 65, 255, 256, 257):
        assert len(c[f"rows_{n}"]["rows"]) == n
    assert len(O.build_map(c["rows_257"]["rows"])[0]) < 257
    s, l = c["run_cross_wave"]["run"]
    assert _run_ok(c["run_cross_wave"]["rows"], s, l) and s // 64 != (s + l - 1) // 64 and s // 256 == (s + l - 1) // 256
    s, l = c["run_cross_block"]["run"]
    assert _run_ok(c["run_cross_block"]["rows"], s, l) and s // 256 != (s + l - 1) // 256
    s, l = c["run_longer_than_wave"]["run"]
    assert _run_ok(c["run_longer_than_wave"]["rows"], s, l) and l > 2 * 64 and (s + l - 1) // 64 - s // 64 == 2
    d = c["run_oor_middle"]
    s, l = d["run"]
    rows = d["rows"]
    assert s // 64 == (s + l - 1) // 64 and s < d["oor"] < s + l - 1
    assert bool((np.delete(rows[s:s + l], d["oor"] - s, 0) == rows[s]).all())
    assert O.in_range(rows).sum() == len(rows) - 1 and not O.in_range(rows[d["oor"]])[0]
    d = c["aba_one_wave"]
    r = d["rows"]
    assert (r[5] == r[7]).all() and not (r[5] == r[6]).all() and (r[20] == r[21]).all() and (r[22] == r[23]).all() \
        and (r[24] == r[20]).all() and not (r[21] == r[22]).all()
    assert len(O.build_map(c["all_equal"]["rows"])[0]) == 1 and len(O.build_map(c["all_distinct"]["rows"])[0]) == 300
    cr = c["range_corners"]["rows"]
    u = O.build_map(cr)
    assert len(u[0]) == 16 and u[2] == 0 and set(cr[:, 0].tolist()) == {0, 1022} and set(cr[:, 1:].ravel().tolist()) == {LO, HI - 1}
    for ax in "xzb":
        d = c[f"oor_{ax}"]
        ok = O.in_range(d["rows"])
        assert ok.sum() == len(ok) - 1 and not ok[d["oor"]] and O.build_map(d["rows"])[2] == 1
    assert c["oor_x"]["rows"][37].tolist() == [0, HI, 0, 0] and c["oor_z"]["rows"][37].tolist() == [0, 0, 0, LO - 1] \
        and c["oor_b"]["rows"][37].tolist() == [1023, 0, 0, 0]
    for f in (2, 4, 8):
        d = c[f"floor_to_{f}"]
        assert d["floor_to"] == f and {-1, -2, -7, -8, -9, LO + 1} <= set(d["rows"][:, 1].tolist())
        got, _, st = O.build_map(d["rows"], floor_to=f)
        assert st == 0 and bool((got[:, 1:] % f == 0).all()) and got[:, 1:].min() == LO
        # towards minus infinity: -1 -> -f, never 0
        assert O.build_map(np.array([[0, -1, -9, LO + 1]], np.int32), floor_to=f)[0].tolist() == [[0, -f, {2: -10, 4: -12, 8: -16}[f], LO]]
    d = c["live_cuts_run"]
    s, l = d["run"]
    assert s < d["n_live"] < s + l and O.build_map(d["rows"], n_live=d["n_live"])[2] == 0 and O.build_map(d["rows"])[2] == 1
    d = c["live_block_edge"]
    assert d["n_live"] % 256 == 0 and 0 < d["n_live"] < len(d["rows"])
    for name in ("live_cuts_run", "live_block_edge", "live_zero"):
        d = c[name]
        tail = d["rows"][d["n_live"]:]
        assert not O.in_range(tail[0::2]).any() and O.in_range(tail[1::2]).all()
        live = {tuple(r) for r in d["rows"][:d["n_live"]].tolist()}
        assert d["n_live"] == 0 or all(tuple(r) in live for r in tail[1::2].tolist())
    assert c["live_zero"]["n_live"] == 0 and len(O.build_map(c["live_zero"]["rows"], n_live=0)[0]) == 0


def test_scan_case_needs_a_second_trip_and_its_carry():
    d = HC.scan_two_trips()
    n = len(d["rows"])
    assert n == 262145 and -(-n // 256) == 1025
    rows, first, st = O.build_map(d["rows"])
    assert st == 0 and first[-1] == n - 1 and 2.5 < n / len(rows) < 3.5
    runs = 1 + int((np.abs(np.diff(d["rows"], axis=0)).sum(1) != 0).sum())
    assert len(rows) < 0.8 * runs          # voxels come back after their run: the table, not the run compression, merges them


@pytest.mark.parametrize("name", list(HC.map_cases()))
def test_build_map_equals_brute_force(name):
    d = HC.map_cases()[name]
    got, want = O.build_map(d["rows"], d["floor_to"], d["n_live"]), brute_build(d["rows"], d["floor_to"], d["n_live"])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64


# ------------------------------------------------------------------------------------------------- probe wrap
def test_probe_wrap_case_wraps():
    d = HC.probe_wrap()
    rows, cap = d["rows"], d["cap"]
    assert len(rows) <= 512 and cap == 1024 and len(np.unique(rows, axis=0)) == len(rows)
    homes = np.array([HC.home(r, cap) for r in rows])
    assert int((homes >= cap - 4).sum()) >= 40 and len(d["absent"]) == 12
    present = {tuple(r) for r in rows.tolist()}
    for a in d["absent"].tolist():
        assert tuple(a) not in present and HC.home(a, cap) >= cap - 4 and (a[0], a[1] + 1, a[2], a[3]) in present
    occ = HC.simulate_table(rows, cap)
    assert bool(occ[cap - 4:].all()) and bool(occ[:36].all())
    # the misses walk across the wrap: the oracle says -1 at offset (-1, 0, 0) of every partner row
    nbr = O.kernel_map(rows, rows, 3, 1)
    assert np.array_equal(nbr, brute_kernel_map(rows, rows, 3, 1))
    idx = {tuple(r): i for i, r in enumerate(rows.tolist())}
    assert all(nbr[idx[(a[0], a[1] + 1, a[2], a[3])], 12] == -1 for a in d["absent"].tolist())
    assert O.kernel_offsets(3)[12] == (-1, 0, 0)


# ------------------------------------------------------------------------------------------------- kernel maps
@pytest.mark.parametrize("name", list(HC.kernel_map_cases()))
def test_kernel_map_equals_brute_force(name):
    c = HC.kernel_map_cases()[name]
    rows = c["rows"]
    assert len(np.unique(rows, axis=0)) == len(rows) and bool(O.in_range(rows).all()) and bool((rows[:, 1:] % c["scale"] == 0).all())
    out_rows, in_rows, scale = _levels(c)
    got = O.kernel_map(out_rows, in_rows, c["ks"], scale)
    assert got.dtype == np.int32 and np.array_equal(got, brute_kernel_map(out_rows, in_rows, c["ks"], scale))
    if c["kind"] == "same":
        assert np.array_equal(got[:, c["ks"] ** 3 // 2], np.arange(len(rows)))


def test_kernel_map_cases_hold_their_facts():
    c = HC.kernel_map_cases()
    for ks, n, mult in ((3, 256, True), (3, 257, False), (5, 256, True), (5, 255, False), (7, 256, True), (7, 255, False)):
        d = c[f"k{ks}_n{n}"]
        assert len(d["rows"]) == n and ((n * ks ** 3) % 256 == 0) == mult and d["ks"] == ks
        hits = (O.kernel_map(d["rows"], d["rows"], 3, 1) >= 0).mean()
        assert 0.25 < hits < 0.6
    assert {c[k]["scale"] for k in c} == {1, 2, 4, 8} and {c[k]["ks"] for k in c} == {3, 5, 7}
    d = c["two_batches"]["rows"]
    a, b = ({tuple(r[1:]) for r in d[d[:, 0] == v].tolist()} for v in (0, 1))
    assert len(a - b) > 50 and len(b - a) > 50 and len(a & b) > 50
    # probes that leave the range, and the two pairs a packed probe would alias
    for name in ("range_faces_k3", "range_faces_k5", "range_faces_k7", "coarse_faces_k3", "coarse_faces_k7"):
        d = c[name]
        offs = np.array(O.kernel_offsets(d["ks"])) * d["scale"]
        q = d["rows"][:, None, 1:].astype(np.int64) + offs[None]
        assert int(((q < LO) | (q >= HI)).any(2).sum()) > 100 * (d["ks"] // 2)
    rows = c["range_faces_k3"]["rows"].tolist()
    nbr = O.kernel_map(c["range_faces_k3"]["rows"], c["range_faces_k3"]["rows"], 3, 1)
    z0, z1, b0, b1 = (rows.index(list(r)) for r in HC.ALIAS_Z + HC.ALIAS_B)
    assert z1 not in nbr[z0] and z0 not in nbr[z1] and b1 not in nbr[b0] and b0 not in nbr[b1]
    d = c["coarse_faces_k7"]
    assert d["scale"] * (d["ks"] // 2) == 24 and d["rows"][:, 1:].max() == HI - 8


def test_big_cases_are_the_smallest_past_the_grid_caps():
    g, s = HC.big_generic(), HC.big_sym()
    ng, ns = len(g["rows"]), len(s["rows"])
    assert ng * 343 > 65536 * 256 >= (ng - 1) * 343 and ng == 48914
    assert ns * 172 > 65536 * 256 >= (ns - 1) * 172 and ns == 97542 and -(-ns * 171 // 256) > HC.FILL_UPPER_BLOCKS
    for d, vol in ((g, 46 * 46 * 47), (s, 58 ** 3)):
        rows = d["rows"]
        assert len(np.unique(rows, axis=0)) == len(rows) and 0.45 < len(rows) / vol < 0.55 and d["ks"] == 7
        assert 0.4 < (O.kernel_map(rows, rows, 3, 1) >= 0).mean() < 0.55


# ------------------------------------------------------------------------------------------------- transpose, frames
def test_transpose_cases():
    c = HC.transpose_cases()
    for name, d in c.items():
        nbr = d["nbr"]
        t = O.transpose_map(nbr, d["n_in"])
        assert t.shape == (d["n_in"], nbr.shape[1]) and int((t >= 0).sum()) == int((nbr >= 0).sum())
        j, k = np.nonzero(t >= 0)
        assert bool((nbr[t[j, k], k] == j).all())
    for name in ("subset_1", "subset_2"):
        t = O.transpose_map(c[name]["nbr"], c[name]["n_in"])
        assert int((t.max(1) < 0).sum()) > 20          # fine rows without a coarse partner
    assert bool((O.transpose_map(c["zero_rows"]["nbr"], 5) == -1).all())


def test_frame_cases_hold_their_facts():
    c = HC.frame_cases()
    sizes = lambda d: [len(x) for x in d["clouds"]]      # noqa: E731
    assert all(o % 256 == 0 for o in O.pyramid(c["block_edges"]["clouds"], 0.3)["offsets"])
    assert sizes(c["empty_first"])[0] == 0 and sizes(c["empty_last"])[-1] == 0 and sizes(c["empty_middle"])[1:3] == [0, 0]
    assert len(c["max_frames"]["clouds"]) == HC.MAX_FRAMES == 64
    for name in ("inside_run", "empty_middle"):
        cl = [x for x in c[name]["clouds"] if len(x)]
        for a, b in zip(cl, cl[1:]):
            va, vb = O.voxelize(a[-2:], 0.3, 0), O.voxelize(b[:2], 0.3, 0)
            assert np.array_equal(va, vb) and (va[0] == va[1]).all()
    for d in c.values():
        p = O.pyramid(d["clouds"], d["vs"])
        assert p["status"] == 0 and int(p["counts"].sum()) == len(p["rows"][1]) and len(p["rows"][8]) <= len(p["rows"][4])
        assert [int(v) for v in p["counts"]] == [len(O.build_map(O.voxelize(x, 0.3, 0))[0]) for x in d["clouds"]]


@pytest.mark.parametrize("extra", [False, True])
def test_compact_cases_sit_on_the_boundary(extra):
    d = HC.compact_case(extra)
    n = sum(len(x) for x in d["clouds"])
    assert n == 262145 and HC.compact_rows(n) == 65536 == d["R"] and HC.compact_rows(n - 1) == 0
    rows = O.build_map(np.concatenate([O.voxelize(x, d["vs"], b) for b, x in enumerate(d["clouds"])]))[0]
    assert len(rows) == d["R"] + int(extra) == d["voxels"]


def test_fill_and_pack_cases():
    short = [(p, n) for p in HC.FILL_PHASES for n in HC.FILL_LENGTHS if HC.fill_head(p) > n > 0]
    assert len(short) > 20 and HC.fill_head(0) == 0 and HC.fill_head(1) == 15
    assert HC.FILL_LONG[0] > 2048 * 256 * 16 and HC.FILL_LONG[1] // 16 > 2048 * 256 * 8
    assert HC.PACK_LONG_SOURCE > 64 * 256 and HC.PACK_LONG_ZERO > 64 * 256


# ------------------------------------------------------------------------------------------------- the two oracles
def test_hash_oracle_equals_me_oracle_on_a_synthetic_frame():
    xyz = synth.make_small_frame(4)
    oc, osel = OME.sparse_quantize(xyz / F32(0.3), return_index=True)
    rows, first, st = O.build_map(O.voxelize(xyz, 0.3, 0))
    assert st == 0 and np.array_equal(rows[:, 1:], oc) and np.array_equal(first, osel)
    ocm = OME.CoordinateManager(OME.batched_coordinates([oc]))
    lv = {1: rows}
    for ts in (2, 4, 8):
        lv[ts] = O.build_map(lv[ts // 2], floor_to=ts)[0]
        assert np.array_equal(lv[ts], ocm.get_coords(ts))
    for ti, to, k in ((1, 1, 3), (1, 1, 5), (1, 2, 3), (2, 2, 3), (4, 8, 3)):
        assert np.array_equal(O.kernel_map(lv[to], lv[ti], k, ti), ocm.get_map(ti, to, k)), (ti, to, k)
    ref = OME.transpose_map(ocm.get_map(1, 2, 3), len(lv[1]))
    assert np.array_equal(O.transpose_map(O.kernel_map(lv[2], lv[1], 3, 1), len(lv[1])), ref)
    assert np.array_equal(O.kernel_map(lv[1], lv[2], 3, -1), ref)


def test_me_oracle_kernel_map_does_not_alias_across_the_range_edge():
    """Packed, (0, 5, 7, 2^17 - 1) + z carries into y and lands on (0, 5, 8, -2^17); (0, 2^17 - 1, 3, 3) + x carries into the
    batch field and lands on (1, -2^17, 3, 3).  Neither is a neighbour."""
    for pair in (HC.ALIAS_Z, HC.ALIAS_B):
        rows = np.array(pair, np.int32)
        for ks in (3, 5):
            nbr = OME.kernel_map(rows, rows, ks, 1)
            want = np.full((2, ks ** 3), -1, np.int32)
            want[:, ks ** 3 // 2] = [0, 1]
            assert np.array_equal(nbr, want)
            assert np.array_equal(O.kernel_map(rows, rows, ks, 1), want)
