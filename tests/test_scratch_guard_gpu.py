"""Every entry point that carves a caller-owned scratch stays inside the bytes its *_scratch_bytes function asked for.

The scratch lies inside a larger allocation of the test's own, [1 MiB][scratch_bytes][1 MiB], filled with 0xA5: once with
its base on a multiple of 256, once 16 bytes further.  After the call both bands are untouched and the outputs equal, bit
for bit, those of a third call on an aligned scratch of twice the size.  A layout that disagrees with its size shows up
here as a failed assertion inside memory the test owns."""
import ctypes as C

import numpy as np
import pytest
import torch

from apr_amd import _lib

pytestmark = pytest.mark.gpu
BAND = 1 << 20
SIZES = [(1, 1), (64, 1), (64, 3), (65, 1), (65, 3), (257, 1), (257, 3)]      # (rows, clouds)


def _host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _guarded(dev, sb, call):
    """call(scratch address, scratch bytes) -> outputs (tensors / arrays / numbers), run three times as described above"""
    assert sb > 0
    runs = []
    for shift in (0, 16):
        buf = torch.full((2 * BAND + sb + 256,), 0xA5, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 256 == 0
        lo = BAND + shift
        out = call(buf.data_ptr() + lo, sb)
        torch.cuda.synchronize()
        assert bool((buf[:lo] == 0xA5).all()), f"bytes below the scratch were written (base + {shift})"
        assert bool((buf[lo + sb:] == 0xA5).all()), f"bytes above the scratch were written (base + {shift})"
        runs.append([_host(o) for o in out])
    ref_buf = torch.full((2 * sb,), 0xA5, dtype=torch.uint8, device=dev)
    ref = call(ref_buf.data_ptr(), 2 * sb)
    torch.cuda.synchronize()
    ref = [_host(o) for o in ref]
    for shift, got in zip((0, 16), runs):
        assert len(got) == len(ref)
        for k, (a, b) in enumerate(zip(got, ref)):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (shift, k)
    return ref


def _cloud(n, seed, scale=1.0):
    return (np.random.default_rng(seed).random((n, 3), dtype=np.float32) * np.float32(scale)).astype(np.float32)


def _lengths(n, nb):
    base = n // nb
    return np.array([base] * (nb - 1) + [n - base * (nb - 1)], np.int32)


def _moved(xyz, seed):
    """xyz under a small rigid motion, float32"""
    a = 0.1 + 0.01 * seed
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float64)
    return (xyz.astype(np.float64) @ R.T + np.array([0.05, -0.02, 0.03])).astype(np.float32)


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_map_build(dev, n):
    lib = _lib.load()
    coords = torch.from_numpy(np.random.default_rng(n).integers(0, 4, (n, 4)).astype(np.int32)).to(dev)
    coords[:, 0] = 0
    cap = int(lib.apr_hash_capacity(n))

    def call(scratch, sb):
        keys = torch.zeros(cap, dtype=torch.int64, device=dev)
        vals = torch.zeros(cap, dtype=torch.int32, device=dev)
        oc = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        first = torch.zeros(n, dtype=torch.int64, device=dev)
        hdr = torch.zeros(2, dtype=torch.int32, device=dev)
        _lib.check(lib.apr_map_build(_lib.ptr(coords), n, None, 0, _lib.ptr(keys), _lib.ptr(vals), cap, _lib.ptr(oc),
                                     _lib.ptr(first), _lib.ptr(hdr), C.c_void_p(hdr.data_ptr() + 4), C.c_void_p(scratch), sb,
                                     _lib.stream()))
        # a key's slot depends on which thread claimed it first: the table is compared as the set of its (key, row) entries
        k, v = keys.cpu().numpy(), vals.cpu().numpy()
        live = k != -1
        order = np.argsort(k[live], kind="stable")
        return [k[live][order], v[live][order], oc, first, hdr]

    ref = _guarded(dev, int(lib.apr_map_scratch_bytes(n)), call)
    assert 0 < ref[4][0] <= n and ref[4][1] == 0 and len(ref[0]) == ref[4][0]


@pytest.mark.parametrize("n,nb", SIZES)
def test_grid_subsample(dev, n, nb):
    lib = _lib.load()
    pts, la = torch.from_numpy(_cloud(n, n + nb)).to(dev), _lengths(n, nb)

    def call(scratch, sb):
        out = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        lens = np.zeros(nb, np.int32)
        _lib.check(lib.apr_grid_subsample(_lib.ptr(pts), n, _hp(la), nb, 0.25, None, 0, _lib.ptr(out), None, _hp(lens),
                                          C.c_void_p(scratch), sb, _lib.stream()))
        return [out, lens]

    ref = _guarded(dev, int(lib.apr_grid_subsample_scratch_bytes(n)), call)
    assert (ref[1] > 0).all() and ref[1].sum() <= n


@pytest.mark.parametrize("n,nb", SIZES)
def test_radius_neighbors_both_forms_and_async(dev, n, nb):
    lib = _lib.load()
    s, q = torch.from_numpy(_cloud(n, 3 * n + nb)).to(dev), torch.from_numpy(_cloud(n, 5 * n + nb)).to(dev)
    la, radius, limit = _lengths(n, nb), 0.3, 24

    def sync_forms(scratch, sb):
        width = C.c_int32(-1)
        _lib.check(lib.apr_radius_neighbors(_lib.ptr(q), n, _lib.ptr(s), n, _hp(la), _hp(la), nb, radius, 0, None, 0,
                                            C.byref(width), C.c_void_p(scratch), sb, _lib.stream()))
        w = max(int(width.value), 1)
        out = torch.zeros((n, w), dtype=torch.int32, device=dev)
        width2 = C.c_int32(-1)
        _lib.check(lib.apr_radius_neighbors(_lib.ptr(q), n, _lib.ptr(s), n, _hp(la), _hp(la), nb, radius, 0, _lib.ptr(out), w,
                                            C.byref(width2), C.c_void_p(scratch), sb, _lib.stream()))
        return [out, np.array([width.value, width2.value])]

    def async_form(scratch, sb):
        out = torch.zeros((n, limit), dtype=torch.int32, device=dev)
        flags = torch.zeros(2, dtype=torch.int32, device=dev)
        _lib.check(lib.apr_radius_neighbors_async(_lib.ptr(q), n, _lib.ptr(s), n, _hp(la), _hp(la), nb, radius, limit,
                                                  _lib.ptr(out), limit, _lib.ptr(flags), C.c_void_p(scratch), sb, _lib.stream()))
        return [out, flags]

    sb = int(lib.apr_radius_scratch_bytes(n, n))
    ref = _guarded(dev, sb, sync_forms)
    assert ref[1][0] == ref[1][1] >= 0
    ref = _guarded(dev, sb, async_form)
    assert ref[1][1] == 0


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_crop_to_radius(dev, n):
    lib = _lib.load()
    key, pts = torch.from_numpy(_cloud(32, 7, 0.6)).to(dev), torch.from_numpy(_cloud(n, 11 * n)).to(dev)

    def call(scratch, sb):
        out = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.apr_crop_to_radius(_lib.ptr(key), 32, _lib.ptr(pts), n, _lib.ptr(out), _lib.ptr(cnt), C.c_void_p(scratch),
                                          sb, _lib.stream()))
        return [out, cnt]

    _guarded(dev, int(lib.apr_crop_scratch_bytes(n)), call)


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_nn3(dev, n):
    lib = _lib.load()
    a, b = torch.from_numpy(_cloud(n, 13 * n)).to(dev), torch.from_numpy(_cloud(n, 17 * n)).to(dev)

    def call(scratch, sb):
        packed = torch.zeros(n, dtype=torch.int64, device=dev)
        total = torch.zeros(1, dtype=torch.float64, device=dev)
        _lib.check(lib.apr_nn3(_lib.ptr(a), n, _lib.ptr(b), n, 0.2, _lib.ptr(packed), _lib.ptr(total), C.c_void_p(scratch), sb,
                               _lib.stream()))
        return [packed, total]

    ref = _guarded(dev, int(lib.apr_nn3_scratch_bytes(n, n)), call)
    assert ((ref[0] & 0xFFFFFFFF) < n).all()


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_reverse_table_build(dev, n):
    lib = _lib.load()
    H = 5
    nbr = torch.from_numpy(np.random.default_rng(n).integers(0, n + 1, (n, H)).astype(np.int32)).to(dev)    # n = padding

    def call(scratch, sb):
        rev = torch.zeros(n * H, dtype=torch.int32, device=dev)
        start = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        _lib.check(lib.apr_reverse_table_build(_lib.ptr(nbr), n, H, n, _lib.ptr(rev), _lib.ptr(start), C.c_void_p(scratch), sb,
                                               _lib.stream()))
        return [rev, start]

    ref = _guarded(dev, int(lib.apr_reverse_table_scratch_bytes(n, H, n)), call)
    assert ref[1][0] == 0 and ref[1][-1] == int((nbr.cpu().numpy() < n).sum())


@pytest.mark.parametrize("n,nb", SIZES)
def test_voxel_down_sample(dev, n, nb):
    lib = _lib.load()
    pts, la = torch.from_numpy(_cloud(n, 19 * n + nb)).to(dev), _lengths(n, nb)

    def call(scratch, sb):
        out = [torch.zeros((n, 3), dtype=torch.float64, device=dev), torch.zeros((n, 3), dtype=torch.float32, device=dev),
               torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
               torch.zeros((n, 3), dtype=torch.int32, device=dev)]
        lens = np.zeros(nb, np.int32)
        _lib.check(lib.apr_voxel_down_sample(_lib.ptr(pts), n, _hp(la), nb, 0.2, *[_lib.ptr(o) for o in out], _hp(lens),
                                             C.c_void_p(scratch), sb, _lib.stream()))
        return out + [lens]

    ref = _guarded(dev, int(lib.apr_voxel_down_sample_scratch_bytes(n)), call)
    assert (ref[5] > 0).all() and ref[2][:ref[5].sum()].sum() == n


def _ransac_inputs(dev, n0, seed):
    xyz0 = _cloud(n0, seed, 10.0)
    xyz1 = _moved(xyz0, seed)
    corr = np.arange(n0, dtype=np.int64)
    corr[::7] = (corr[::7] * 3 + 1) % n0                 # some wrong matches
    return torch.from_numpy(xyz0).to(dev), torch.from_numpy(xyz1).to(dev), torch.from_numpy(corr).to(dev)


def _ransac_pose(dev, n0, max_iter):
    lib = _lib.load()
    x0, x1, corr = _ransac_inputs(dev, n0, n0)

    def call(scratch, sb):
        res = (C.c_double * 20)()
        _lib.check(lib.apr_ransac_pose(_lib.ptr(x0), n0, _lib.ptr(x1), n0, _lib.ptr(corr), 0.3, 0.9, max_iter, 5,
                                       C.c_void_p(scratch), sb, res, _lib.stream()))
        return [np.array(list(res))]

    return _guarded(dev, int(lib.apr_ransac_scratch_bytes(n0, max_iter)), call)[0]


@pytest.mark.parametrize("n0", [4, 65, 300])
def test_ransac_pose(dev, n0):
    res = _ransac_pose(dev, n0, 1000)
    assert res[15] == 1.0 and res[19] >= 0


def test_ransac_pose_chunked_rounds_repack(dev):
    """force_rounds = 1 and more than 2^20 iterations: two rounds, the second behind a re-pack of the records"""
    lib = _lib.load()
    _lib.check(lib.apr_ransac_set_option(3, 1))
    try:
        res = _ransac_pose(dev, 300, (1 << 20) + 1000)
    finally:
        _lib.check(lib.apr_ransac_set_option(3, -1))
    assert res[16] > 150 and res[19] > 0


@pytest.mark.parametrize("n0", [4, 65, 300])
def test_ransac_pose_geometric(dev, n0):
    lib = _lib.load()
    x0, x1, corr = _ransac_inputs(dev, n0, n0 + 1)

    def call(scratch, sb):
        res = (C.c_double * 20)()
        _lib.check(lib.apr_ransac_pose_geometric(_lib.ptr(x0), n0, _lib.ptr(x1), n0, _lib.ptr(corr), 0.3, 0.9, 1000, 100, 5,
                                                 C.c_void_p(scratch), sb, res, _lib.stream()))
        return [np.array(list(res))]

    ref = _guarded(dev, int(lib.apr_ransac_geometric_scratch_bytes(n0, n0, 1000)), call)
    assert ref[0][15] == 1.0


@pytest.mark.parametrize("n_pairs", [4, 65])
def test_ransac_pose_pairs_geometric(dev, n_pairs):
    lib = _lib.load()
    n0 = 300
    x0, x1, _ = _ransac_inputs(dev, n0, 2)
    rows = np.random.default_rng(n_pairs).integers(0, n0, n_pairs).astype(np.int32)
    pairs = torch.from_numpy(np.stack([rows, rows], 1).copy()).to(dev)

    def call(scratch, sb):
        res = (C.c_double * 20)()
        _lib.check(lib.apr_ransac_pose_pairs_geometric(_lib.ptr(x0), n0, _lib.ptr(x1), n0, _lib.ptr(pairs), n_pairs, 0.3, 1000,
                                                       100, 5, C.c_void_p(scratch), sb, res, _lib.stream()))
        return [np.array(list(res))]

    ref = _guarded(dev, int(lib.apr_ransac_pairs_geometric_scratch_bytes(n0, n0, n_pairs, 1000, 100)), call)
    assert ref[0][15] == 1.0


@pytest.mark.parametrize("lanes", [1, 3])
def test_match_pose_batch(dev, lanes):
    lib = _lib.load()
    B, c, max_iter = 3, 32, 10000
    keep, descs = [], (_lib.PairDesc * B)()
    for i, (n0, n1) in enumerate([(300, 310), (297, 290), (305, 300)]):
        rng = np.random.default_rng(100 + i)
        p0 = _cloud(n0, 200 + i, 10.0)
        f0 = rng.standard_normal((n0, c)).astype(np.float32)
        sel = rng.integers(0, n0, n1)
        p1, f1 = _moved(p0[sel], i), (f0[sel] + 0.05 * rng.standard_normal((n1, c))).astype(np.float32)
        t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (f0, f1, p0, p1)]
        keep += t
        d = descs[i]
        d.f0, d.n0, d.f1, d.n1 = t[0].data_ptr(), n0, t[1].data_ptr(), n1
        d.xyz0, d.xyz1, d.seed = t[2].data_ptr(), t[3].data_ptr(), i

    def call(scratch, sb):
        res = (C.c_double * (20 * B))()
        _lib.check(lib.apr_match_pose_batch(descs, B, c, 0.3, 0.9, max_iter, C.c_void_p(scratch), sb, res, _lib.stream()))
        return [np.array(list(res)).reshape(B, 20)]

    _lib.check(lib.apr_match_pose_set_lanes(lanes))
    try:
        ref = _guarded(dev, int(lib.apr_match_pose_batch_scratch_bytes(B, 305, 310, c, max_iter)), call)
    finally:
        _lib.check(lib.apr_match_pose_set_lanes(1))
    assert (ref[0][:, 15] == 1.0).all()


def _icp_inputs(dev):
    n = 257
    tgt = _cloud(n, 31, 4.0)
    return n, torch.from_numpy(_moved(tgt, 0)).to(dev), torch.from_numpy(tgt).to(dev), np.array([0, n], np.int64)


def test_icp_batch(dev):
    lib = _lib.load()
    n, src, tgt, off = _icp_inputs(dev)
    init = torch.eye(4, dtype=torch.float64, device=dev).reshape(1, 16).contiguous()

    def call(scratch, sb):
        rec = torch.zeros((1, 20), dtype=torch.float64, device=dev)
        corr = torch.zeros(n, dtype=torch.int32, device=dev)
        _lib.check(lib.apr_icp_batch(_lib.ptr(src), _hp(off), _lib.ptr(tgt), _hp(off), 1, None, 1, _lib.ptr(init), 1.0, 30, 1e-6,
                                     1e-6, _lib.ptr(rec), _lib.ptr(corr), C.c_void_p(scratch), sb, _lib.stream()))
        return [rec, corr]

    ref = _guarded(dev, int(lib.apr_icp_scratch_bytes(n, n, 1)), call)
    assert ref[0][0, 18] > 0


def test_information_batch(dev):
    lib = _lib.load()
    n, src, tgt, off = _icp_inputs(dev)
    T = torch.eye(4, dtype=torch.float64, device=dev).reshape(1, 16).contiguous()

    def call(scratch, sb):
        info = torch.zeros((1, 36), dtype=torch.float64, device=dev)
        sums = torch.zeros((1, 10), dtype=torch.float64, device=dev)
        corr = torch.zeros(n, dtype=torch.int32, device=dev)
        _lib.check(lib.apr_information_batch(_lib.ptr(src), _hp(off), _lib.ptr(tgt), _hp(off), 1, None, 1, _lib.ptr(T), 16, 1.0,
                                             _lib.ptr(info), _lib.ptr(sums), _lib.ptr(corr), C.c_void_p(scratch), sb,
                                             _lib.stream()))
        return [info, sums, corr]

    ref = _guarded(dev, int(lib.apr_information_scratch_bytes(n, n, 1)), call)
    assert ref[1][0, 0] > 0
