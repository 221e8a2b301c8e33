"""APG aggregation and the ground-truth pairs row by row (csrc/apg.hip: k_transform, k_max_sqnorm, k_crop_flags,
k_scan_counts, k_compact_points, k_nn3_min, k_sum_bits; csrc/points.hip: k_radius through apg.get_matching_indices) against
tests/apg_oracle.py, on the inputs of tests/apg_cases.py.

The crop is checked without an escape clause: every output row is matched to its input row by its 12 bytes; the source
indices must rise strictly; float64 decides every row outside an 8u band, and the kept mask equals the float32 statement
((x*x + y*y) + z*z) < max(same over the key) on every row, band included.  The pairs are compared with np.array_equal, order
included, on the GPU's own transformed source.  Each test prints its figures (`-s` shows them) before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

from apr_amd import _lib
from apr_amd.fcgf.lib import apg
from tests import apg_cases as CASES
from tests import apg_oracle as O
from tests import icp_oracle

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------ transform
@pytest.mark.parametrize("pose_as", ["numpy64", "device32"])
@pytest.mark.parametrize("name", CASES.POSES)
@pytest.mark.parametrize("n", CASES.TRANSFORM_SIZES)
def test_transform_within_the_dot_product_bound(dev, n, name, pose_as):
    pts = CASES.transform_points(n, name)
    T = CASES.pose(name)
    arg = T if pose_as == "numpy64" else torch.from_numpy(T.astype(np.float32)).to(dev)
    got = apg.apply_transform(pts, arg)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 3)
    got = got.cpu().numpy()
    ref, bound = O.transform64(pts, T)
    if name == "identity":
        assert np.array_equal(got.view(np.uint32), pts.view(np.uint32))
        return
    frac = np.abs(got.astype(np.float64) - ref) / bound
    print(f"APGFIG transform n={n} pose={name}/{pose_as}: worst error {frac.max():.3f} of its bound")
    assert (frac <= 1.0).all(), (int(np.argmax(frac.max(1))), float(frac.max()))


# ----------------------------------------------------------------------------------------------------------- crop
def _crop_checked(dev, key, pts, planted, label):
    d_key, d_pts = torch.from_numpy(key).to(dev), torch.from_numpy(pts).to(dev)
    out = apg.crop_to_radius(d_key, d_pts)
    assert out.dtype == torch.float32 and out.dim() == 2 and out.shape[1] == 3
    again = apg.crop_to_radius(d_key, d_pts)
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.cpu().numpy().view(np.uint32)), "a second call gives other bits"
    # the float64 statement first (it must hold whatever the kernels' rounding), then the float32 one
    src, n_band = O.check_crop(key, pts, got, max_band=O.band_limit(len(pts)), planted=planted)
    at_limit = CASES.at_limit(key, pts, planted)
    kept_at_limit = int(np.isin(at_limit, src).sum())
    print(f"APGFIG crop {label}: n={len(pts)} n_key={len(key)} kept={len(got)} band={n_band} planted={len(planted)} "
          f"at_limit={len(at_limit)} at_limit_kept={kept_at_limit}")
    O.check_crop(key, pts, got, planted=planted, exact=True)   # the planted rows tell a fused norm from the rounded one
    assert kept_at_limit == 0                                  # rows AT the limit: the strict < drops them
    return src


@pytest.mark.parametrize("pattern,n", CASES.crop_case_list())
def test_crop_rows_order_and_mask(dev, pattern, n):
    key, pts, planted = CASES.crop_case(pattern, n)
    src = _crop_checked(dev, key, pts, planted, pattern)
    if pattern == "all":
        assert len(src) == n
    elif pattern == "none":
        assert len(src) == 0
    elif pattern == "blocks":
        assert np.array_equal(src, np.flatnonzero((np.arange(n) // CASES.KBLOCK) % 2 == 0))
    elif pattern == "one_first":
        assert src.tolist() == [0]
    elif pattern == "one_last":
        assert src.tolist() == [n - 1]


@pytest.mark.parametrize("n_key,far_at", CASES.KEY_CASES)
def test_crop_key_maximum_over_every_key_row(dev, n_key, far_at):
    key, pts, planted = CASES.key_case(n_key, far_at)
    src = _crop_checked(dev, key, pts, planted, f"key[{far_at}]")
    if n_key > 1:                                              # a maximum that missed the farthest row would keep < 5 %
        assert 0.5 * len(pts) < len(src) < len(pts)


def test_crop_of_no_points_is_empty(dev):
    key, _, _ = CASES.crop_case("blocks", 1)
    out = apg.crop_to_radius(key, np.zeros((0, 3), np.float32))
    assert tuple(out.shape) == (0, 3) and out.dtype == torch.float32 and out.is_cuda


@pytest.mark.parametrize("n", [257, CASES.N_ONE_TRIP + 1])
def test_crop_writes_only_its_rows_and_its_scratch(dev, n):
    lib = _lib.load()
    key, pts, planted = CASES.crop_case("gauss", n)
    d_key, d_pts = torch.from_numpy(key).to(dev), torch.from_numpy(pts).to(dev)
    canary_f = float(np.frombuffer(np.uint32(0x4B1D4B1D).tobytes(), np.float32)[0])
    out = torch.full((n + 64, 3), canary_f, dtype=torch.float32, device=dev)       # 64 rows past the largest output
    sb = int(lib.apr_crop_scratch_bytes(n))
    lead = 512
    buf = torch.full((lead + sb + 512,), 0xA5, dtype=torch.uint8, device=dev)
    cnt = torch.full((3,), -77, dtype=torch.int32, device=dev)
    _lib.check(lib.apr_crop_to_radius(_lib.ptr(d_key), len(key), _lib.ptr(d_pts), n, _lib.ptr(out),
                                      C.c_void_p(cnt.data_ptr() + 4), C.c_void_p(buf.data_ptr() + lead), sb, _lib.stream()))
    torch.cuda.synchronize()
    cnt = cnt.cpu().numpy()
    m = int(cnt[1])
    assert cnt[0] == -77 and cnt[2] == -77 and 0 < m < n
    host = out.cpu().numpy()
    src, _ = O.check_crop(key, pts, host[:m], max_band=O.band_limit(n), planted=planted, exact=True)
    assert len(src) == m
    assert (host[m:].view(np.uint32) == 0x4B1D4B1D).all(), "rows past the count were written"
    b = buf.cpu().numpy()
    assert (b[:lead] == 0xA5).all() and (b[lead + sb:] == 0xA5).all(), "bytes outside the scratch were written"
    cnt2 = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.AprHipError):                      # one byte short: refused before anything is launched
        _lib.check(lib.apr_crop_to_radius(_lib.ptr(d_key), len(key), _lib.ptr(d_pts), n, _lib.ptr(out), _lib.ptr(cnt2),
                                          C.c_void_p(buf.data_ptr() + lead), sb - 1, _lib.stream()))


# ------------------------------------------------------------------------------------------------------ GT pairs
@pytest.mark.parametrize("name", CASES.PAIR_CASES)
def test_matching_indices_equal_the_float32_statement(dev, name):
    src, tgt, T, r = CASES.pair_case(name)
    moved = apg.apply_transform(src, T).cpu().numpy()          # pinned: the search is judged on the GPU's own moved source
    ref = O.radius_pairs_f32(moved, tgt, r)
    per_query = np.bincount(ref[:, 0], minlength=len(src))
    assert per_query.max() < 1024                              # under k_radius' rank buffer
    got = apg.get_matching_indices(src, tgt, T, r)
    assert got.dtype == torch.int64 and got.dim() == 2 and got.shape[1] == 2
    got = got.cpu().numpy()
    print(f"APGFIG pairs {name}: n_src={len(src)} n_tgt={len(tgt)} pairs={len(ref)} most per query={per_query.max()}")
    assert np.array_equal(got, ref)
    got1 = apg.get_matching_indices(src, tgt, T, r, K=1)
    assert got1.dtype == torch.int64 and got1.dim() == 2 and got1.shape[1] == 2
    assert np.array_equal(got1.cpu().numpy(), O.first_pair_per_source(ref))
    if name == "no_pairs":
        assert tuple(got.shape) == (0, 2)
    elif name == "planted":
        E = len(tgt)
        assert got[got[:, 0] == 0][:, 1].tolist() == [E - 1, 104, 105, E - 3, E - 2, 1, 3]
    elif name == "far_queries":
        assert len(ref) > 0 and not np.isin(got[:, 0], np.arange(30, len(src) - 30)).any()


# ---------------------------------------------------------------------------------------------------------- chain
def test_aggregate_frames_is_transform_crop_first_rows(dev):
    key, frames, poses, vs = CASES.chain_case()
    nghb, sel = apg.aggregate_frames(key, frames, poses, vs)
    moved = torch.cat([apg.apply_transform(f, M) for f, M in zip(frames, poses)], 0)
    want = apg.crop_to_radius(key, moved)
    got = nghb.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.cpu().numpy().view(np.uint32))
    moved_h = moved.cpu().numpy()
    for f, M, lo in zip(frames, poses, np.cumsum([0] + [len(f) for f in frames])):
        ref, bound = O.transform64(f, M)
        assert (np.abs(moved_h[lo:lo + len(f)].astype(np.float64) - ref) <= bound).all()
    src, n_band = O.check_crop(key, moved_h, got, max_band=O.band_limit(len(moved_h)), exact=True)
    print(f"APGFIG chain: n={len(moved_h)} kept={len(got)} band={n_band}")
    assert 0.35 * len(moved_h) < len(got) < 0.65 * len(moved_h)
    assert sel.dtype == torch.int64
    assert np.array_equal(np.sort(sel.cpu().numpy()), icp_oracle.voxel_first_rows(got, vs))


# -------------------------------------------------------------------------------------------------------- chamfer
@pytest.mark.parametrize("m", CASES.CHAMFER_M)
@pytest.mark.parametrize("n", CASES.CHAMFER_N)
def test_chamfer_sum_matches_float64(dev, n, m):
    a, b = CASES.chamfer_case(n, m)
    got = apg.chamfer_sum(a, b)
    assert got.dtype == torch.float64 and got.dim() == 0
    ref = O.chamfer_sum64(a, b)
    print(f"APGFIG chamfer n={n} m={m}: relative error {abs(float(got) - ref) / ref:.2e}")
    assert abs(float(got) - ref) <= 1e-6 * ref
