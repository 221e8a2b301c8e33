"""tests/apg_oracle.py has to be able to fail: every kind of wrong crop output is rejected, and its float32 statements agree
with float64 wherever float64 can decide -- on the very inputs tests/test_apg_gpu.py feeds the kernels."""
import numpy as np
import pytest

from tests import apg_cases as CASES
from tests import apg_oracle as O
from tests import icp_oracle


def _correct_crop(key, pts):
    return pts[O.crop_decision(key, pts)[3]]


@pytest.fixture(scope="module")
def crop_input():
    key, pts, planted = CASES.crop_case("gauss", 1537)
    good = _correct_crop(key, pts)
    must_keep, must_drop, band, keep = O.crop_decision(key, pts)
    assert 0.5 * len(pts) < len(good) < len(pts) - 8 and must_drop.sum() > 8
    return key, pts, planted, good


def test_correct_crop_passes(crop_input):
    key, pts, planted, good = crop_input
    src, n_band = O.check_crop(key, pts, good, max_band=O.band_limit(len(pts)), planted=planted, exact=True)
    assert np.array_equal(pts[src], good) and n_band <= O.band_limit(len(pts))


def _row(mask, which=0):
    return int(np.flatnonzero(mask)[which])


def test_dropped_must_keep_row_is_rejected(crop_input):
    key, pts, planted, good = crop_input
    must_keep, _, _, keep = O.crop_decision(key, pts)
    decided = np.flatnonzero(must_keep[np.flatnonzero(keep)])  # rows of `good` that float64 decides (all but planted ones)
    for at in decided[[0, len(decided) // 2, -1]]:
        with pytest.raises(AssertionError, match="missing"):
            O.check_crop(key, pts, np.delete(good, at, 0), planted=planted)


def test_extra_must_drop_row_is_rejected(crop_input):
    key, pts, planted, good = crop_input
    must_drop = O.crop_decision(key, pts)[1]
    i = _row(must_drop, 3)
    at = int(np.searchsorted(np.flatnonzero(O.crop_decision(key, pts)[3]), i))      # in order: only the decision is wrong
    with pytest.raises(AssertionError, match="outside the radius were kept"):
        O.check_crop(key, pts, np.insert(good, at, pts[i], 0), planted=planted)


def test_swapped_rows_are_rejected(crop_input):
    key, pts, planted, good = crop_input
    for a, b in ((0, 1), (255, 256), (len(good) - 2, len(good) - 1), (3, 700)):
        bad = good.copy()
        bad[[a, b]] = bad[[b, a]]
        with pytest.raises(AssertionError, match="not strictly increasing"):
            O.check_crop(key, pts, bad, planted=planted)


def test_duplicated_row_is_rejected(crop_input):
    key, pts, planted, good = crop_input
    with pytest.raises(AssertionError, match="not strictly increasing"):          # a repeat in place of its neighbour
        bad = good.copy()
        bad[11] = bad[10]
        O.check_crop(key, pts, bad, planted=planted)
    with pytest.raises(AssertionError, match="not strictly increasing"):          # a repeat appended
        O.check_crop(key, pts, np.concatenate([good, good[-1:]], 0), planted=planted)


@pytest.mark.parametrize("bit", [0, 7, 22])
def test_flipped_mantissa_bit_is_rejected(crop_input, bit):
    key, pts, planted, good = crop_input
    bad = good.copy()
    bad.view(np.uint32)[300, 1] ^= np.uint32(1 << bit)
    with pytest.raises(AssertionError, match="no bitwise copy"):
        O.match_rows(bad, pts)
    with pytest.raises(AssertionError, match="no bitwise copy"):
        O.check_crop(key, pts, bad, planted=planted)


def test_wrong_decision_in_the_band_is_rejected_by_the_exact_mask_only(crop_input):
    key, pts, planted, good = crop_input
    i = int(CASES.at_limit(key, pts, planted)[2])              # |p|^2 == limit in float32: the strict < drops it
    at = int(np.searchsorted(np.flatnonzero(O.crop_decision(key, pts)[3]), i))
    bad = np.insert(good, at, pts[i], 0)
    O.check_crop(key, pts, bad, planted=planted)               # float64 cannot tell
    with pytest.raises(AssertionError, match="float32 statement"):
        O.check_crop(key, pts, bad, planted=planted, exact=True)


def test_band_limit_is_enforced():
    key = np.array([[3.0, 4.0, 12.0]], np.float32)
    pts = CASES.mirror_images(key[0])                          # 8 rows AT the limit, none declared as planted ...
    pts = np.concatenate([pts, pts[:1] * np.float32(1 + 2.0 ** -22)], 0)      # ... and a ninth within the band
    with pytest.raises(AssertionError, match="undecided rows"):
        O.check_crop(key, pts, pts[:0], max_band=O.band_limit(len(pts)))
    O.check_crop(key, pts, pts[:0], max_band=O.band_limit(len(pts)), planted=range(8), exact=True)


def test_match_rows_refuses_ambiguous_input(crop_input):
    key, pts, planted, good = crop_input
    twice = pts.copy()
    twice[900] = twice[20]
    with pytest.raises(AssertionError, match="bit-equal"):
        O.match_rows(good, twice)
    assert O.match_rows(pts[:0], pts).shape == (0,) and O.match_rows(pts[:0], pts).dtype == np.int64


def _crop_inputs():
    for pattern, n in CASES.crop_case_list():
        yield f"{pattern}-{n}", CASES.crop_case(pattern, n)
    for n_key, far_at in CASES.KEY_CASES:
        yield f"key-{n_key}", CASES.key_case(n_key, far_at)


def test_keep_f32_agrees_with_float64_outside_the_band_on_every_gpu_input():
    seen = 0
    for name, (key, pts, planted) in _crop_inputs():
        must_keep, must_drop, band, keep_f32 = O.crop_decision(key, pts)
        assert keep_f32[must_keep].all() and not keep_f32[must_drop].any(), name
        assert band[planted].all(), name                                       # planted rows: float64 cannot decide them
        assert not keep_f32[CASES.at_limit(key, pts, planted)].any(), name      # AT the limit: dropped by the strict <
        free = band.copy()
        free[planted] = False
        assert free.sum() <= O.band_limit(len(pts)), (name, int(free.sum()))
        O.check_crop(key, pts, pts[keep_f32], max_band=O.band_limit(len(pts)), planted=planted, exact=True)
        seen += 1
    assert seen == len(CASES.crop_case_list()) + len(CASES.KEY_CASES)


def _fused_masks(key, pts):
    """The kept masks of builds that fuse the squared norm: both kernels alike (fma1 on both sides), and the two kernels
    differently (rows fma1, the limit fma2: k_max_sqnorm's unrolled loop body before sqnorm_rn was made uncontracted)."""
    f1 = O.sqnorm_contracted(pts, "fma1")
    return {"alike": f1 < O.sqnorm_contracted(key, "fma1").max(), "differently": f1 < O.sqnorm_contracted(key, "fma2").max()}


def test_fused_restatements_of_the_mask_fail_the_exact_check_on_every_planted_input():
    seen = 0
    for name, (key, pts, planted) in _crop_inputs():
        if not (name.startswith("gauss") or name.startswith("key")) or len(pts) < 63:
            continue
        far = key[np.argmax(O.sqnorm_f32(key))]
        rn, f1, f2 = (float(v[0]) for v in CASES._norms(far))
        assert f1 < f2 and rn != f1, (name, rn, f1, f2)                         # the farthest key point tells them apart
        if len(key) > 65536:                                                    # ... and sits in a two-trip thread
            assert (int(np.argmax(O.sqnorm_f32(key))) % 65536) + 65536 < len(key)
        for kind, mask in _fused_masks(key, pts).items():
            O.check_crop(key, pts, pts[mask], max_band=O.band_limit(len(pts)), planted=planted)      # float64 cannot tell
            with pytest.raises(AssertionError, match="float32 statement"):
                O.check_crop(key, pts, pts[mask], planted=planted, exact=True)
        # fused differently, the rows bit-equal to the farthest point and its mirror images are KEPT
        lim = CASES.at_limit(key, pts, planted)
        assert _fused_masks(key, pts)["differently"][lim].sum() >= min(8, len(lim)) - 3, name
        seen += 1
    assert seen == 8 + len(CASES.KEY_CASES)


def test_large_gaussian_case_keeps_about_85_percent():
    key, pts, planted = CASES.crop_case("gauss", CASES.N_THREE_TRIPS)
    frac = O.crop_decision(key, pts)[3].mean()
    assert 0.80 < frac < 0.90, frac
    blocks = -(-len(pts) // CASES.KBLOCK)
    assert blocks == 2050 and -(-blocks // CASES.SCAN) == 3


@pytest.mark.parametrize("name", CASES.PAIR_CASES)
def test_radius_pairs_f32_agrees_with_float64_on_every_decided_pair(name):
    src, tgt, T, r = CASES.pair_case(name)
    moved = icp_oracle.apply_transform(src, T)
    pairs = O.radius_pairs_f32(moved, tgt, r)
    assert pairs.dtype == np.int64 and pairs.shape[1:] == (2,)
    code = pairs[:, 0] * len(tgt) + pairs[:, 1]
    inside, undecided = O.radius_decided64(moved, tgt, r)
    assert len(np.unique(code)) == len(code)
    assert np.isin(inside, code).all()                                          # decided inside: listed
    assert np.isin(code, np.concatenate([inside, undecided])).all()             # listed: inside or undecided
    # the order: by i, then by (float32) distance, then by j
    m, t = moved[pairs[:, 0]], tgt[pairs[:, 1]]
    dx, dy, dz = m[:, 0] - t[:, 0], m[:, 1] - t[:, 1], m[:, 2] - t[:, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    key = np.stack([pairs[:, 0].astype(np.float64), d2.astype(np.float64), pairs[:, 1].astype(np.float64)], 1)
    assert all(tuple(a) < tuple(b) for a, b in zip(key[:-1], key[1:]))
    assert np.bincount(pairs[:, 0], minlength=1).max(initial=0) < 1024
    # no d2 within a rounding of r^2 or of a rival's d2: a build that fuses d2 into FMAs lists the same pairs in the same order
    for fused in ("fma1", "fma2"):
        assert np.array_equal(O.radius_pairs_f32(moved, tgt, r, fused=fused), pairs), fused


def test_planted_pairs_come_out_as_designed():
    src, tgt, T, r = CASES.pair_case("planted")
    pairs = O.radius_pairs_f32(src, tgt, r)
    E = len(tgt)
    assert pairs[pairs[:, 0] == 0][:, 1].tolist() == [E - 1, 104, 105, E - 3, E - 2, 1, 3]
    src, tgt, T, r = CASES.pair_case("far_queries")
    pairs = O.radius_pairs_f32(src, tgt, r)
    assert not np.isin(pairs[:, 0], np.arange(30, len(src) - 30)).any() and len(pairs) > 0
    src, tgt, T, r = CASES.pair_case("no_pairs")
    assert O.radius_pairs_f32(icp_oracle.apply_transform(src, T), tgt, r).shape == (0, 2)


def test_transform64_bound_holds_for_float32_evaluations():
    for name in CASES.POSES:
        pts = CASES.transform_points(4099, name)
        T = CASES.pose(name)
        ref, bound = O.transform64(pts, T)
        T32 = T.astype(np.float32)
        a = pts @ T32[:3, :3].T + T32[:3, 3]                                     # numpy's order
        x, y, z = pts[:, 0:1], pts[:, 1:2], pts[:, 2:3]
        R = T32[:3, :3].T[None]
        b = ((T32[:3, 3] + z * R[:, 2]) + y * R[:, 1]) + x * R[:, 0]             # another order, every step rounded
        for got in (a, b):
            frac = np.abs(got.astype(np.float64) - ref) / bound
            assert frac.max() < 1.0, (name, frac.max())
        wrong = b + np.float32(4e-4) * (np.abs(b) > 1)                            # ~1e-5 relative off: outside the bound
        assert (np.abs(wrong.astype(np.float64) - ref) > bound).any()


def test_chain_case_crops_about_half():
    key, frames, poses, vs = CASES.chain_case()
    cat = np.concatenate([icp_oracle.apply_transform(f, M) for f, M in zip(frames, poses)], 0)
    frac = O.crop_decision(key, cat)[3].mean()
    assert 0.35 < frac < 0.65, frac
