"""The float64 oracle of the FCGF losses (tests/fcgf_losses_oracle.py) held to the reference's own text: the fp64 leg of
tests/golden/fcgf_losses_ref.npz (tests/golden/make_fcgf_losses_ref_golden.py executes the reference's functions).

Values at 1e-12 relative; draws, masks, mined rows and the position of the NumPy stream exactly; gradients at 1e-9 rel-L2
(the fixture stores them to 2^-35).  No GPU.
"""
import numpy as np
import pytest

from tests import fcgf_losses_oracle as O

Z = O.load_fixture()
SEED = 77


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.all(np.abs(a - b) <= tol * np.abs(b)), (a, b)


def _grad_close(g, z, key, tol=1e-9):
    want = O.fixture_grad(z, key, len(g))
    assert np.linalg.norm(g - want) <= tol * np.linalg.norm(want)
    untouched = np.setdiff1d(np.arange(len(g)), z[key + "_rows"])
    assert not g[untouched].any()


def _inputs(tag):
    return Z[f"{tag}_F0"], Z[f"{tag}_F1"], Z[f"{tag}_pairs"], [int(v) for v in Z[f"{tag}_args"]]


@pytest.mark.parametrize("tag", O.CASES)
def test_generate_rand_negative_pairs(tag):
    F0, F1, pairs, _ = _inputs(tag)
    np.random.seed(SEED)
    neg = O.generate_rand_negative_pairs(pairs, max(len(F0), len(F1)), len(F0), len(F1))
    assert neg.dtype == np.int64 and np.array_equal(neg, Z[f"{tag}_con_neg_pairs"])
    assert np.random.rand() == float(Z[f"{tag}_con_next"])


@pytest.mark.parametrize("tag", O.CASES)
def test_contrastive(tag):
    F0, F1, pairs, _ = _inputs(tag)
    r = O.contrastive(F0, F1, pairs, Z[f"{tag}_con_neg_pairs"])
    _close([r["pos"], r["neg"]], Z[f"{tag}_con_values"])
    _grad_close(r["gF0_pos"] + r["gF0_neg"], Z, f"{tag}_con_gF0")
    _grad_close(r["gF1_pos"] + r["gF1_neg"], Z, f"{tag}_con_gF1")


@pytest.mark.parametrize("tag", O.CASES)
def test_triplet(tag):
    F0, F1, pairs, (num_pos, _, num_rand) = _inputs(tag)
    np.random.seed(SEED)
    draws = O.draw_triplet(len(F0), len(F1), len(pairs), num_pos, num_rand)
    assert np.random.rand() == float(Z[f"{tag}_tri_next"])
    for got, want in zip(draws, O.fixture_draws(Z, tag, "tri")):
        assert np.array_equal(got, want)
    r = O.triplet(F0, F1, pairs, draws)
    _close([r["loss"], r["pos_dist"], r["neg_dist"]], Z[f"{tag}_tri_values"])
    assert np.array_equal(r["rand_mask"], Z[f"{tag}_tri_rand_mask"])
    _grad_close(r["gF0"], Z, f"{tag}_tri_gF0")
    _grad_close(r["gF1"], Z, f"{tag}_tri_gF1")


@pytest.mark.parametrize("tag", O.CASES)
def test_hardest_triplet(tag):
    F0, F1, pairs, (num_pos, num_hn, num_rand) = _inputs(tag)
    np.random.seed(SEED)
    draws = O.draw_hardest(len(F0), len(F1), len(pairs), num_pos, num_hn, num_rand)
    assert np.random.rand() == float(Z[f"{tag}_hard_next"])
    for got, want in zip(draws, O.fixture_draws(Z, tag, "hard")):
        assert np.array_equal(got, want)
    r = O.hardest_triplet(F0, F1, pairs, draws)
    _close([r["loss"], r["pos_dist"], r["neg_dist"]], Z[f"{tag}_hard_values"])
    for k in ("mask0", "mask1", "rand_mask", "D01ind", "D10ind"):
        assert np.array_equal(r[k], Z[f"{tag}_hard_{k}"]), k
    _grad_close(r["gF0"], Z, f"{tag}_hard_gF0")
    _grad_close(r["gF1"], Z, f"{tag}_hard_gF1")
    # the planted tie went to the lower index of the sub-sample
    row, lo, hi = (int(v) for v in Z[f"{tag}_tie"])
    assert r["D01"][row, lo] == r["D01"][row, hi] == r["D01"][row].min() and r["D01ind"][row] == draws[1][lo]


def test_pinned_mined_rows_are_used():
    F0, F1, pairs, _ = _inputs("c128")
    draws = O.fixture_draws(Z, "c128", "hard")
    base = O.hardest_triplet(F0, F1, pairs, draws)
    other = base["D01ind"].copy()
    other[0] = draws[1][(list(draws[1]).index(other[0]) + 1) % len(draws[1])]
    r = O.hardest_triplet(F0, F1, pairs, draws, mined=(other, base["D10ind"]))
    assert r["D01ind"][0] == other[0] and r["loss"] != base["loss"]


def test_unequal_triplet_lengths_raise():
    """min(len(pairs), num_rand_triplet) != min(N1, num_rand_triplet): the reference's _hash fails to broadcast (:569)."""
    F0, F1, pairs, _ = _inputs("c128")
    np.random.seed(SEED)
    draws = O.draw_triplet(len(F0), len(F1), len(pairs), 24, 33)      # 30 pairs, N1 = 36: 30 != 33
    assert len(draws[1]) == 30 and len(draws[2]) == 33
    with pytest.raises(ValueError, match="broadcast"):
        O.triplet(F0, F1, pairs, draws)
    with pytest.raises(ValueError, match="broadcast"):
        O.hardest_triplet(F0, F1, pairs, (np.arange(4), np.arange(4)) + draws)
