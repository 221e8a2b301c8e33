"""apr_kpconv_weighted_c32 (KPConv step 1 for cin = 32 on the fp32 MFMA: the first layer of the symmetric generator) element
by element against the float64 oracle tests/kpconv_oracle.py and its derived bound (ratio 1, no row excluded) on the cases
of tests/kpconv_c32_cases.py, which assert at import that they reach the edges: a query whose neighbours are all shadow, a
neighbour on a kernel point, a neighbour at distance float32(extent), support rows with zero and negative feature sums
inside a ball (listed, not counted: blocks.py:369-372).  The same inputs through apr_kpconv_weighted (its generic kernel),
the refusals, the wrapper's switch, and KPConvFunction end to end at cin = 32 with an input that takes no gradient -- the
bar of test_kpconv_function_end_to_end in test_kpconv_edges_gpu.py.

Measured on an MI355X (records, not thresholds): worst |kernel - oracle| / bound 0.253 on both entries; end to end out
4.2e-7, d W 4.5e-7.
"""
import numpy as np
import pytest
import torch

import kpconv_c32_cases as CC
import kpconv_cases as K
import kpconv_oracle as O
from apr_amd import _lib
from apr_amd.predator import kp_ops

pytestmark = pytest.mark.gpu
NAN = float("nan")
KK = 15 * CC.CIN


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _direct(dev, c, entry):
    """NaN-filled wf [nq, 480 + 32 guard columns] through `entry` -> (wf[:, :480], guard)"""
    lib = _lib.load()
    q, s, nbr, kp = _t(c["q"], dev), _t(c["s"], dev), _t(c["nbr"], dev), _t(c["kp"], dev)
    x = _t(c["x"], dev)
    rs = kp_ops.row_sums(x)
    ldwf = KK + 32
    wf = torch.full((c["nq"], ldwf), NAN, dtype=torch.float32, device=dev)
    _lib.check(getattr(lib, entry)(_lib.ptr(q), c["nq"], _lib.ptr(s), c["ns"], _lib.ptr(nbr), c["H"], _lib.ptr(x), CC.CIN, CC.CIN,
                                   _lib.ptr(kp), 15, c["extent"], _lib.ptr(rs), _lib.ptr(wf), ldwf, _lib.stream()))
    torch.cuda.synchronize()
    wf = wf.cpu().numpy()
    return wf[:, :KK], wf[:, KK:]


def _within(got, c, what):
    ref, _, _ = O.weighted(*CC.args(c))
    bound = O.bound_weighted(*CC.args(c))
    ratio, at = O.compare_rows(got, ref, bound)
    print(f"{what}: worst |kernel - oracle| / bound {ratio:.4f}")
    assert ratio <= 1.0, (what, ratio, at, None if at is None else (float(got[at]), float(ref[at]), float(bound[at])))


@pytest.mark.parametrize("entry", ["apr_kpconv_weighted_c32", "apr_kpconv_weighted"])
@pytest.mark.parametrize("name", list(CC.CASES))
def test_every_element_within_bound(dev, name, entry):
    """the new entry, and the generic kernel of apr_kpconv_weighted on the same inputs: every element inside the bound (a
    row no wave wrote is still NaN), the 32 guard columns still NaN"""
    c = CC.CASES[name]
    got, guard = _direct(dev, c, entry)
    assert np.isnan(guard).all(), "columns behind 15 * cin were written"
    _within(got, c, f"{name}/{entry}")


def test_all_shadow_query_is_exactly_zero(dev):
    name, qi = CC.FACTS["all_shadow"][0]
    got, _ = _direct(dev, CC.CASES[name], "apr_kpconv_weighted_c32")
    assert not got[qi].any() and not np.isnan(got[qi]).any()


@pytest.mark.parametrize("what", ["H129", "nkp14", "cin64", "x4off", "ldx33"])
def test_refusals(dev, what):
    """H = 129, 14 kernel points, cin = 64, and rows of x off the 8-byte grid: the argument error, nothing written"""
    lib = _lib.load()
    cin = 64 if what == "cin64" else 32
    H = 129 if what == "H129" else 5
    n_kp = 14 if what == "nkp14" else 15
    nq, ns = 5, 9
    rng = np.random.default_rng(7)
    q, s = _t(rng.uniform(-1, 1, (nq, 3)).astype(np.float32), dev), _t(rng.uniform(-1, 1, (ns, 3)).astype(np.float32), dev)
    kp = _t(rng.uniform(-1, 1, (15, 3)).astype(np.float32), dev)
    nbr = _t(rng.integers(0, ns + 1, (nq, H)).astype(np.int32), dev)
    big = _t(rng.standard_normal((ns, cin + 2)).astype(np.float32), dev)
    x, ldx = big[:, :cin], cin + 2
    if what == "x4off":
        x = big[:, 1:cin + 1]
    elif what == "ldx33":
        big = _t(rng.standard_normal((ns, cin + 1)).astype(np.float32), dev)
        x, ldx = big[:, :cin], cin + 1
    rs = kp_ops.row_sums(x)
    wf = torch.full((nq * 15 * cin * 4,), 0xA5, dtype=torch.uint8, device=dev)
    rc = lib.apr_kpconv_weighted_c32(_lib.ptr(q), nq, _lib.ptr(s), ns, _lib.ptr(nbr), H, _lib.ptr(x), ldx, cin, _lib.ptr(kp), n_kp,
                                     1.2, _lib.ptr(rs), _lib.ptr(wf), 15 * cin, _lib.stream())
    assert rc == -1 and lib.apr_last_error().decode()          # APR_EINVAL
    torch.cuda.synchronize()
    assert bool((wf == 0xA5).all()), "a refused call wrote to its output"


@pytest.mark.parametrize("name", list(CC.CASES))
def test_wrapper_with_the_switch_on_and_off(dev, name):
    """kp_ops.kpconv_weighted: [nq, 15 * cin rounded up to 32] (480: no padding column at this width, and none may appear),
    inside the bound on both routes"""
    c = CC.CASES[name]
    q, s, nbr, kp, x = (_t(c[k], dev) for k in ("q", "s", "nbr", "kp", "x"))
    saved = kp_ops.KPCONV_C32
    try:
        for on in (True, False):
            kp_ops.KPCONV_C32 = on
            wf = kp_ops.kpconv_weighted(q, s, nbr, x, kp, c["extent"]).cpu().numpy()
            assert wf.shape == (c["nq"], (KK + 31) // 32 * 32)
            assert not wf[:, KK:].any() and not np.isnan(wf[:, KK:]).any()
            _within(wf[:, :KK], c, f"{name}/wrapper switch {int(on)}")
    finally:
        kp_ops.KPCONV_C32 = saved


def test_wrapper_keeps_a_misaligned_input_on_the_generic_kernel(dev):
    """a column slice 4 bytes off the 8-byte grid: the wrapper must not hand it to the entry that refuses it"""
    c = CC.CASES["q5-H5-ns40"]
    q, s, nbr, kp = (_t(c[k], dev) for k in ("q", "s", "nbr", "kp"))
    big = torch.full((c["ns"], CC.CIN + 8), NAN, dtype=torch.float32, device=dev)
    view = big[:, 1:CC.CIN + 1]
    view.copy_(_t(c["x"], dev))
    wf = kp_ops.kpconv_weighted(q, s, nbr, view, kp, c["extent"]).cpu().numpy()
    _within(wf[:, :KK], c, "misaligned slice")


def _rows_rel_l2(got, ref):
    """the measure of test_kpconv_edges_gpu.py::test_kpconv_function_end_to_end: per row |got - ref|_2 / max(|ref|_2, median
    row norm); rows that are exactly 0 in the reference must be exactly 0"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    norms = np.linalg.norm(ref, axis=1)
    zero = norms == 0
    assert not got[zero].any(), "a row that is exactly 0 in the reference is not exactly 0"
    floor = np.median(norms)
    return float((np.linalg.norm(got - ref, axis=1) / np.maximum(norms, floor if floor > 0 else 1.0)).max())


def test_kpconv_function_end_to_end(dev):
    """KPConvFunction at cin = 32, cout = 128, the input NOT requiring grad (the generator's first layer reads detached
    descriptors): out and d W against the float64 oracle at that test's bars (5e-6, 1e-4), no d x, two runs the same bits"""
    name, cout = CC.END_TO_END
    c = CC.CASES[name]
    W, d_out = K.weights(c, cout)
    q, s, nbr, kp = (_t(c[k], dev) for k in ("q", "s", "nbr", "kp"))
    runs = []
    for _ in range(2):
        x = _t(c["x"], dev)
        Wt = _t(W, dev).requires_grad_(True)
        out = kp_ops.KPConvFunction.apply(q, s, nbr, x, Wt, kp, c["extent"])
        out.backward(_t(d_out, dev))
        assert x.grad is None
        runs.append((out.detach().cpu().numpy(), Wt.grad.cpu().numpy()))
    r_out = _rows_rel_l2(runs[0][0], O.forward(*CC.args(c), W))
    r_dw = _rows_rel_l2(runs[0][1].reshape(15, -1), O.d_W(*CC.args(c), d_out).reshape(15, -1))
    print(f"{name} cout {cout}: out {r_out:.3g}  d_W {r_dw:.3g}")
    assert r_out < 5e-6 and r_dw < 1e-4, (r_out, r_dw)
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
