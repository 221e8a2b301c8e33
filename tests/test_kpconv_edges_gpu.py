"""KPConv step 1, its feature gradient (contribution and atomic form), the reverse table's ordered sum and the neighbour
pools on the GPU, element by element against the float64 oracle (tests/kpconv_oracle.py) on the named cases of
tests/kpconv_cases.py.  The thresholds are the oracle's derived bounds (ratio 1) and exact equality where the oracle says
exact; no row is excluded.  tests/test_kpconv_oracle_cpu.py shows on the host that the cases make every decision with a
margin, that the bounds hold for a plain float32 evaluation and that they reject one-rule mutants.

Worst |kernel - oracle| / bound measured on the MI355X over all cases (records, not thresholds; printed by
test_print_worst_ratios):  wf 0.516,  contrib 0.229,  d_x 0.172.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import kpconv_cases as K
import kpconv_oracle as O
from apr_amd import _lib
from apr_amd.predator import kp_ops

pytestmark = pytest.mark.gpu
NAN = float("nan")
WORST = {"wf": 0.0, "contrib": 0.0, "d_x": 0.0}


def _args(c):
    return c["q"], c["s"], c["nbr"], c["x"], c["kp"], c["extent"]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _view(values, layout, dev):
    """the values [n, c] as an aligned tensor, as the column slice big[:, 1:c + 1] of a NaN-filled buffer (16-byte rows, base
    4 bytes off) or with a row stride of c + 1 floats (ld % 4 != 0 for c % 4 == 0) -> (view, ld)"""
    n, c = values.shape
    if layout == "aligned":
        t = _t(values, dev)
        return t, c
    big = torch.full((n, c + 8 if layout == "slice1" else c + 1), NAN, dtype=torch.float32, device=dev)
    view = big[:, 1:c + 1] if layout == "slice1" else big[:, :c]
    view.copy_(_t(values, dev))
    return view, big.stride(0)


def _geom(c, dev):
    return _t(c["q"], dev), _t(c["s"], dev), _t(c["nbr"], dev), _t(c["kp"], dev)


def _record(key, got, ref, bound, what):
    ratio, at = O.compare_rows(got, ref, bound)
    print(f"{what}: worst {key} ratio {ratio:.4f}")
    WORST[key] = max(WORST[key], ratio if np.isfinite(ratio) else 1e30)
    assert ratio <= 1.0, (what, key, ratio, at, None if at is None else (float(got[at]), float(ref[at]), float(bound[at])))


def _weighted_direct(dev, c, layout):
    lib = _lib.load()
    q, s, nbr, kp = _geom(c, dev)
    nq, ns, H, cin = c["nq"], c["ns"], c["H"], c["cin"]
    xv, ldx = _view(c["x"], layout, dev)
    rs = kp_ops.row_sums(xv)
    kk = 15 * cin
    ldwf = (kk + 31) // 32 * 32 + 32
    wf = torch.full((nq, ldwf), NAN, dtype=torch.float32, device=dev)
    _lib.check(lib.apr_kpconv_weighted(_lib.ptr(q), nq, _lib.ptr(s), ns, _lib.ptr(nbr), H, _lib.ptr(xv), ldx, cin, _lib.ptr(kp), 15,
                                       c["extent"], _lib.ptr(rs), _lib.ptr(wf), ldwf, _lib.stream()))
    torch.cuda.synchronize()
    wf = wf.cpu().numpy()
    return wf[:, :kk], wf[:, kk:]


# ----------------------------------------------------------------------------------------------------------- step 1
@pytest.mark.parametrize("name", list(K.FORWARD))
def test_step1_every_element_within_bound(dev, name):
    """NaN-filled wf with 32 guard columns behind 15 * cin rounded up to 32: every element inside is within the bound (a row
    or channel group that no wave wrote is still NaN, one written twice with another query's values is off), every guard
    element is still NaN."""
    c = K.FORWARD[name]
    ref, _, _ = O.weighted(*_args(c))
    got, guard = _weighted_direct(dev, c, c["layout"])
    assert np.isnan(guard).all(), "columns behind 15 * cin were written"
    _record("wf", got, ref, O.bound_weighted(*_args(c)), name)


@pytest.mark.parametrize("layout", ["slice1", "ldodd"])
@pytest.mark.parametrize("name", ["m1-c64", "m2-c128", "m4-c320"])
def test_step1_both_routes_meet_the_oracle_on_the_same_values(dev, name, layout):
    """an aligned case again through a misaligned column slice / a row stride that is no multiple of 4: the generic kernel on
    the MFMA kernel's input"""
    c = K.FORWARD[name]
    assert K.expected_route(c["cin"], c["H"], layout) == "generic" != K.expected_route(c["cin"], c["H"], "aligned")
    ref, _, _ = O.weighted(*_args(c))
    got, guard = _weighted_direct(dev, c, layout)
    assert np.isnan(guard).all()
    _record("wf", got, ref, O.bound_weighted(*_args(c)), f"{name}/{layout}")


@pytest.mark.parametrize("name", list(K.FORWARD))
def test_step1_wrapper_pads_with_zeros(dev, name):
    """kp_ops.kpconv_weighted: [nq, 15 * cin rounded up to 32], the padding columns exactly 0 (the GEMM reads them)"""
    c = K.FORWARD[name]
    q, s, nbr, kp = _geom(c, dev)
    xv, _ = _view(c["x"], c["layout"], dev)
    wf = kp_ops.kpconv_weighted(q, s, nbr, xv, kp, c["extent"]).cpu().numpy()
    kk = 15 * c["cin"]
    assert wf.shape == (c["nq"], (kk + 31) // 32 * 32)
    assert not wf[:, kk:].any() and not np.isnan(wf[:, kk:]).any()
    ref, _, _ = O.weighted(*_args(c))
    _record("wf", wf[:, :kk], ref, O.bound_weighted(*_args(c)), name + "/wrapper")


# -------------------------------------------------------------------------------------------------- feature gradient
def _dwf(c, dev):
    kk = 15 * c["cin"]
    big = torch.full((c["nq"], kk + 3), NAN, dtype=torch.float32, device=dev)
    big[:, :kk] = _t(c["dwf"], dev)
    return big, kk + 3


def _rev_build(dev, nbr_t, nq, H, ns):
    lib = _lib.load()
    rev = torch.full((nq * H,), -1, dtype=torch.int32, device=dev)
    start = torch.full((ns + 1,), -1, dtype=torch.int32, device=dev)
    sb = int(lib.apr_reverse_table_scratch_bytes(nq, H, ns))
    scratch = torch.empty(max(sb, 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.apr_reverse_table_build(_lib.ptr(nbr_t), nq, H, ns, _lib.ptr(rev), _lib.ptr(start), _lib.ptr(scratch), sb,
                                           _lib.stream()))
    return rev, start


@pytest.mark.parametrize("name", [n for n, c in K.BACKWARD.items() if c["cin"] % 4 == 0])
def test_contribution_rows_and_ordered_sum(dev, name):
    c = K.BACKWARD[name]
    lib = _lib.load()
    nq, ns, H, cin = c["nq"], c["ns"], c["H"], c["cin"]
    q, s, nbr, kp = _geom(c, dev)
    x = _t(c["x"], dev)
    rs = kp_ops.row_sums(x)
    dwf, lddwf = _dwf(c, dev)
    contrib = torch.full((nq * H, cin), NAN, dtype=torch.float32, device=dev)
    _lib.check(lib.apr_kpconv_dfeat_contrib(_lib.ptr(q), nq, _lib.ptr(s), ns, _lib.ptr(nbr), H, _lib.ptr(dwf), lddwf, cin,
                                            _lib.ptr(kp), 15, c["extent"], _lib.ptr(rs), _lib.ptr(contrib), _lib.stream()))
    rows = contrib.cpu().numpy()
    real = O.real_mask(c["nbr"], ns).reshape(-1)
    assert np.isnan(rows[~real]).all(), "rows of padding neighbours are documented as untouched"
    ref, bound = O.contrib(*_args(c), c["dwf"]), O.bound_contrib(*_args(c), c["dwf"])
    _record("contrib", rows[real], ref[real], bound[real], name)

    rev, start = _rev_build(dev, nbr, nq, H, ns)
    ldo, total = cin + 4, nq * H

    def fresh():
        return torch.full((ns, ldo), NAN, dtype=torch.float32, device=dev)

    def ranged(edges):
        out = fresh()
        for i, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
            src = C.c_void_p(contrib.data_ptr() + lo * cin * 4)
            _lib.check(lib.apr_reverse_gather_range(src, cin, _lib.ptr(rev), _lib.ptr(start), ns, lo, hi, int(i > 0), _lib.ptr(out),
                                                    ldo, _lib.stream()))
        return out.cpu().numpy()

    whole = fresh()
    _lib.check(lib.apr_reverse_gather(_lib.ptr(contrib), cin, _lib.ptr(rev), _lib.ptr(start), ns, _lib.ptr(whole), ldo,
                                      _lib.stream()))
    whole = whole.cpu().numpy()
    assert np.isnan(whole[:, cin:]).all() and not np.isnan(whole[:, :cin]).any()
    mid = (nq // 2) * H
    sums = {"1 query": ranged(list(range(0, total + 1, H))),
            "3 queries": ranged(sorted(set(list(range(0, total, 3 * H)) + [total]))),
            "all": ranged([0, total]),
            "empty chunk": ranged([0, mid, mid, total])}
    for what, got in sums.items():
        assert np.isnan(got[:, cin:]).all(), what
        assert got[:, :cin].tobytes() == whole[:, :cin].tobytes(), f"chunks of {what}: other bits than one gather"
    pointed = np.zeros(ns, bool)
    pointed[c["nbr"].reshape(-1)[real]] = True
    assert not whole[~pointed, :cin].any(), "a support row nobody points at is not exactly 0"
    _record("d_x", whole[:, :cin], O.d_x_from_dwf(*_args(c), c["dwf"]), O.bound_dx(*_args(c), c["dwf"]), name)


@pytest.mark.parametrize("name", list(K.BACKWARD))
def test_atomic_form(dev, name):
    c = K.BACKWARD[name]
    lib = _lib.load()
    nq, ns, H, cin = c["nq"], c["ns"], c["H"], c["cin"]
    q, s, nbr, kp = _geom(c, dev)
    x = _t(c["x"], dev)
    rs = kp_ops.row_sums(x)
    dwf, lddwf = _dwf(c, dev)
    lddx = cin + 3
    dx = torch.zeros((ns, lddx), dtype=torch.float32, device=dev)
    dx[:, cin:] = NAN
    _lib.check(lib.apr_kpconv_dfeat(_lib.ptr(q), nq, _lib.ptr(s), ns, _lib.ptr(nbr), H, _lib.ptr(dwf), lddwf, cin, _lib.ptr(kp), 15,
                                    c["extent"], _lib.ptr(rs), _lib.ptr(dx), lddx, _lib.stream()))
    got = dx.cpu().numpy()
    assert np.isnan(got[:, cin:]).all(), "columns behind cin were touched"
    _record("d_x", got[:, :cin], O.d_x_from_dwf(*_args(c), c["dwf"]), O.bound_dx(*_args(c), c["dwf"]), name + "/atomic")


@pytest.mark.parametrize("name", list(K.REFUSED))
def test_refusals(dev, name):
    """cin = 513 and H = 129 (feature gradient) and 14 kernel points (all three entry points): the argument error, nothing
    written"""
    r = K.REFUSED[name]
    lib = _lib.load()
    cin, H, n_kp, nq, ns = r["cin"], r["H"], r["n_kp"], 5, 9
    rng = np.random.default_rng(7)
    q, s = _t(rng.uniform(-1, 1, (nq, 3)).astype(np.float32), dev), _t(rng.uniform(-1, 1, (ns, 3)).astype(np.float32), dev)
    kp = _t(rng.uniform(-1, 1, (15, 3)).astype(np.float32), dev)
    nbr = _t(rng.integers(0, ns + 1, (nq, H)).astype(np.int32), dev)
    x = _t(rng.standard_normal((ns, cin)).astype(np.float32), dev)
    dwf = _t(rng.standard_normal((nq, 15 * cin)).astype(np.float32), dev)
    rs = kp_ops.row_sums(x)
    pattern = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    dx, contrib, wf = pattern(ns * cin * 4), pattern(nq * H * cin * 4), pattern(nq * 15 * cin * 4)
    calls = [
        lambda: lib.apr_kpconv_dfeat(_lib.ptr(q), nq, _lib.ptr(s), ns, _lib.ptr(nbr), H, _lib.ptr(dwf), 15 * cin, cin, _lib.ptr(kp), n_kp,
                                     1.2, _lib.ptr(rs), _lib.ptr(dx), cin, _lib.stream()),
        lambda: lib.apr_kpconv_dfeat_contrib(_lib.ptr(q), nq, _lib.ptr(s), ns, _lib.ptr(nbr), H, _lib.ptr(dwf), 15 * cin, cin,
                                             _lib.ptr(kp), n_kp, 1.2, _lib.ptr(rs), _lib.ptr(contrib), _lib.stream()),
    ]
    if n_kp != 15:
        calls.append(lambda: lib.apr_kpconv_weighted(_lib.ptr(q), nq, _lib.ptr(s), ns, _lib.ptr(nbr), H, _lib.ptr(x), cin, cin,
                                                     _lib.ptr(kp), n_kp, 1.2, _lib.ptr(rs), _lib.ptr(wf), 15 * cin, _lib.stream()))
    for call in calls:
        assert call() == -1                                     # APR_EINVAL
        assert lib.apr_last_error().decode()
    torch.cuda.synchronize()
    for buf in (dx, contrib, wf):
        assert bool((buf == 0xA5).all()), "a refused call wrote to its output"


# ---------------------------------------------------------------------------------------------------- reverse table
@pytest.mark.parametrize("name", list(K.REVERSE))
def test_reverse_table_build(dev, name):
    c = K.REVERSE[name]
    nq, H, ns = c["nq"], c["H"], c["ns"]
    ref_rev, ref_start = O.reverse_table(c["nbr"], ns)
    nbr = _t(c["nbr"], dev)
    rev, start = (t.cpu().numpy() for t in _rev_build(dev, nbr, nq, H, ns))
    n_real = int(ref_start[ns])
    assert np.array_equal(start, ref_start)
    assert np.array_equal(rev[:n_real], ref_rev[:n_real])
    assert sorted(rev[n_real:]) == sorted(ref_rev[n_real:]), "the tail holds the padding positions"
    rev2, start2 = (t.cpu().numpy() for t in _rev_build(dev, nbr, nq, H, ns))
    assert rev2.tobytes() == rev.tobytes() and start2.tobytes() == start.tobytes()


# ------------------------------------------------------------------------------------------------------ end to end
def _rows_rel_l2(got, ref):
    """per row: |got - ref|_2 / max(|ref|_2, median row norm); rows that are exactly 0 in the reference must be exactly 0"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    norms = np.linalg.norm(ref, axis=1)
    zero = norms == 0
    assert not got[zero].any(), "a row that is exactly 0 in the reference is not exactly 0"
    floor = np.median(norms)
    return float((np.linalg.norm(got - ref, axis=1) / np.maximum(norms, floor if floor > 0 else 1.0)).max())


@pytest.mark.parametrize("det", [True, False], ids=["default", "atomic"])
@pytest.mark.parametrize("name,cout", K.END_TO_END)
def test_kpconv_function_end_to_end(dev, name, cout, det):
    c = K.ALL[name]
    W, d_out = K.weights(c, cout)
    q, s, nbr, kp = _geom(c, dev)
    x = _t(c["x"], dev).requires_grad_(True)
    Wt = _t(W, dev).requires_grad_(True)
    saved = kp_ops.DET_DX
    kp_ops.DET_DX = det
    try:
        out = kp_ops.KPConvFunction.apply(q, s, nbr, x, Wt, kp, c["extent"])
        out.backward(_t(d_out, dev))
    finally:
        kp_ops.DET_DX = saved
    r_out = _rows_rel_l2(out.detach().cpu().numpy(), O.forward(*_args(c), W))
    r_dx = _rows_rel_l2(x.grad.cpu().numpy(), O.d_x(*_args(c), W, d_out))
    dW, dW_ref = Wt.grad.cpu().numpy(), O.d_W(*_args(c), d_out)
    r_dw = _rows_rel_l2(dW.reshape(15, -1), dW_ref.reshape(15, -1))
    print(f"{name} cout {cout} det {det}: out {r_out:.3g}  d_x {r_dx:.3g}  d_W {r_dw:.3g}")
    assert r_out < 5e-6 and r_dx < 1e-4 and r_dw < 1e-4, (r_out, r_dx, r_dw)


# ------------------------------------------------------------------------------------------------------------ pools
@pytest.mark.parametrize("name", list(K.POOLS))
def test_pools_exact(dev, name):
    c = K.POOLS[name]
    lib = _lib.load()
    nq, ns, H, ch = c["nq"], c["ns"], c["H"], c["c"]
    xv, ldx = _view(c["x"], c["layout"], dev)
    inds = _t(c["inds"], dev)
    ref_out, ref_amax = O.max_pool(c["x"], c["inds"])
    ref_out, ref_close = ref_out.astype(np.float32), O.closest_pool(c["x"], c["inds"]).astype(np.float32)
    assert np.array_equal(kp_ops.gather_pool(xv, inds, "max").cpu().numpy(), ref_out)
    assert np.array_equal(kp_ops.gather_pool(xv, inds, "closest").cpu().numpy(), ref_close)
    # the arg-max kernel itself, on the same view
    out = torch.full((nq, ch + 1), NAN, dtype=torch.float32, device=dev)
    amax = torch.full((nq, ch), 0xEE, dtype=torch.uint8, device=dev)
    _lib.check(lib.apr_gather_pool_argmax(_lib.ptr(xv), ldx, ns, ch, _lib.ptr(inds), H, nq, _lib.ptr(out), ch + 1, _lib.ptr(amax),
                                          _lib.stream()))
    out = out.cpu().numpy()
    assert np.array_equal(out[:, :ch], ref_out) and np.isnan(out[:, ch]).all()
    assert np.array_equal(amax.cpu().numpy(), ref_amax.astype(np.uint8)), "not the first maximum"
    # forward and backward of the training functions
    for mode, ref_fwd, ref_grad in (("max", ref_out, O.max_pool_grad), ("closest", ref_close, O.closest_pool_grad)):
        x = _t(c["x"], dev).requires_grad_(True)
        y = kp_ops.PoolFunction.apply(x, inds, mode)
        assert np.array_equal(y.detach().cpu().numpy(), ref_fwd)
        y.backward(_t(c["dout"], dev))
        assert np.array_equal(x.grad.cpu().numpy(), ref_grad(c["x"], c["inds"], c["dout"]).astype(np.float32)), mode
    for row, plant in c["plants"].items():
        if plant[0] == "shadowmax":      # a gradient that arrives at the shadow maximum alone goes to no row
            x = _t(c["x"], dev).requires_grad_(True)
            y = kp_ops.PoolFunction.apply(x, inds, "max")
            g = torch.zeros_like(y)
            g[row, 0] = 3.0
            y.backward(g)
            assert float(y.detach()[row, 0]) == 0.0 and not x.grad.cpu().numpy().any()


def test_print_worst_ratios():
    print("worst kernel / bound:", {k: round(v, 4) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())
