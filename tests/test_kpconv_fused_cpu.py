"""Host-side checks of the fused KPConv forward (apr_kpconv_fused): the shape predicate and the refusals (no device
needed), the facts that make the exact cases of tests/test_kpconv_fused_gpu.py exact, and a NumPy float32 emulation of the
six-term split contraction that shows the bound cases leave the kernel its margin."""
import ctypes as C

import numpy as np
import pytest

import kpconv_fused_cases as F
import kpconv_oracle as O


def test_shape_predicate_refusals_and_struct_sizes(lib):
    from apr_amd import _lib
    for cin in (0, 1, 32, 63, 64, 65, 96, 128, 192, 256, 320, 448, 512, 513, 576, 1024):
        for cout in (0, 32, 64, 96, 128, 256, 448, 512, 576):
            for H in (-1, 0, 1, 2, 64, 127, 128, 129, 255):
                want = cin % 64 == 0 and 64 <= cin <= 512 and cout % 64 == 0 and 64 <= cout <= 512 and 1 <= H <= 128
                assert bool(lib.apr_kpconv_fused_ok(cin, cout, H)) == want, (cin, cout, H)
                assert lib.apr_kpconv_fused_route(1000, cin, cout, H) in ((0, 1) if want else (0,))
    assert lib.apr_kpconv_fused_route(0, 64, 64, 5) == 0
    A = 0x10000      # stand-in pointers: every refusal comes before anything is read or launched

    def call(nq=5, ns=9, H=5, x=A, ldx=64, cin=64, n_kp=15, extent=1.2, w=A, cout=64, out=A, ldo=64):
        return lib.apr_kpconv_fused(A, nq, A, ns, A, H, x, ldx, cin, A, n_kp, extent, A, w, cout, out, ldo, None)

    refused = dict(nkp14=dict(n_kp=14), cin513=dict(cin=513, ldx=516), cin32=dict(cin=32), cin576=dict(cin=576, ldx=576),
                   cout96=dict(cout=96, ldo=96), cout576=dict(cout=576, ldo=576), H0=dict(H=0), H129=dict(H=129),
                   ldx_small=dict(ldx=60), ldo_small=dict(ldo=60), ldx_odd=dict(ldx=65), ldo_odd=dict(ldo=66),
                   x_misaligned=dict(x=A + 4), out_misaligned=dict(out=A + 8), w_misaligned=dict(w=A + 4),
                   ns0=dict(ns=0), nq_negative=dict(nq=-1), extent0=dict(extent=0.0))
    for name, kw in refused.items():
        assert call(**kw) == -1, name                                   # APR_EINVAL
        assert b"apr_kpconv_fused" in lib.apr_last_error(), name
    assert call(nq=0) == 0                                              # nothing to do, nothing launched
    # route 1 of the block with a shape the kernel does not take is an argument error as well
    d = _lib.KpResnetDesc()
    d.x = d.q_pts = d.s_pts = d.nbr = d.w_kpconv = d.w_unary2 = d.kernel_points = d.out = d.scratch = A
    d.ldx = d.ldo = 256
    d.n_in = d.n_out = 10
    d.in_dim, d.mid, d.out_dim, d.H, d.n_kp, d.extent, d.nseg = 256, 64, 256, 129, 15, 1.2, 1
    d.w_unary1 = A
    d.scratch_bytes = 1 << 30
    d.kpconv_route = 1
    assert lib.apr_kp_resnet_block(C.byref(d), None) == -1 and b"kpconv_route" in lib.apr_last_error()
    d.kpconv_route, d.H = 2, 5
    assert lib.apr_kp_resnet_block(C.byref(d), None) == -1 and b"kpconv_route" in lib.apr_last_error()
    out = (C.c_int32 * 16)()
    n = lib.apr_struct_sizes(out, 16)
    assert C.sizeof(_lib.KpResnetDesc) in list(out[:n])
    assert _lib.KpResnetDesc._fields_[-1][0] == "kpconv_route"
    # the scratch walk does not depend on the route
    d.kpconv_route = 0
    a = lib.apr_kp_resnet_scratch_bytes(C.byref(d))
    d.kpconv_route = 1
    assert a > 0 and lib.apr_kp_resnet_scratch_bytes(C.byref(d)) == a


@pytest.mark.parametrize("name", F.EXACT)
def test_exact_cases_are_exact(name):
    """From the oracle's intermediates: influences 0 or 1, num a power of two, wf * num and W integers, sum |wf num| |W| <
    2^24 per output, and the three cross products the kernel drops are 0 for every term.  Then every float32 evaluation
    gives the float64 result."""
    c = F.exact(name)
    out, wf, num, w = F.reference(name)
    assert np.isin(w, (0.0, 1.0)).all()
    assert (num >= 1).all() and (np.log2(num) == np.round(np.log2(num))).all()
    a = wf * num[:, None]
    W2 = c["W"].astype(np.float64).reshape(-1, c["cout"])
    assert np.array_equal(a, np.round(a)) and np.array_equal(W2, np.round(W2))
    assert (np.abs(a) @ np.abs(W2)).max() < 2.0 ** 24
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    a32 = wf.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), wf)                   # wf itself (a / 2^k) is a float32
    _, am, al = F.split3_trunc(a32)
    _, wm, wl = F.split3_rn(W2.astype(np.float32))
    for x, y in ((am, wl), (al, wm), (al, wl)):
        assert not (np.abs(x) @ np.abs(y)).any()
    if c["ns"] >= 8 and c["nq"] >= 60:      # the planted values are reached, with all their pieces
        assert am.any() and al.any() and wm.any() and (a >= 65793).any()
    if c["nq"] >= 3:
        assert not ((c["nbr"][1] >= 0) & (c["nbr"][1] < c["ns"])).any() and not out[1].any()
    assert out.any()


@pytest.mark.parametrize("name", F.BOUND)
def test_split_contraction_emulation_stays_inside_both_thresholds(name):
    """The six cross terms, small first, as float32 matrix products of the bf16 pieces (exact products, float32 sums) on the
    float32-rounded oracle wf: inside the row statistic and the element bound the GPU test asserts."""
    c = F.bound_case(name)
    ref, wf, _, _ = F.reference(name)
    ah, am, al = F.split3_trunc(wf.astype(np.float32))
    wh, wm, wl = F.split3_rn(c["W"].reshape(-1, c["cout"]))
    got = np.zeros(ref.shape, np.float32)
    for x, y in ((ah, wl), (al, wh), (am, wm), (ah, wm), (am, wh), (ah, wh)):
        got = got + x @ y
    r = F.rows_rel_l2(got, ref)
    ratio, at = O.compare_rows(got, ref, F.element_bound(name))
    print(f"{name}: rows rel-L2 {r:.3g}, worst |err| / bound {ratio:.3f}")
    assert r < 5e-6, r
    assert ratio <= 1.0, (ratio, at)
