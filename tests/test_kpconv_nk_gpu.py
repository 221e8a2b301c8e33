"""Rigid KPConv with any kernel-point count on the GPU (apr_kpconv_weighted_nk, apr_kpconv_dfeat_contrib_nk;
csrc/kpconv_nk.hip): step 1, the contribution rows and their ordered sum element by element against the float64 oracle
(tests/kpconv_nk_oracle.py) on the named cases of tests/kpconv_nk_cases.py at the oracle's derived bounds (ratio 1; every
mode at n_kp = 7, 15 and 20, (linear, sum) and (gaussian, closest) elsewhere; both routes), n_kp = 15 bit for bit against the
*_mode entries in every mode on both routes, the wrapper's zero padding, the one-call residual block at n_kp = 7, blocks.KPConv at K = 7 and
20 on the kernels and on the torch formulation, a deformable K = 7 layer, KPFCNN(kitti_config(num_kernel_points=7)) against
oracle/kpfcnn_oracle.py, and one training iteration at K = 7.

Worst |kernel - oracle| / bound measured on the MI355X over all cases and modes (records, not thresholds; printed by
test_print_worst_ratios; by mode in DESIGN section 38):  wf 0.439,  contrib 0.385,  d_x 0.417.
"""
import numpy as np
import pytest
import torch

import kpconv_nk_cases as NC
import kpconv_nk_oracle as NO
from apr_amd import _lib, synth
from apr_amd.predator import kp_ops
from apr_amd.predator.configs.models import kitti_config
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
NAN = float("nan")
WORST = {}
P = _lib.ptr
CASE_MODES = [(n, m) for n in NC.CASES for m in NC.case_modes(n)]
CASE_MODE_IDS = [f"{n}-{NO.mode_name(m)}" for n, m in CASE_MODES]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _args(c):
    return c["q"], c["s"], c["nbr"], c["x"], c["kp"], c["extent"]


def _view(values, layout, dev):
    """the values [n, c] as an aligned tensor or as the column slice big[:, 1:c + 1] of a NaN-filled buffer (16-byte rows, the
    base 4 bytes off) -> (view, ld)"""
    n, c = values.shape
    if layout == "aligned":
        return _t(values, dev), c
    big = torch.full((n, c + 8), NAN, dtype=torch.float32, device=dev)
    view = big[:, 1:c + 1]
    view.copy_(_t(values, dev))
    return view, big.stride(0)


def _record(key, mode, got, ref, bound, what):
    ratio, at = NO.compare_rows(got, ref, bound)
    print(f"{what} {NO.mode_name(mode)}: worst {key} ratio {ratio:.4f}")
    k = (key, NO.mode_name(mode))
    WORST[k] = max(WORST.get(k, 0.0), ratio if np.isfinite(ratio) else 1e30)
    assert ratio <= 1.0, (what, key, mode, ratio, at, None if at is None else (float(got[at]), float(ref[at]), float(bound[at])))


def _dev(c, dev):
    d = dict(q=_t(c["q"], dev), s=_t(c["s"], dev), nbr=_t(c["nbr"], dev), kp=_t(c["kp"], dev))
    d["x"], d["ldx"] = _view(c["x"], c["layout"], dev)
    d["rs"] = kp_ops.row_sums(d["x"])
    return d


def _step1(lib, fn, c, d, mode, dev):
    """-> wf [nq, K cin rounded up to 4, + 32 guard columns], NaN-filled before the call"""
    nq, ns, H, cin, K = c["nq"], c["ns"], c["H"], c["cin"], c["n_kp"]
    ld = (K * cin + 3) // 4 * 4 + 32
    wf = torch.full((nq, ld), NAN, dtype=torch.float32, device=dev)
    _lib.check(fn(P(d["q"]), nq, P(d["s"]), ns, P(d["nbr"]), H, P(d["x"]), d["ldx"], cin, P(d["kp"]), K, c["extent"], P(d["rs"]),
                  P(wf), ld, mode[0], mode[1], _lib.stream()))
    return wf


# ------------------------------------------------------------------------------------- the two entries, every case
@pytest.mark.parametrize("name,mode", CASE_MODES, ids=CASE_MODE_IDS)
def test_step1_and_feature_gradient_within_bound(dev, name, mode):
    c = NC.CASES[name]
    lib = _lib.load()
    nq, ns, H, cin, K = c["nq"], c["ns"], c["H"], c["cin"], c["n_kp"]
    d = _dev(c, dev)
    kk = K * cin
    a = _args(c)
    wf_t = _step1(lib, lib.apr_kpconv_weighted_nk, c, d, mode, dev)
    wf = wf_t.cpu().numpy()
    assert np.isnan(wf[:, kk:]).all(), "columns behind n_kp * cin were written"
    _record("wf", mode, wf[:, :kk], NO.weighted(*a, mode)[0], NO.bound_weighted(*a, mode), name)
    for row, kind in c["plants"].items():
        if kind == "allpad":
            assert not wf[row, :kk].any(), "a query with no real neighbour: not exactly 0"
    assert torch.equal(_step1(lib, lib.apr_kpconv_weighted_nk, c, d, mode, dev)[:, :kk], wf_t[:, :kk]), "two runs, other bits"
    if K == 15:      # the bits of the entry built for 15 kernel points, on whichever route the case takes
        old = _step1(lib, lib.apr_kpconv_weighted_mode, c, d, mode, dev)
        assert torch.equal(old[:, :kk], wf_t[:, :kk]), "n_kp = 15: other bits than apr_kpconv_weighted_mode"

    lddwf = kk + 4
    dwf = torch.full((nq, lddwf), NAN, dtype=torch.float32, device=dev)
    dwf[:, :kk] = _t(c["dwf"], dev)

    def contrib_rows(fn):
        buf = torch.full((nq * H, cin), NAN, dtype=torch.float32, device=dev)
        _lib.check(fn(P(d["q"]), nq, P(d["s"]), ns, P(d["nbr"]), H, P(dwf), lddwf, cin, P(d["kp"]), K, c["extent"], P(d["rs"]),
                      P(buf), mode[0], mode[1], _lib.stream()))
        return buf

    contrib = contrib_rows(lib.apr_kpconv_dfeat_contrib_nk)
    rows = contrib.cpu().numpy()
    real = NO.O.real_mask(c["nbr"], ns).reshape(-1)
    assert np.isnan(rows[~real]).all(), "rows of padding neighbours are documented as untouched"
    _record("contrib", mode, rows[real], NO.contrib(*a, c["dwf"], mode)[real], NO.bound_contrib(*a, c["dwf"], mode)[real], name)
    if K == 15:      # every mode: kpconv_nk.hip spells out the d2 forms that k_kpconv_dfeat compiles to (dfeat_d2)
        old = contrib_rows(lib.apr_kpconv_dfeat_contrib_mode).cpu().numpy()
        same = old.view(np.uint32) == rows.view(np.uint32)
        assert same.all(), ("n_kp = 15: other bits than apr_kpconv_dfeat_contrib_mode", int((~same).sum()), same.size)
    if cin % 4 == 0:      # the ordered sum reads 16-byte rows
        rev, start = kp_ops.reverse_table(d["nbr"], ns)
        dx = torch.full((ns, cin + 4), NAN, dtype=torch.float32, device=dev)
        _lib.check(lib.apr_reverse_gather(P(contrib), cin, P(rev), P(start), ns, P(dx), cin + 4, _lib.stream()))
        dx = dx.cpu().numpy()
        assert np.isnan(dx[:, cin:]).all() and not np.isnan(dx[:, :cin]).any()
        _record("d_x", mode, dx[:, :cin], NO.d_x_from_dwf(*a, c["dwf"], mode), NO.bound_dx(*a, c["dwf"], mode), name)


@pytest.mark.parametrize("name", ["k7-c64-H5-nq70", "k20-c128-H65-nq5", "k32-c320-H64-nq5"])
def test_generic_route_meets_the_oracle_on_the_mfma_cases(dev, name):
    """an aligned case again through a misaligned column slice: one thread per (query, kernel point) on the MFMA kernel's input"""
    c = dict(NC.CASES[name], layout="slice1")
    assert NC.expected_route(c) == "generic" != NC.expected_route(NC.CASES[name])
    lib = _lib.load()
    d = _dev(c, dev)
    kk = c["n_kp"] * c["cin"]
    for mode in (NO.DEFAULT, (NO.LINEAR, 1)):
        wf = _step1(lib, lib.apr_kpconv_weighted_nk, c, d, mode, dev).cpu().numpy()
        assert np.isnan(wf[:, kk:]).all()
        _record("wf", mode, wf[:, :kk], NO.weighted(*_args(c), mode)[0], NO.bound_weighted(*_args(c), mode), name + "/slice")


@pytest.mark.parametrize("name", ["k7-c1-H5-nq70", "k20-c3-H65-nq5", "k17-c32-H3-nq5", "k7-c64-H5-nq70", "k1-c1-H1-nq1"])
def test_wrapper_pads_with_exact_zeros(dev, name):
    """kp_ops.kpconv_weighted at K != 15: [nq, K cin rounded up to 32], the padding columns exactly 0 (the GEMM reads them)"""
    c = NC.CASES[name]
    xv, _ = _view(c["x"], c["layout"], dev)
    wf = kp_ops.kpconv_weighted(_t(c["q"], dev), _t(c["s"], dev), _t(c["nbr"], dev), xv, _t(c["kp"], dev), c["extent"]).cpu().numpy()
    kk = c["n_kp"] * c["cin"]
    assert wf.shape == (c["nq"], (kk + 31) // 32 * 32)
    assert not wf[:, kk:].any() and not np.isnan(wf[:, kk:]).any()
    _record("wf", NO.DEFAULT, wf[:, :kk], NO.weighted(*_args(c))[0], NO.bound_weighted(*_args(c)), name + "/wrapper")


# ------------------------------------------------------------------------------------------------------- the module
def _rows_rel_l2(got, ref):
    """per row: |got - ref|_2 / max(|ref|_2, median row norm); rows that are exactly 0 in the reference must be exactly 0"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    norms = np.linalg.norm(ref, axis=1)
    zero = norms == 0
    assert not got[zero].any(), "a row that is exactly 0 in the reference is not exactly 0"
    floor = np.median(norms)
    return float((np.linalg.norm(got - ref, axis=1) / np.maximum(norms, floor if floor > 0 else 1.0)).max())


def _count_torch_route(monkeypatch, blocks):
    calls = []
    orig = blocks.KPConv._forward_autograd

    def spy(self, *a):
        calls.append(self.K)
        return orig(self, *a)

    monkeypatch.setattr(blocks.KPConv, "_forward_autograd", spy)
    return calls


@pytest.mark.parametrize("mode", [NO.DEFAULT, (NO.GAUSSIAN, 1)], ids=NO.mode_name)
@pytest.mark.parametrize("name,cout", NC.MODULE)
def test_module_on_the_kernels_and_on_the_torch_formulation(dev, name, cout, mode, monkeypatch):
    """blocks.KPConv(7, ..) and (20, ..) at cin = 64: inference out and training out element by element inside the oracle's bound
    carried through the contraction (below); out, d x and d W against the float64 statement at the bars every KPConv module
    test here uses (out 5e-6, gradients 1e-4; per row / per kernel point, relative L2 floored at the median row norm: the
    oracle has no element bound for a gradient behind two GEMMs, and these are the bars of tests/test_kpconv_modes_gpu.py and
    tests/test_kpconv_deform_gpu.py) -- on the *_nk kernels and, with KPCONV_NK_HIP off, on the torch formulation.  Padding is spelled ns,
    as the reference's tables spell it."""
    from apr_amd.predator.models import blocks
    monkeypatch.setattr(blocks, "KPCONV_MODES", True)
    c = dict(NC.CASES[name])
    K = c["n_kp"]
    c["nbr"] = np.where(NO.O.real_mask(c["nbr"], c["ns"]), c["nbr"], c["ns"]).astype(np.int32)
    W, d_out = NC.weights(c, cout)
    np.random.seed(1)
    conv = blocks.KPConv(K, 3, c["cin"], cout, c["extent"], 1.0, KP_influence=NO.MO.NAMES[mode[0]],
                         aggregation_mode="closest" if mode[1] else "sum")
    assert tuple(conv.kernel_points.shape) == (K, 3) and tuple(conv.weights.shape) == (K, c["cin"], cout)
    with torch.no_grad():
        conv.weights.copy_(torch.from_numpy(W))
        conv.kernel_points.copy_(torch.from_numpy(c["kp"]))
    conv = conv.to(dev)
    a = _args(c)
    ref = dict(out=NO.forward(*a, W, mode), d_x=NO.d_x(*a, W, d_out, mode), d_W=NO.d_W(*a, d_out, mode))
    # the oracle's bound carried through the contraction, per element of out: the error of wf enters linearly (bound_weighted @
    # |W|); a float32 sum of K cin products in any order adds K cin u sum |wf W|, the bf16-split six-term contraction of the
    # inference GEMM 16 eps32 sum |wf W|: their sum covers either GEMM
    W2 = np.abs(W.astype(np.float64).reshape(K * c["cin"], cout))
    b_out = NO.bound_weighted(*a, mode) @ W2 + (16 * NO.EPS32 + K * c["cin"] * NO.U) * (np.abs(NO.weighted(*a, mode)[0]) @ W2)
    calls = _count_torch_route(monkeypatch, blocks)
    q, s, nbr = _t(c["q"], dev), _t(c["s"], dev), _t(c["nbr"], dev)
    for hip in (True, False):
        monkeypatch.setattr(blocks, "KPCONV_NK_HIP", hip)
        del calls[:]
        with torch.no_grad():
            inf = conv(q, s, nbr, _t(c["x"], dev)).cpu().numpy()
        conv.zero_grad()
        x = _t(c["x"], dev).requires_grad_(True)
        out = conv(q, s, nbr, x)
        out.backward(_t(d_out, dev))
        assert len(calls) == (0 if hip else 2), "the layer did not take the route the switch names"
        for what, got in (("inference out", inf), ("training out", out.detach().cpu().numpy())):
            ratio, at = NO.compare_rows(got, ref["out"], b_out)
            print(f"{name} {NO.mode_name(mode)} {'HIP' if hip else 'torch'} {what}: worst |out - oracle| / bound {ratio:.4f}")
            assert ratio <= 1.0, (what, ratio, at)
        e = dict(inf=_rows_rel_l2(inf, ref["out"]), out=_rows_rel_l2(out.detach().cpu().numpy(), ref["out"]),
                 d_x=_rows_rel_l2(x.grad.cpu().numpy(), ref["d_x"]),
                 d_W=_rows_rel_l2(conv.weights.grad.cpu().numpy().reshape(K, -1), ref["d_W"].reshape(K, -1)))
        print(f"{name} {NO.mode_name(mode)} {'HIP' if hip else 'torch'}: {({k: float(f'{v:.3g}') for k, v in e.items()})}")
        assert e["inf"] < 5e-6 and e["out"] < 5e-6 and e["d_x"] < 1e-4 and e["d_W"] < 1e-4, e


def test_deformable_k7_layer_matches_its_all_torch_route(dev, monkeypatch):
    """KPConv(7, deformable, modulated): offset_conv is a rigid K = 7 layer (the *_nk kernels in inference), the deformed
    correlation has no K != 15 kernel and runs the torch formulation.  Forward and backward against the route with
    KPCONV_NK_HIP off at the bars of tests/test_kpconv_deform_gpu.py's module test (out 5e-6, gradients 1e-4)."""
    from apr_amd.predator.models import blocks
    c = dict(NC.CASES["k7-c64-H5-nq70"])
    c["nbr"] = np.where(NO.O.real_mask(c["nbr"], c["ns"]), c["nbr"], c["ns"]).astype(np.int32)
    K, cin, cout = 7, c["cin"], 64
    W, d_out = NC.weights(c, cout)
    np.random.seed(2)
    torch.manual_seed(2)
    conv = blocks.KPConv(K, 3, cin, cout, c["extent"], 1.0, deformable=True, modulated=True)
    assert conv.offset_dim == 28 and conv.offset_conv.K == 7
    rng = np.random.default_rng(77)
    with torch.no_grad():
        conv.weights.copy_(torch.from_numpy(W))
        conv.kernel_points.copy_(torch.from_numpy(c["kp"]))
        conv.offset_conv.kernel_points.copy_(torch.from_numpy(c["kp"]))
        conv.offset_conv.weights.copy_(torch.from_numpy((rng.standard_normal((K, cin, 28)) * 0.15 / np.sqrt(K * cin)).astype(np.float32)))
        conv.offset_bias.copy_(torch.from_numpy((rng.standard_normal(28) * 0.05).astype(np.float32)))
    conv = conv.to(dev)
    q, s, nbr = _t(c["q"], dev), _t(c["s"], dev), _t(c["nbr"], dev)
    calls = _count_torch_route(monkeypatch, blocks)
    res = {}
    for hip in (True, False):
        monkeypatch.setattr(blocks, "KPCONV_NK_HIP", hip)
        del calls[:]
        with torch.no_grad():
            inf = conv(q, s, nbr, _t(c["x"], dev)).cpu().numpy()
        assert len(calls) == (0 if hip else 1), "offset_conv's inference route"
        assert tuple(conv.deformed_KP.shape) == (c["nq"], 7, 3) and tuple(conv.min_d2.shape) == (c["nq"], 7)
        conv.zero_grad()
        x = _t(c["x"], dev).requires_grad_(True)
        out = conv(q, s, nbr, x)
        out.backward(_t(d_out, dev))
        res[hip] = dict(inf=inf, out=out.detach().cpu().numpy(), d_x=x.grad.cpu().numpy(),
                        d_W=conv.weights.grad.cpu().numpy().reshape(K, -1),
                        d_W_off=conv.offset_conv.weights.grad.cpu().numpy().reshape(K, -1),
                        d_b_off=conv.offset_bias.grad.cpu().numpy().reshape(1, -1))
        assert all(np.isfinite(v).all() for v in res[hip].values()) and res[hip]["out"].any() and res[hip]["d_W_off"].any()
    e = {k: _rows_rel_l2(res[True][k], res[False][k]) for k in res[True]}
    print("deformable K = 7, kernels vs all-torch:", {k: float(f"{v:.3g}") for k, v in e.items()})
    assert e["inf"] < 5e-6 and e["out"] < 5e-6, e
    assert max(e[k] for k in ("d_x", "d_W", "d_W_off", "d_b_off")) < 1e-4, e


# ------------------------------------------------------------------------------------------------------ the network
def _small_pair():
    from oracle import predator_points_oracle as PREF
    a, b, _ = synth.make_pair(11, n_beams=4, n_azimuth=200)
    pts, lens = PREF.subsample_batch(np.concatenate([a, b]), np.array([len(a), len(b)], np.int32), sampleDl=0.3)
    return pts[:lens[0]], pts[lens[0]:]


def test_kpfcnn_k7_matches_the_oracle(dev):
    """KPFCNN(kitti_config(num_kernel_points=7)) on a synthetic pair of about 600 points per cloud against
    oracle/kpfcnn_oracle.py fed the model's state_dict, at the tolerance of the K = 15 parity test
    (tests/test_predator_gpu.py::test_kpfcnn_matches_oracle_other_seed: 1e-4)."""
    from apr_amd.predator.datasets.dataloader import collate_fn_descriptor
    from apr_amd.predator.models import blocks
    from apr_amd.predator.models.architectures import KPFCNN
    from oracle import kpfcnn_oracle as KO
    from oracle import predator_points_oracle as PREF
    if not PREF.available():
        pytest.skip("oracle/_ref not built")
    cfg, lim = kitti_config(num_kernel_points=7), [35, 33, 34, 36]
    np.random.seed(5)
    torch.manual_seed(5)
    model = KPFCNN(cfg).to(dev).eval()
    assert all(tuple(m.kernel_points.shape) == (7, 3) for m in model.modules() if isinstance(m, blocks.KPConv))
    src, tgt = _small_pair()
    assert 500 <= len(src) <= 700 and 500 <= len(tgt) <= 700
    ref = KO.kpfcnn_forward({k: v.cpu() for k, v in model.state_dict().items()}, cfg, KO.collate(src, tgt, cfg, lim))
    batch = collate_fn_descriptor([(src, tgt, np.ones((len(src), 1), np.float32), np.ones((len(tgt), 1), np.float32))], cfg, lim)
    fused = []
    orig = blocks.ResnetBottleneckBlock._forward_fused

    def spy(self, *a, **kw):
        r = orig(self, *a, **kw)
        fused.append(r is not None)
        return r

    blocks.ResnetBottleneckBlock._forward_fused = spy
    try:
        feats, ov, sal = model(batch)
    finally:
        blocks.ResnetBottleneckBlock._forward_fused = orig
    n_blocks = sum(isinstance(m, blocks.ResnetBottleneckBlock) for m in model.modules())
    print(f"{len(fused)} of {n_blocks} residual blocks took the one-call route")
    assert blocks.FUSED_BLOCK and fused and all(fused), "a K = 7 residual block left the one-call route"
    e = rel_l2(feats.cpu(), ref[0]), float((ov.cpu() - ref[1]).abs().max()), float((sal.cpu() - ref[2]).abs().max())
    print("KPFCNN K = 7 vs oracle (feats rel L2, overlap, saliency max abs):", e)
    assert e[0] < 1e-4 and e[1] < 1e-4 and e[2] < 1e-4
    # the one-call block (apr_kp_resnet_block with n_kp = 7 -> apr_kpconv_weighted_nk) against one library call per op, as
    # tests/test_predator_gpu.py::test_fused_resnet_block_call_equals_the_modular_path holds the two at K = 15: the block's
    # Linear + InstanceNorm pairs group their fp64 partial sums by GEMM tile, so the paths agree to the last bits (2e-5)
    blocks.FUSED_BLOCK = False
    try:
        plain = model(batch)
    finally:
        blocks.FUSED_BLOCK = True
    for a, b in zip((feats, ov, sal), plain):
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 2e-5
    again = model(batch)
    assert all(torch.equal(a, b) for a, b in zip((feats, ov, sal), again)), "two runs, other bits"


def test_resnet_block_k7_one_call_equals_its_kernels(dev):
    """apr_kp_resnet_block with n_kp = 7 and kpconv_route 0 on one level (in_dim = out_dim = 256, mid = 64: unary1, no shortcut
    Linear) against the same kernels called module by module -- unary1, apr_kpconv_weighted_nk + the dense GEMM with its
    norm, unary2 with the shortcut: the same launches on the same inputs, so the same bits."""
    import ctypes as C
    lib = _lib.load()
    c = NC.CASES["k7-c64-H5-nq70"]
    nq, ns, H, cin, K = c["nq"], c["ns"], c["H"], c["cin"], c["n_kp"]
    rng = np.random.default_rng(3)
    n = ns      # a same-level block maps n rows to n rows: queries = supports
    s = _t(c["s"], dev)
    nbr = _t(np.where(NO.O.real_mask(c["nbr"], ns), c["nbr"], ns)[np.arange(n) % nq].astype(np.int32), dev)
    x = _t(np.abs(rng.standard_normal((n, 256))).astype(np.float32), dev)
    mk = lambda ci, co: kp_ops.pack_linear(_t((rng.standard_normal((ci, co)) / np.sqrt(ci)).astype(np.float32), dev))
    w1, wk, w2 = mk(256, 64), mk(K * 64, 64), mk(64, 256)
    assert w1[5] is not None and wk[5] is not None and w2[5] is not None
    kp = _t(c["kp"], dev)
    out = torch.full((n, 256), NAN, dtype=torch.float32, device=dev)
    d = _lib.KpResnetDesc()
    d.x, d.ldx, d.n_in = x.data_ptr(), 256, n
    d.in_dim, d.mid, d.out_dim, d.strided = 256, 64, 256, 0
    d.q_pts, d.s_pts, d.n_out = s.data_ptr(), s.data_ptr(), n
    d.nbr, d.H, d.n_kp = nbr.data_ptr(), H, K
    d.kernel_points, d.extent, d.eps, d.slope, d.nseg = kp.data_ptr(), c["extent"], 1e-5, 0.1, 1
    d.w_unary1, d.w_kpconv, d.w_unary2, d.w_shortcut = w1[5].data_ptr(), wk[5].data_ptr(), w2[5].data_ptr(), None
    d.out, d.ldo, d.kpconv_route = out.data_ptr(), 256, 0
    sb = int(lib.apr_kp_resnet_scratch_bytes(C.byref(d)))
    scratch = torch.zeros(sb, dtype=torch.uint8, device=dev)
    d.scratch, d.scratch_bytes = scratch.data_ptr(), sb
    _lib.check(lib.apr_kp_resnet_block(C.byref(d), _lib.stream()))
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and got.any()
    # module by module with the same kernels: unary1 -> KPConv (apr_kpconv_weighted_nk + GEMM) -> norm -> unary2 + shortcut
    u1 = kp_ops.linear_norm_act(x, w1, leaky=0.1)
    wf = kp_ops.kpconv_weighted(s, s, nbr, u1, kp, c["extent"])
    y = kp_ops.linear_norm_act(wf, wk, leaky=0.1)
    ref = kp_ops.linear_norm_act(y, w2, leaky=0.1, residual=x)
    assert torch.equal(out, ref), "apr_kp_resnet_block at n_kp = 7: other bits than the module-by-module kernels"


def test_one_training_iteration_at_k7_is_finite_and_repeats_bit_for_bit(dev):
    from apr_amd.predator.lib.trainer import PredatorPairTrainStep
    from apr_amd.predator.models.architectures import KPFCNN
    from apr_amd.predator.models.mlp import GenerativeMLP_98
    from oracle import predator_points_oracle as PREF
    from tests.predator_loss_fixture import collated, small_pair, train_config
    if not PREF.available():
        pytest.skip("oracle/_ref not built")
    pair = small_pair()
    runs = []
    for _ in range(2):
        np.random.seed(7)
        torch.manual_seed(7)
        cfg = train_config()
        cfg.update(num_kernel_points=7)
        model = KPFCNN(cfg).to(dev)
        gen = GenerativeMLP_98(in_channel=cfg.final_feats_dim, out_points=cfg.point_generation_ratio, radius=None,
                               bn_momentum=cfg.batch_norm_momentum).to(dev)
        opt = torch.optim.SGD([{"params": model.parameters()}, {"params": gen.parameters()}], lr=0.01, momentum=0.98,
                              weight_decay=1e-6)
        step = PredatorPairTrainStep(model, gen, opt, cfg)
        batch = collated(pair, cfg, [30, 30, 30, 30], dev)
        grads = []
        hooks = [p.register_hook(lambda g: grads.append(g.detach().clone())) for p in model.parameters() if p.requires_grad]
        np.random.seed(5)
        stats = step(batch)[0]
        for h in hooks:
            h.remove()
        runs.append((stats, grads, [p.detach().clone() for p in model.parameters()]))
    stats, grads, _ = runs[0]
    assert all(np.isfinite(float(v)) for v in stats.values()), stats
    assert len(grads) > 50 and all(torch.isfinite(g).all() for g in grads) and any(g.abs().max() > 0 for g in grads)
    for k in stats:
        assert float(stats[k]) == float(runs[1][0][k]), k
    assert all(torch.equal(a, b) for a, b in zip(grads, runs[1][1])) and all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))


def test_print_worst_ratios():
    table = {}
    for (key, mode), v in sorted(WORST.items()):
        table.setdefault(key, {})[mode] = round(v, 4)
    for key, row in table.items():
        print(f"worst |kernel - oracle| / bound, {key}: {row}")
