"""Every entry point of apr_amd/csrc/norm.hip on the GPU, element by element against the float64 oracle (tests/norm_oracle.py)
on the named cases of tests/norm_cases.py: apr_bn_stats, apr_col_sums, apr_norm_params, apr_instance_norm_act[_seg],
apr_affine_act, apr_act_backward, apr_l2_normalize[_backward], apr_norm_backward, apr_bn_train_fwd / _bwd.  The thresholds are
the oracle's derived bounds (ratio 1) and exact equality where the oracle says exact; no element is excluded and there is no
whole-tensor norm.  Every tensor lives in a NaN-filled buffer at the case's leading dimension and base offset, and every
element outside an output's slice must still be NaN afterwards.  tests/test_norm_oracle_cpu.py shows on the host that the
cases reach their edges, that a float32 restatement of the kernels stays inside the bounds and that one-rule mutants do not.

Bit equality of the segmented launch with one call per segment is asserted where the order of every sum is the same by
construction (outputs, saved statistics, running statistics, dx, dres); dgamma / dbeta are NOT: the segmented launch adds
the segments' fp64 sums and rounds once, separate calls round per segment.

Worst |kernel - oracle| / bound measured on the MI355X over all cases (records, not thresholds; printed by
test_zz_print_worst_ratios; DESIGN 24 has the table):  y_bn 0.868,  y_in 0.811,  dx 0.692,  dgamma 0.584,  running 0.474,
saved rstd 0.513,  scale / shift 0.479 / 0.520,  affine 0.673,  L2 y / dx 0.243 / 0.216;  the quantities that are one
float32 rounding of an fp64 sum (mean, var, column sums, dbeta, dy * slope) sit at 0.95 .. 1.00 by nature.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import norm_cases as K
import norm_oracle as O
from apr_amd import _lib, ops
from apr_amd.predator import kp_ops

pytestmark = pytest.mark.gpu
NAN = float("nan")
HEAD, TAIL = 4, 8               # guard floats in front of and behind every buffer (HEAD keeps the 16-byte alignment)
WORST = {}
RSTD_CLAMPED = np.float32(1) / np.sqrt(np.float32(K.EPS))       # what a variance clamped to 0 gives, bit for bit
ptr, check, stream = _lib.ptr, _lib.check, _lib.stream


class Buf:
    """[n, c] values at leading dimension c + extra, `off` floats into a NaN-filled flat buffer"""

    def __init__(self, dev, n, c, layout=(0, 0), values=None):
        extra, off = layout
        self.n, self.c, self.ld = n, c, c + extra
        self.flat = torch.full((HEAD + off + n * self.ld + TAIL,), NAN, dtype=torch.float32, device=dev)
        assert self.flat.data_ptr() % 16 == 0
        self.view = torch.as_strided(self.flat, (n, c), (self.ld, 1), HEAD + off)
        inside = torch.zeros_like(self.flat, dtype=torch.bool)
        torch.as_strided(inside, (n, c), (self.ld, 1), HEAD + off).fill_(True)
        self.outside = ~inside
        if values is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32)).to(dev))

    @property
    def p(self):
        return ptr(self.view)

    def get(self):
        """the slice as numpy, after checking that nothing outside it was written"""
        assert bool(torch.isnan(self.flat[self.outside]).all()), "an element outside the slice was written"
        return self.view.cpu().numpy()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _nanvec(dev, *shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=dev)


def _scratch(dev, nbytes):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def _offs(offs, force=False):
    """(ctypes int64 array or None, nseg) as the entry points take them; force: an offsets array even for one segment"""
    if len(offs) <= 2 and not force:
        return None, 0
    return (C.c_int64 * len(offs))(*offs), len(offs) - 1


def _same(a, b):
    return a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------- direct callers
def run_stats(dev, case):
    lib = _lib.load()
    n, c = case["n"], case["c"]
    x = Buf(dev, n, c, K.lay(case, "x"), case["x"])
    sb = int(lib.apr_bn_stats_scratch_bytes(n, c))
    scratch = _scratch(dev, sb)
    mean, var, sums, scale, shift = (_nanvec(dev, c) for _ in range(5))
    check(lib.apr_bn_stats(x.p, x.ld, n, c, ptr(mean), ptr(var), ptr(scratch), sb, stream()))
    check(lib.apr_col_sums(x.p, x.ld, n, c, ptr(sums), ptr(scratch), sb, stream()))
    check(lib.apr_norm_params(x.p, x.ld, n, c, case["eps"], ptr(scale), ptr(shift), ptr(scratch), sb, stream()))
    return {"mean": mean.cpu().numpy(), "var": var.cpu().numpy(), "colsum": sums.cpu().numpy(), "scale": scale.cpu().numpy(),
            "shift": shift.cpu().numpy()}


def run_inst(dev, case, mode, with_res, offs, rows=None, force_seg=False):
    """apr_instance_norm_act_seg (more than one segment, or force_seg) or apr_instance_norm_act over the rows
    [rows[0], rows[1])"""
    lib = _lib.load()
    a, e = rows or (0, case["n"])
    n, c = e - a, case["c"]
    x = Buf(dev, n, c, K.lay(case, "x"), case["x"][a:e])
    res = Buf(dev, n, c, K.lay(case, "res"), case["res_in"][a:e]) if with_res else None
    y = Buf(dev, n, c, K.lay(case, "y"))
    arr, nseg = _offs(offs, force_seg)
    sb = int(lib.apr_bn_stats_scratch_bytes(n + 256 * max(nseg, 1), c))
    scratch = _scratch(dev, sb)
    rp, ldr = (res.p, res.ld) if with_res else (None, 0)
    if nseg:
        check(lib.apr_instance_norm_act_seg(x.p, x.ld, n, c, case["eps"], rp, ldr, mode, case["slope"], y.p, y.ld, arr, nseg,
                                            ptr(scratch), sb, stream()))
    else:
        check(lib.apr_instance_norm_act(x.p, x.ld, n, c, case["eps"], rp, ldr, mode, case["slope"], y.p, y.ld, ptr(scratch), sb,
                                        stream()))
    return {"y_in": y.get()}


def run_bn_fwd(dev, case, relu, with_res, offs=None, rows=None, state=None, force_seg=False):
    """apr_bn_train_fwd over the case's segments (or one call over `rows`, carrying the running `state` along)"""
    lib = _lib.load()
    offs = case["offs"] if offs is None else offs
    a, e = rows or (0, case["n"])
    n, c = e - a, case["c"]
    z = Buf(dev, n, c, K.lay(case, "x"), case["x"][a:e])
    res = Buf(dev, n, c, K.lay(case, "res"), case["res"][a:e]) if with_res else None
    y = Buf(dev, n, c, K.lay(case, "y"))
    arr, nseg = _offs(offs, force_seg)
    ns = max(nseg, 1)
    if state is None:
        state = (_t(case["rm"], dev), _t(case["rv"], dev), torch.tensor([case["count"]], dtype=torch.int64, device=dev))
    rm, rv, cnt = state
    sm, sr = _nanvec(dev, ns, c), _nanvec(dev, ns, c)
    sb = int(lib.apr_bn_stats_scratch_bytes(n + 256 * ns, c))
    scratch = _scratch(dev, sb)
    rp, ldr = (res.p, res.ld) if with_res else (None, 0)
    gamma, beta = _t(case["gamma"], dev), _t(case["beta"], dev)
    check(lib.apr_bn_train_fwd(z.p, z.ld, n, c, ptr(gamma), ptr(beta), case["eps"],
                               case["momentum"], ptr(rm), ptr(rv), rp, ldr, int(relu), y.p, y.ld, ptr(sm), ptr(sr), ptr(cnt), arr,
                               nseg, ptr(scratch), sb, stream()))
    return {"y_bn": y.get(), "save_mean": sm.cpu().numpy(), "save_rstd": sr.cpu().numpy(), "run_mean": rm.cpu().numpy(),
            "run_var": rv.cpu().numpy(), "count": int(cnt.item()), "state": state}


def run_bn_bwd(dev, case, relu, want_dres, y, mean, rstd, offs=None, rows=None, force_seg=False):
    lib = _lib.load()
    offs = case["offs"] if offs is None else offs
    a, e = rows or (0, case["n"])
    n, c = e - a, case["c"]
    z = Buf(dev, n, c, K.lay(case, "x"), case["x"][a:e])
    dy = Buf(dev, n, c, K.lay(case, "dy"), case["dy"][a:e])
    yb = Buf(dev, n, c, K.lay(case, "yb"), y[a:e]) if relu else None
    dx = Buf(dev, n, c, K.lay(case, "dx"))
    dres = Buf(dev, n, c, K.lay(case, "dres")) if want_dres else None
    dg, db = _nanvec(dev, c), _nanvec(dev, c)
    arr, nseg = _offs(offs, force_seg)
    sb = int(lib.apr_bn_stats_scratch_bytes(n + 256 * max(nseg, 1), c))
    scratch = _scratch(dev, sb)
    mean, rstd, gamma = _t(mean, dev), _t(rstd, dev), _t(case["gamma"], dev)
    check(lib.apr_bn_train_bwd(z.p, z.ld, yb.p if relu else None, yb.ld if relu else 0, dy.p, dy.ld, n, c, ptr(mean),
                               ptr(rstd), ptr(gamma), int(relu), dx.p, dx.ld,
                               dres.p if want_dres else None, dres.ld if want_dres else 0, ptr(dg), ptr(db), arr, nseg,
                               ptr(scratch), sb, stream()))
    out = {"dx": dx.get(), "dgamma": dg.cpu().numpy(), "dbeta": db.cpu().numpy()}
    if want_dres:
        out["dres"] = dres.get()
    return out


def run_norm_bwd(dev, case, with_gamma, mean, rstd):
    lib = _lib.load()
    n, c = case["n"], case["c"]
    x = Buf(dev, n, c, K.lay(case, "x"), case["x"])
    dy = Buf(dev, n, c, K.lay(case, "dy"), case["dy"])
    dx = Buf(dev, n, c, K.lay(case, "dx"))
    dg, db = (_nanvec(dev, c), _nanvec(dev, c)) if with_gamma else (None, None)
    sb = int(lib.apr_norm_backward_scratch_bytes(n, c))
    scratch = _scratch(dev, sb)
    mean, rstd, gamma = _t(mean[0], dev), _t(rstd[0], dev), _t(case["gamma"], dev)
    check(lib.apr_norm_backward(x.p, x.ld, dy.p, dy.ld, n, c, ptr(mean), ptr(rstd),
                                ptr(gamma) if with_gamma else None, dx.p, dx.ld, ptr(dg), ptr(db), ptr(scratch),
                                sb, stream()))
    out = {"dx": dx.get()}
    if with_gamma:
        out["dgamma"], out["dbeta"] = dg.cpu().numpy(), db.cpu().numpy()
    return out


def run_act_in(dev, case, y):
    """apr_act_backward, LeakyReLU, on the instance norm's own output"""
    lib = _lib.load()
    n, c = case["n"], case["c"]
    dy = Buf(dev, n, c, K.lay(case, "dy"), case["dy"])
    yb = Buf(dev, n, c, K.lay(case, "yb"), y)
    dz = Buf(dev, n, c, K.lay(case, "dres"))
    check(lib.apr_act_backward(dy.p, dy.ld, yb.p, yb.ld, n, c, 2, case["slope"], dz.p, dz.ld, stream()))
    return {"dz_in": dz.get()}


def run_affine(dev, case, mode, layout=(0, 0)):
    lib = _lib.load()
    n, c = case["n"], case["c"]
    x = Buf(dev, n, c, layout, case["x"])
    res = Buf(dev, n, c, layout, case["res"])
    dy = Buf(dev, n, c, layout, case["dy"])
    y, dz = Buf(dev, n, c, layout), Buf(dev, n, c, layout)
    scale, shift = _t(case["scale"], dev), _t(case["shift"], dev)
    check(lib.apr_affine_act(x.p, x.ld, n, c, ptr(scale), ptr(shift), res.p, res.ld, mode,
                             case["slope"], y.p, y.ld, stream()))
    check(lib.apr_act_backward(dy.p, dy.ld, y.p, y.ld, n, c, mode, case["slope"], dz.p, dz.ld, stream()))
    return {"y_aff": y.get(), "dz": dz.get()}


def run_l2(dev, case):
    lib = _lib.load()
    n, c = case["n"], case["c"]
    lay = K.LAYOUTS[case["layout"]]
    x = Buf(dev, n, c, lay.get("x", (0, 0)), case["x"])
    dy = Buf(dev, n, c, lay.get("dy", (0, 0)), case["dy"])
    y, dx = Buf(dev, n, c, lay.get("y", (0, 0))), Buf(dev, n, c, lay.get("dx", (0, 0)))
    check(lib.apr_l2_normalize(x.p, x.ld, n, c, y.p, y.ld, stream()))
    check(lib.apr_l2_normalize_backward(x.p, x.ld, dy.p, dy.ld, n, c, dx.p, dx.ld, stream()))
    return y.get(), dx.get()


def _segments(case):
    return list(zip(case["offs"][:-1], case["offs"][1:]))


# ------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("name", list(K.NORM))
def test_stats_col_sums_and_norm_params(dev, name):
    case = K.NORM[name]
    got = run_stats(dev, case)
    K.check(name, got, K.expect_stats(case), WORST)
    if case["negvar"]:
        # the one-pass variance of column 5 is negative in the kernel's order: the clamp stores 0 and rstd = 1 / sqrt(eps)
        assert got["var"][5] == 0 and _same(got["scale"][5], RSTD_CLAMPED)
    again = run_stats(dev, case)
    assert all(_same(got[k], again[k]) for k in got), "a second run gave other bits"


@pytest.mark.parametrize("name", list(K.NORM))
def test_instance_norm_every_element(dev, name):
    case = K.NORM[name]
    got = run_inst(dev, case, 2, True, case["offs"])
    K.check(name, got, K.expect_inst(case, 2, True), WORST)
    assert _same(got["y_in"], run_inst(dev, case, 2, True, case["offs"])["y_in"]), "a second run gave other bits"
    if case["special"]:
        assert (got["y_in"][case["zero_in"]] == 0).all()                      # the planted y == 0
    dz = run_act_in(dev, case, got["y_in"])
    K.check(name, dz, K.expect_act_in(case), WORST)
    if case["special"]:                                                       # y == 0 takes the slope
        assert _same(dz["dz_in"][case["zero_in"]], (case["dy"][case["zero_in"]] * np.float32(case["slope"])).astype(np.float32))
    if len(case["offs"]) == 2 and case["n"] <= 3000:
        # one segment through the segmented entry (nseg = 1): the bits of the plain entry
        assert _same(got["y_in"], run_inst(dev, case, 2, True, case["offs"], force_seg=True)["y_in"])
    K.check(name, run_inst(dev, case, 1, True, case["offs"]), K.expect_inst(case, 1, True), WORST)
    K.check(name, run_inst(dev, case, 0, False, O.one(case["n"])), K.expect_inst(case, 0, False, False), WORST)
    if len(case["offs"]) > 2 and case["n"] <= 3000:
        # one call per segment: the same block partials in the same order, so the same bits
        for a, e in _segments(case):
            part = run_inst(dev, case, 2, True, O.one(e - a), rows=(a, e))["y_in"]
            assert _same(part, got["y_in"][a:e]), (name, "segment", a, e)
            part = run_inst(dev, case, 2, True, O.one(e - a), rows=(a, e), force_seg=True)["y_in"]
            assert _same(part, got["y_in"][a:e]), (name, "segment through the segmented entry", a, e)


@pytest.mark.parametrize("name", list(K.BN))
def test_bn_train_forward_every_element(dev, name):
    case = K.BN[name]
    got = run_bn_fwd(dev, case, True, True)
    e = K.expect_bn_fwd(case, True, True)
    K.check(name, got, e, WORST)
    if case["negvar"]:
        assert _same(got["save_rstd"][0, 5], RSTD_CLAMPED)                    # the clamp, as in apr_bn_stats
    again = run_bn_fwd(dev, case, True, True)
    assert all(_same(got[k], again[k]) for k in ("y_bn", "save_mean", "save_rstd", "run_mean", "run_var")) and got["count"] == again["count"]
    if case["special"]:
        # the constant column: (z - mean) is exactly 0, the output is beta + res bit for bit (0 at the planted rows)
        want = np.maximum((case["beta"][1] + case["res"][:, 1]).astype(np.float32), np.float32(0))
        assert _same(got["y_bn"][:, 1], want)
        assert (got["y_bn"][case["zero_bn"]] == 0).all()
    K.check(name, run_bn_fwd(dev, case, False, False), K.expect_bn_fwd(case, False, False), WORST)
    if len(case["offs"]) > 2 and case["n"] <= 3000:
        # one call per segment, the running statistics carried from call to call: the same bits
        state = None
        for s, (a, b) in enumerate(_segments(case)):
            # every other call hands over an offsets array with nseg = 1 (make_segs' one-segment branch)
            part = run_bn_fwd(dev, case, True, True, offs=O.one(b - a), rows=(a, b), state=state, force_seg=bool(s % 2))
            state = part["state"]
            assert _same(part["y_bn"], got["y_bn"][a:b]) and _same(part["save_mean"][0], got["save_mean"][s])
            assert _same(part["save_rstd"][0], got["save_rstd"][s])
        assert _same(part["run_mean"], got["run_mean"]) and _same(part["run_var"], got["run_var"]) and part["count"] == got["count"]


@pytest.mark.parametrize("name", list(K.BN))
def test_bn_train_backward_every_element(dev, name):
    case = K.BN[name]
    mean, rstd = K.given_stats(case)
    for relu in (True, False):
        e = K.expect_bn_bwd(case, relu)
        got = run_bn_bwd(dev, case, relu, relu, e["y"], mean, rstd)
        K.check(name, got, e, WORST, absent=() if relu else ("dres",))
        if relu:
            again = run_bn_bwd(dev, case, relu, relu, e["y"], mean, rstd)
            assert all(_same(got[k], again[k]) for k in got), "a second run gave other bits"
            if case["special"]:
                assert (got["dres"][case["zero_bn"]] == 0).all() and (case["dy"][case["zero_bn"]] != 0).all()
                assert (got["dres"][:, 1][e["y"][:, 1] <= 0] == 0).all()
            if len(case["offs"]) > 2 and case["n"] <= 3000:
                for s, (a, b) in enumerate(_segments(case)):
                    part = run_bn_bwd(dev, case, True, True, e["y"], mean[s:s + 1], rstd[s:s + 1], offs=O.one(b - a), rows=(a, b),
                                      force_seg=bool(s % 2))
                    assert _same(part["dx"], got["dx"][a:b]) and _same(part["dres"], got["dres"][a:b]), (name, "segment", s)


@pytest.mark.parametrize("name", list(K.NORM))
def test_norm_backward_every_element(dev, name):
    case = K.NORM[name]
    for with_gamma in (False, True):
        e = K.expect_norm_bwd(case, with_gamma)
        got = run_norm_bwd(dev, case, with_gamma, e["mean"], e["rstd"])
        K.check(name, got, e, WORST, absent=() if with_gamma else ("dgamma", "dbeta"))
    again = run_norm_bwd(dev, case, True, e["mean"], e["rstd"])
    assert all(_same(got[k], again[k]) for k in got), "a second run gave other bits"


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", K.STRIDE_NAMES)
def test_affine_act_and_act_backward_past_one_sweep(dev, name, mode):
    case = K.stride_case(name)
    got = run_affine(dev, case, mode)
    K.check(name, got, K.expect_affine(case, mode), WORST)
    flat_y, flat_dz, flat_dy = got["y_aff"].reshape(-1), got["dz"].reshape(-1), case["dy"].reshape(-1)
    for t in case["planted"]:                       # the first element of the second sweep and the last: y == 0 exactly
        assert flat_y[t] == 0 and flat_dz[t] == (np.float32(flat_dy[t]) * np.float32(case["slope"]) if mode == 2 else 0)


@pytest.mark.parametrize("layout", [(0, 0), (1, 0), (4, 1)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_affine_act_and_act_backward_small(dev, mode, layout):
    """41 x 5 at ld = c, c + 1 and c + 4 with the base 4 bytes off: every mode, the planted y == 0 in the middle and last"""
    case = K._memo(("affine-small",), lambda: K.build_stride("affine-small", 41 * 5, 5, 74))
    got = run_affine(dev, case, mode, layout)
    K.check(case["name"], got, K.expect_affine(case, mode), WORST)
    assert mode == 0 or all(got["y_aff"].reshape(-1)[t] == 0 for t in case["planted"])


@pytest.mark.parametrize("name", list(K.L2))
def test_l2_rows_every_element_and_special_rows_in_kind(dev, name):
    case = K.L2[name]
    y, dx = run_l2(dev, case)
    ry, rd = K.check_l2(case, y, dx)
    WORST["y_l2"], WORST["dx_l2"] = max(WORST.get("y_l2", 0.0), ry), max(WORST.get("dx_l2", 0.0), rd)
    y2, dx2 = run_l2(dev, case)
    assert _same(y, y2) and _same(dx, dx2)


def test_refusals_raise(dev):
    """bad arguments only: every call returns before a launch"""
    lib = _lib.load()
    n, c = 20, 8
    x = Buf(dev, n, c, (0, 0), np.ones((n, c), np.float32))
    y = Buf(dev, n, c)
    v = [_nanvec(dev, 4, c) for _ in range(6)]
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    big = int(lib.apr_bn_stats_scratch_bytes(n + 256 * 40, c))
    scratch = _scratch(dev, big)
    one = int(lib.apr_bn_stats_scratch_bytes(n, c))

    def inst_seg(offs, nn=n, sb=big, eps=1e-5, ldx=c):
        arr, nseg = (C.c_int64 * len(offs))(*offs), len(offs) - 1
        return lib.apr_instance_norm_act_seg(x.p, ldx, nn, c, eps, None, 0, 0, 0.0, y.p, c, arr, nseg, ptr(scratch), sb, stream())

    def bn_fwd(offs=None, nn=n, sb=big, eps=1e-5, ldz=c, ldy=c):
        arr, nseg = ((C.c_int64 * len(offs))(*offs), len(offs) - 1) if offs else (None, 0)
        return lib.apr_bn_train_fwd(x.p, ldz, nn, c, None, None, eps, 0.1, ptr(v[0]), ptr(v[1]), None, 0, 0, y.p, ldy, ptr(v[2]),
                                    ptr(v[3]), ptr(cnt), arr, nseg, ptr(scratch), sb, stream())

    def bn_bwd(offs=None, nn=n, sb=big, lddx=c):
        arr, nseg = ((C.c_int64 * len(offs))(*offs), len(offs) - 1) if offs else (None, 0)
        return lib.apr_bn_train_bwd(x.p, c, None, 0, x.p, c, nn, c, ptr(v[2]), ptr(v[3]), None, 0, y.p, lddx, None, 0, ptr(v[4]),
                                    ptr(v[5]), arr, nseg, ptr(scratch), sb, stream())

    calls = {}
    for what, offs in K.REFUSED_OFFSETS.items():
        nn = offs[-1] if what != "offsets not ending at n" else offs[-1] + 1
        calls[f"inst_seg: {what}"] = lambda offs=offs, nn=nn: inst_seg(offs, nn)
        calls[f"bn_fwd: {what}"] = lambda offs=offs, nn=nn: bn_fwd(offs, nn)
        calls[f"bn_bwd: {what}"] = lambda offs=offs, nn=nn: bn_bwd(offs, nn)
    calls["bn_fwd: a 1-row segment"] = lambda: bn_fwd([0, 10, 11, 20])
    calls["bn_bwd: a 1-row segment"] = lambda: bn_bwd([0, 10, 11, 20])
    calls["bn_fwd: n = 1"] = lambda: bn_fwd(None, 1)
    calls["bn_fwd: ldz < c"] = lambda: bn_fwd(ldz=c - 1)
    calls["bn_fwd: ldy < c"] = lambda: bn_fwd(ldy=c - 1)
    calls["bn_bwd: lddx < c"] = lambda: bn_bwd(lddx=c - 1)
    calls["bn_fwd: eps < 0"] = lambda: bn_fwd(eps=-1e-5)
    calls["bn_fwd: scratch one byte short"] = lambda: bn_fwd(sb=int(lib.apr_bn_stats_scratch_bytes(n + 256, c)) - 1)
    calls["bn_bwd: scratch one byte short"] = lambda: bn_bwd(sb=int(lib.apr_bn_stats_scratch_bytes(n + 256, c)) - 1)
    calls["inst_seg: ldx < c"] = lambda: inst_seg([0, 10, n], ldx=c - 1)
    calls["inst_seg: eps < 0"] = lambda: inst_seg([0, 10, n], eps=-1e-5)
    calls["inst_seg: scratch one byte short"] = lambda: inst_seg([0, 10, n], sb=int(lib.apr_bn_stats_scratch_bytes(n + 512, c)) - 1)
    calls["inst: ldy < c"] = lambda: lib.apr_instance_norm_act(x.p, c, n, c, 1e-5, None, 0, 0, 0.0, y.p, c - 1, ptr(scratch), big, stream())
    calls["inst: ldr < c"] = lambda: lib.apr_instance_norm_act(x.p, c, n, c, 1e-5, x.p, c - 1, 0, 0.0, y.p, c, ptr(scratch), big, stream())
    calls["inst: eps < 0"] = lambda: lib.apr_instance_norm_act(x.p, c, n, c, -1e-5, None, 0, 0, 0.0, y.p, c, ptr(scratch), big, stream())
    calls["inst: scratch one byte short"] = lambda: lib.apr_instance_norm_act(x.p, c, n, c, 1e-5, None, 0, 0, 0.0, y.p, c, ptr(scratch),
                                                                               one - 1, stream())
    calls["bn_stats: ld < c"] = lambda: lib.apr_bn_stats(x.p, c - 1, n, c, ptr(v[0]), ptr(v[1]), ptr(scratch), big, stream())
    calls["bn_stats: scratch one byte short"] = lambda: lib.apr_bn_stats(x.p, c, n, c, ptr(v[0]), ptr(v[1]), ptr(scratch), one - 1, stream())
    calls["col_sums: ld < c"] = lambda: lib.apr_col_sums(x.p, c - 1, n, c, ptr(v[0]), ptr(scratch), big, stream())
    calls["col_sums: scratch one byte short"] = lambda: lib.apr_col_sums(x.p, c, n, c, ptr(v[0]), ptr(scratch), one - 1, stream())
    calls["norm_params: eps < 0"] = lambda: lib.apr_norm_params(x.p, c, n, c, -1e-5, ptr(v[0]), ptr(v[1]), ptr(scratch), big, stream())
    calls["norm_params: ld < c"] = lambda: lib.apr_norm_params(x.p, c - 1, n, c, 1e-5, ptr(v[0]), ptr(v[1]), ptr(scratch), big, stream())
    calls["norm_params: scratch one byte short"] = lambda: lib.apr_norm_params(x.p, c, n, c, 1e-5, ptr(v[0]), ptr(v[1]), ptr(scratch),
                                                                               one - 1, stream())
    nb = int(lib.apr_norm_backward_scratch_bytes(n, c))
    calls["norm_backward: lddx < c"] = lambda: lib.apr_norm_backward(x.p, c, x.p, c, n, c, ptr(v[0]), ptr(v[1]), None, y.p, c - 1, None,
                                                                     None, ptr(scratch), big, stream())
    calls["norm_backward: scratch one byte short"] = lambda: lib.apr_norm_backward(x.p, c, x.p, c, n, c, ptr(v[0]), ptr(v[1]), None, y.p, c,
                                                                                   None, None, ptr(scratch), nb - 1, stream())
    calls["affine_act: ldy < c"] = lambda: lib.apr_affine_act(x.p, c, n, c, None, None, None, 0, 0, 0.0, y.p, c - 1, stream())
    calls["act_backward: lddz < c"] = lambda: lib.apr_act_backward(x.p, c, x.p, c, n, c, 1, 0.0, y.p, c - 1, stream())
    calls["act_backward: mode 3"] = lambda: lib.apr_act_backward(x.p, c, x.p, c, n, c, 3, 0.0, y.p, c, stream())
    calls["l2_normalize: ldy < c"] = lambda: lib.apr_l2_normalize(x.p, c, n, c, y.p, c - 1, stream())
    calls["l2_normalize_backward: lddx < c"] = lambda: lib.apr_l2_normalize_backward(x.p, c, x.p, c, n, c, y.p, c - 1, stream())
    assert len(calls) == 39
    for what, call in calls.items():
        with pytest.raises(_lib.AprHipError):
            check(call())
            pytest.fail(f"{what}: accepted")
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.flat).all()) and all(bool(torch.isnan(t).all()) for t in v) and int(cnt.item()) == 0, "a refused call wrote"


# ---------------------------------------------------------------------------- end to end through the autograd nodes
def _grad_bounds(case, offs, g, gamma, chain):
    """the backward's bounds when the kernel uses the statistics of its OWN forward: dm / Rr are the forward's bounds"""
    b = O.stat_bounds(case["x"], offs, case["eps"])
    dx, dg, db = O.norm_backward(case["x"], g, offs, b["mean"], b["rstd"], gamma)
    bdx, bdg, bdb = O.bound_norm_backward(case["x"], g, offs, b["mean"], b["rstd"], gamma, dm=b["bm"], Rr=b["R"], chain=chain)
    return {"dx": (dx, bdx), "dgamma": (dg, bdg), "dbeta": (db, bdb)}


@pytest.mark.parametrize("name,leaky,relu", [("n256-c60", None, True), ("seg-ragged", 0.1, False), ("seg-2-700", 0.1, False),
                                             ("n257-c63", None, False)])
def test_norm_act_function_gradients(dev, name, leaky, relu):
    """kp_ops.NormActFunction: odd width, ragged segments, the planted y == 0 (n256-c60 under ReLU)"""
    case = K.NORM[name]
    mode = 2 if leaky is not None else int(relu)
    x = _t(case["x"], dev).requires_grad_(True)
    res = _t(case["res_in"], dev).requires_grad_(True)
    segs = case["offs"] if len(case["offs"]) > 2 else None
    y = kp_ops.NormActFunction.apply(x, res, case["eps"], leaky, relu, segs)
    y.backward(_t(case["dy"], dev))
    e = K.expect_inst(case, mode, True)
    K.check(name, {"y_in": y.detach().cpu().numpy()}, e, WORST)
    g = O.act_backward(case["dy"], e["y_in"][0], mode, case["slope"])
    want = _grad_bounds(case, case["offs"], g, None, True)
    K.check(name, {"dx": x.grad.cpu().numpy()}, {"dx": want["dx"]}, WORST)
    K.check(name, {"dres": res.grad.cpu().numpy()}, {"dres": (g, O.bound_act_backward(case["dy"], e["y_in"][0], mode, case["slope"]))}, WORST)
    if case["special"] and mode:
        assert (y.detach().cpu().numpy()[case["zero_in"]] == 0).all()


@pytest.mark.parametrize("name", ["n257-c63", "n256-c60", "n3-c3"])
def test_norm_function_gradients(dev, name):
    """ops.NormFunction (subtract-first apply through apr_affine_act, apr_norm_backward)"""
    case = K.NORM[name]
    x = _t(case["x"], dev).requires_grad_(True)
    w = _t(case["gamma"], dev).requires_grad_(True)
    b = _t(case["beta"], dev).requires_grad_(True)
    y, mean, var = ops.NormFunction.apply(x, w, b, case["eps"])
    y.backward(_t(case["dy"], dev))
    offs = O.one(case["n"])
    st = K.expect_stats(case)
    K.check(name, {"mean": mean.cpu().numpy(), "var": var.cpu().numpy()}, {"mean": st["mean"], "var": st["var"]}, WORST)
    K.check(name, {"y_bn": y.detach().cpu().numpy()},
            {"y_bn": (O.norm_act(case["x"], offs, case["eps"], case["gamma"], case["beta"]),
                      O.bound_norm_act(case["x"], offs, case["eps"], case["gamma"], case["beta"], form="subtract"))}, WORST)
    want = _grad_bounds(case, offs, case["dy"], case["gamma"], True)
    K.check(name, {"dx": x.grad.cpu().numpy(), "dgamma": w.grad.cpu().numpy(), "dbeta": b.grad.cpu().numpy()}, want, WORST)


@pytest.mark.parametrize("name", ["seg-ragged", "n257-c63", "seg-2-700"])
def test_bn_train_function_gradients(dev, name):
    """ops.BnTrainFunction: the batch norm alone (no residual, no ReLU) per segment, running statistics updated"""
    case = K.NORM[name]
    c = case["c"]
    bn = torch.nn.BatchNorm1d(c, eps=case["eps"], momentum=case["momentum"]).to(dev)
    with torch.no_grad():
        bn.weight.copy_(_t(case["gamma"], dev))
        bn.bias.copy_(_t(case["beta"], dev))
        bn.running_mean.copy_(_t(case["rm"], dev))
        bn.running_var.copy_(_t(case["rv"], dev))
        bn.num_batches_tracked.fill_(case["count"])
    x = _t(case["x"], dev).requires_grad_(True)
    segs = case["offs"] if len(case["offs"]) > 2 else None
    y = ops.BnTrainFunction.apply(x, bn.weight, bn.bias, bn, segs)
    y.backward(_t(case["dy"], dev))
    e = K.expect_bn_fwd(case, False, False)
    K.check(name, {"y_bn": y.detach().cpu().numpy(), "run_mean": bn.running_mean.cpu().numpy(), "run_var": bn.running_var.cpu().numpy(),
                   "count": int(bn.num_batches_tracked)}, e, WORST, absent=("save_mean", "save_rstd"))
    want = _grad_bounds(case, case["offs"], case["dy"], case["gamma"], False)
    K.check(name, {"dx": x.grad.cpu().numpy(), "dgamma": bn.weight.grad.cpu().numpy(), "dbeta": bn.bias.grad.cpu().numpy()}, want, WORST)


def test_zz_print_worst_ratios():
    print("worst kernel / bound:", {k: round(v, 3) for k, v in sorted(WORST.items())})
    assert all(v <= 1.0 for v in WORST.values())
