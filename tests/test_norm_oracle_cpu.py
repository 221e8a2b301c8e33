"""Host checks of the normalisation oracle (tests/norm_oracle.py) and its cases (tests/norm_cases.py), no GPU:
* every case plants the fact it names and is decision-safe;
* a float32 restatement of apr_amd/csrc/norm.hip in the kernels' own order of operations (fp64 block partials, the
  stride-32 combine, float32 apply, scale/shift against subtract-first) stays inside the oracle's bounds on every case; the
  worst ratio per quantity is printed;
* one-rule mutants of that restatement are each rejected by a named case, and the restatement itself is not.
Measured worst restatement ratios: DESIGN 24."""
import numpy as np
import pytest
import torch

import norm_cases as K
import norm_oracle as O

F32 = np.float32
NAN = float("nan")
WORST = {}


def _fma(a, b, c):
    """float32 fused multiply-add: the product is exact in float64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


# ------------------------------------------------------------------------------------------- the restatement
def _segs(offs, mut):
    blk0 = [0]
    for s in range(len(offs) - 1):
        blk0.append(blk0[-1] + O.cdiv(offs[s + 1] - offs[s], 256))
    if mut == "blk0_row0":
        blk0 = [o // 256 for o in offs]
    return blk0


def _partials(A, B, offs, mut, form):
    """fp64 sums of A and B per 256-row block of every segment in the partial kernel's own order of rows (K.block_sum; form:
    which kernel), stored at blk0[s] + b (scratch starts as NaN)"""
    blk0 = _segs(offs, mut)
    n, c = A.shape
    dt = np.float32 if mut == "fp32acc" else np.float64
    P = np.full((max(blk0[-1], 1) + O.cdiv(n, 256) + 2, 2, c), NAN)
    for s in range(len(offs) - 1):
        for b in range(blk0[s + 1] - blk0[s]):
            r0 = offs[s] + b * 256
            r1 = min(r0 + 256, offs[s + 1] if mut != "noclamp" else n)
            with np.errstate(over="ignore"):
                P[blk0[s] + b, 0] = K.block_sum(A[r0:r1], form, dt)
                P[blk0[s] + b, 1] = K.block_sum(B[r0:r1], form, dt)
    return P, blk0


def _combine(P, mut, chain=False):
    """[nblk, c] -> [c] in the order of k_bn_finish / k_norm_apply / column_sums (or apr_norm_backward's chain)"""
    dt = np.float32 if mut == "fp32acc" else np.float64
    nblk = len(P)
    if chain:
        s = np.zeros(P.shape[1], dt)
        for b in range(nblk):
            s = (s + P[b].astype(dt)).astype(dt)
        return s.astype(np.float64)
    grp = []
    for g in range(4):
        s = np.zeros(P.shape[1], dt)
        for b0 in range(g, nblk, 32):
            for u in range(7 if mut == "unroll7" else 8):
                b = b0 + 4 * u
                if b < nblk:
                    s = (s + P[b].astype(dt)).astype(dt)
            if mut == "stop32":
                break
        grp.append(s)
    return (((grp[0] + grp[1]).astype(dt) + grp[2]).astype(dt) + grp[3]).astype(np.float64)


def _stats(x, offs, eps, mut, form):
    """-> mf, vf, rs [nseg, c] float32 as the kernels form them (form: k_bn_partial's 16-byte or 4-byte order)"""
    xd = x.astype(np.float64)
    P, blk0 = _partials(xd, xd * xd, offs, mut, form)
    nseg = len(offs) - 1
    mf, vf, rs = (np.empty((nseg, x.shape[1]), F32) for _ in range(3))
    for s in range(nseg):
        ns = offs[s + 1] - offs[s] if mut != "total_n" else offs[-1]
        seg = P[blk0[s]:blk0[s + 1]]
        m = _combine(seg[:, 0], mut) / ns
        v = _combine(seg[:, 1], mut) / ns - m * m
        mf[s] = m.astype(F32)
        vf[s] = (np.maximum(v, 0.0) if mut != "noclamp_var" else v).astype(F32)
        with np.errstate(invalid="ignore", divide="ignore"):
            rs[s] = F32(1.0) / np.sqrt((vf[s] + F32(eps)).astype(F32))
    return mf, vf, rs


def _act32(v, mode, slope):
    if mode == 1:
        return np.maximum(v, F32(0))
    if mode == 2:
        return np.where(v > 0, v, (v * F32(slope)).astype(F32))
    return v


def _store(values, case, role, mut=None):
    """the kernel's output inside its NaN-filled buffer [n, ld] -> (slice, guard columns)"""
    n, c = values.shape
    extra = K.lay(case, role)[0]
    buf = np.full((n, c + extra), NAN, F32)
    buf[:, :c] = values
    if mut == "dead_column" and c % 4 and extra:
        buf[:, c:min((c + 3) // 4 * 4, c + extra)] = 0          # the dead columns of the last live quad
    return buf[:, :c], buf[:, c:]


def r_bn_fwd(case, relu, with_res, mut=None):
    x, offs, eps = case["x"], case["offs"], case["eps"]
    mf, vf, rs = _stats(x, offs, eps, mut, K.x_form(case["c"], case["layout"]))
    y = np.empty_like(x)
    for s in range(len(offs) - 1):
        a, e = offs[s], offs[s + 1]
        k = 0 if mut == "seg0_stats" else s
        v = _fma((x[a:e] - mf[k]).astype(F32), (rs[k] * case["gamma"]).astype(F32), case["beta"])
        if with_res:
            v = (v + case["res"][a:e]).astype(F32)
        y[a:e] = np.maximum(v, F32(0)) if relu else v
    rm, rv = case["rm"].copy(), case["rv"].copy()
    mom = F32(case["momentum"])
    segs = range(len(offs) - 1) if mut != "running_last" else [len(offs) - 2]
    for s in segs:
        ns = offs[s + 1] - offs[s]
        unb = vf[s] if mut == "running_biased" else (vf[s] * F32(F32(ns) / F32(ns - 1))).astype(F32)
        rm = ((rm * F32(F32(1) - mom)).astype(F32) + (mf[s] * mom).astype(F32)).astype(F32)
        rv = ((rv * F32(F32(1) - mom)).astype(F32) + (unb * mom).astype(F32)).astype(F32)
    ys, guard = _store(y, case, "y", mut)
    return {"y_bn": ys, "guard": guard, "save_mean": mf, "save_rstd": rs, "run_mean": rm, "run_var": rv,
            "count": case["count"] + (1 if mut == "counter1" else len(offs) - 1)}


def r_inst(case, mode, with_res, segmented=True, mut=None):
    x, eps = case["x"], case["eps"]
    offs = case["offs"] if segmented else O.one(case["n"])
    mf, vf, rs = _stats(x, offs, eps, mut, K.x_form(case["c"], case["layout"]))
    y = np.empty_like(x)
    for s in range(len(offs) - 1):
        a, e = offs[s], offs[s + 1]
        k = 0 if mut == "seg0_stats" else s
        v = _fma(x[a:e], rs[k], (-mf[k] * rs[k]).astype(F32))
        if with_res:
            v = (v + case["res_in"][a:e]).astype(F32)
        if mut == "leaky_side" and mode == 2:
            v = np.where(v > 0, (v * F32(case["slope"])).astype(F32), v)
        else:
            v = _act32(v, mode, case["slope"])
        y[a:e] = v
    ys, guard = _store(y, case, "y", mut)
    return {"y_in": ys, "guard": guard}


def r_stats(case, mut=None):
    x, n = case["x"], case["n"]
    form = K.x_form(case["c"], case["layout"])
    mf, vf, rs = _stats(x, O.one(n), case["eps"], mut, form)
    xd = x.astype(np.float64)
    P, _ = _partials(xd, xd * xd, O.one(n), mut, form)
    return {"mean": mf[0], "var": vf[0], "scale": rs[0], "shift": (-mf[0] * rs[0]).astype(F32),
            "colsum": _combine(P[:O.nblocks(n), 0], mut).astype(F32)}


def r_bwd(x, y, dy, offs, mean, rstd, gamma, relu, mut=None, chain=False):
    """k_bn_train_bwd_partial / _apply (chain: apr_norm_backward) -> dx, dres, dgamma, dbeta"""
    g = dy if not relu else np.where((y >= 0) if mut == "mask_ge" else (y > 0), dy, F32(0)).astype(F32)
    xh = np.empty_like(x)
    for s in range(len(offs) - 1):
        a, e = offs[s], offs[s + 1]
        xh[a:e] = ((x[a:e] - mean[s]).astype(F32) * rstd[s]).astype(F32)
    gd = g.astype(np.float64)
    P, blk0 = _partials(gd, gd * xh.astype(np.float64), offs, mut, "norm_bwd" if chain else "bn_bwd")
    dx = np.empty_like(x)
    ta, tb = np.zeros(x.shape[1]), np.zeros(x.shape[1])
    gam = np.ones(x.shape[1], F32) if gamma is None else gamma
    for s in range(len(offs) - 1):
        a, e = offs[s], offs[s + 1]
        ns = e - a if mut != "total_n" else offs[-1]
        seg = P[blk0[s]:blk0[s + 1]]
        sa, sb = _combine(seg[:, 0], mut, chain), _combine(seg[:, 1], mut, chain)
        if s == 0 or mut != "dgamma_seg0":
            ta, tb = ta + sa, tb + sb
        k1, k2 = (sa / ns).astype(F32), (sb / ns).astype(F32)
        gs = (gam * rstd[s]).astype(F32)
        dx[a:e] = (gs * _fma(-xh[a:e], k2, (g[a:e] - k1).astype(F32))).astype(F32)
    return {"dx": dx, "dres": g, "dgamma": tb.astype(F32), "dbeta": ta.astype(F32)}


def r_act_in(case, y, mut=None):
    """k_act_backward, LeakyReLU, on the instance norm's output"""
    dy = case["dy"]
    return {"dz_in": np.where((y >= 0) if mut == "leaky_mask_ge" else (y > 0), dy, (dy * F32(case["slope"])).astype(F32))}


def r_affine(case, mode, mut=None):
    """k_affine_act / k_act_backward; `one_sweep`: the grid-stride loop runs once"""
    x = case["x"]
    v = (x * case["scale"]).astype(F32)
    v = (v + case["shift"]).astype(F32)
    v = (v + case["res"]).astype(F32)
    y = _act32(v, mode, case["slope"])
    dy = case["dy"]
    if mode == 0:
        dz = dy.copy()
    else:
        other = (dy * F32(case["slope"])).astype(F32) if mode == 2 else np.zeros_like(dy)
        dz = np.where(y > 0, dy, other)
    if mut == "one_sweep":
        y, dz = y.copy().reshape(-1), dz.copy().reshape(-1)
        y[K.SWEEP:] = NAN
        dz[K.SWEEP:] = NAN
        y, dz = y.reshape(x.shape), dz.reshape(x.shape)
    return {"y_aff": y, "dz": dz}


def r_l2(case, mut=None):
    """one wave per row: lane sums by multiply-add over col = lane, lane + 64, .., then the xor butterfly"""
    x, dy = case["x"], case["dy"]
    n, c = x.shape
    with np.errstate(all="ignore"):
        ss, dot = np.zeros((n, 64), F32), np.zeros((n, 64), F32)
        for col in range(c):
            ss[:, col % 64] = _fma(x[:, col], x[:, col], ss[:, col % 64])
            dot[:, col % 64] = _fma(x[:, col], dy[:, col], dot[:, col % 64])
        for d in (32, 16, 8, 4, 2, 1):
            perm = np.arange(64) ^ d
            ss, dot = (ss + ss[:, perm]).astype(F32), (dot + dot[:, perm]).astype(F32)
        nrm = np.sqrt(ss[:, :1])
        y = (x / nrm).astype(F32)
        k = dot[:, :1] / ((nrm * nrm).astype(F32) if mut != "l2_once" else nrm)
        dx = (_fma(-x, k, dy) / nrm).astype(F32)
    return y, dx


# ------------------------------------------------------------------------------------------------ running a case
def _restate_case(case, mut=None):
    """every quantity of one case through the restatement against the oracle; raises AssertionError where one is outside"""
    name = case["name"]
    w = WORST if mut is None else None
    got = r_inst(case, 2, True, True, mut)
    assert np.isnan(got["guard"]).all(), (name, "guard columns written")
    K.check(name, got, K.expect_inst(case, 2, True), w)
    K.check(name, r_act_in(case, got["y_in"], mut), K.expect_act_in(case), w)
    K.check(name, r_inst(case, 1, True, True, mut), K.expect_inst(case, 1, True), w)
    K.check(name, r_inst(case, 0, False, False, mut), K.expect_inst(case, 0, False, False), w)
    K.check(name, r_stats(case, mut), K.expect_stats(case), w)
    for with_gamma in (False, True):
        e = K.expect_norm_bwd(case, with_gamma)
        got = r_bwd(case["x"], None, case["dy"], O.one(case["n"]), e["mean"], e["rstd"], case["gamma"] if with_gamma else None,
                    False, mut, chain=True)
        K.check(name, got, e, w)
    if case["inst_only"]:
        return
    for relu in (True, False):
        got = r_bn_fwd(case, relu, True, mut)
        assert np.isnan(got["guard"]).all(), (name, "guard columns written")
        K.check(name, got, K.expect_bn_fwd(case, relu, True), w)
        e = K.expect_bn_bwd(case, relu)
        mean, rstd = K.given_stats(case)
        K.check(name, r_bwd(case["x"], got["y_bn"], case["dy"], case["offs"], mean, rstd, case["gamma"], relu, mut), e, w)
    K.check(name, r_bn_fwd(case, False, False, mut), K.expect_bn_fwd(case, False, False), w)


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", list(K.NORM))
def test_case_plants_its_fact_and_is_decision_safe(name):
    c = K.NORM[name]
    n, cc, offs = c["n"], c["c"], c["offs"]
    assert offs[0] == 0 and offs[-1] == n and len(offs) - 1 <= O.MAX_SEG and all(b > a for a, b in zip(offs, offs[1:]))
    assert c["inst_only"] == any(b - a == 1 for a, b in zip(offs, offs[1:]))
    m = O.pre_margin(c["x"], offs, c["eps"], None, None, c["res_in"], "scaleshift")
    v = O.pre_activation(c["x"], offs, c["eps"], None, None, c["res_in"])
    assert (v[c["zero_in"]] == 0).all() and (m[~c["zero_in"]] > 4).all(), name
    if not c["inst_only"]:
        m = O.pre_margin(c["x"], offs, c["eps"], c["gamma"], c["beta"], c["res"], "subtract")
        v = O.pre_activation(c["x"], offs, c["eps"], c["gamma"], c["beta"], c["res"])
        assert (v[c["zero_bn"]] == 0).all() and (m[~c["zero_bn"]] > 4).all(), name
    if c["special"]:
        mean, var, _ = O.seg_stats(c["x"], offs, c["eps"])
        assert (np.abs(mean[:, 0]) / np.sqrt(var[:, 0] + 1e-30) > 500).all() or min(b - a for a, b in zip(offs, offs[1:])) < 8
        assert (var[:, 1] == 0).all() and (c["x"][:, 2] == 0).all() and c["gamma"][3] == 0 and c["gamma"][4] < 0
        assert c["zero_bn"].sum() == c["zero_in"].sum() == (2 if n > 1 else 1)
        assert np.abs(c["x"][:, 6]).max() < 1e-16 and np.abs(c["x"][:, 7]).max() > 1e16 or n < 8
        assert (c["dy"][c["zero_in"]] != 0).all()
    if c["negvar"]:
        # the search found a seed: negative in the order of both forms of k_bn_partial, the last product fused or not
        form = K.x_form(cc, c["layout"])
        assert form == ("vec" if name == "negvar-c8" else "scalar")
        assert all(K.one_pass_var(c["x"][:, 5], f, fused) < -2 * c["eps"] for f in ("vec", "scalar") for fused in (False, True))
        mf, vf, rs = _stats(c["x"], offs, c["eps"], None, form)
        assert vf[0, 5] == 0 and rs[0, 5] == F32(1) / np.sqrt(F32(c["eps"])) and np.isfinite(rs).all()
        assert not np.isfinite(_stats(c["x"], offs, c["eps"], "noclamp_var", form)[2][0, 5])
    nb = [O.nblocks(b - a) for a, b in zip(offs, offs[1:])]
    if name.startswith("blk"):
        assert str(max(nb)) == name.split("-")[0][3:]
    # the 16-byte form needs c % 4 == 0: a layout that misaligns one tensor only means something there
    if c["layout"] not in ("contig", "ld1", "slice4", "y_ld"):
        assert cc % 4 == 0, name


def test_case_list_covers_the_issue():
    rows = {b - a for c in K.NORM.values() for a, b in zip(c["offs"], c["offs"][1:])}
    assert {1, 2, 3, 255, 256, 257, 511, 513, 31 * 256, 32 * 256 + 1, 33 * 256, 64 * 256, 65 * 256 + 1} <= rows
    widths = {c["c"] for c in K.NORM.values()}
    assert {1, 3, 4, 5, 60, 63, 64, 65, 68, 129, 252, 258, 260} <= widths
    assert {c["c"] for c in K.L2.values()} >= {1, 3, 5, 63, 64, 65, 129, 512, 516}
    assert {c["layout"] for c in K.NORM.values()} == set(K.LAYOUTS)
    big = [c for c in K.NORM.values() if c["n"] > 3000]
    assert all(c["c"] in (5, 68) for c in big)
    nseg = {len(c["offs"]) - 1 for c in K.NORM.values()}
    assert 32 in nseg and 1 in nseg and 2 in nseg
    longest = {int(np.argmax(np.diff(c["offs"]))) / max(len(c["offs"]) - 2, 1) for c in K.NORM.values() if len(c["offs"]) > 3}
    assert 1.0 in longest and any(0 < v < 1 for v in longest)


@pytest.mark.parametrize("name", list(K.NORM))
def test_float32_restatement_stays_inside_the_bounds(name):
    _restate_case(K.NORM[name])


@pytest.mark.parametrize("name", K.STRIDE_NAMES)
def test_grid_stride_cases(name):
    c = K.stride_case(name)
    total = c["n"] * c["c"]
    assert total > K.SWEEP and c["planted"] == [K.SWEEP, total - 1]
    for mode in (1, 2):
        e = K.expect_affine(c, mode)
        y = e["y_aff"][0].reshape(-1)
        assert (y[c["planted"]] == 0).all() and (c["dy"].reshape(-1)[c["planted"]] != 0).all()
        pre = O.affine_act(c["x"], c["scale"], c["shift"], c["res"], 0)
        margin = np.abs(pre) / O.bound_affine_act(c["x"], c["scale"], c["shift"], c["res"], 0)
        margin.reshape(-1)[c["planted"]] = np.inf
        assert margin.min() > 1e4
        K.check(name, r_affine(c, mode), e, WORST)
        assert _rejected(lambda: K.check(name, r_affine(c, mode, "one_sweep"), e)), "one_sweep not rejected"
    print(f"mutant one_sweep rejected by {name}")


@pytest.mark.parametrize("name", list(K.L2))
def test_l2_cases_and_restatement(name):
    c = K.L2[name]
    e = K.expect_l2(c)
    z, o, d = c["special_rows"]
    # what the reference's float32 expression yields there: NaN for the zero row, 0 for the overflowing one, inf for denormals
    assert (e["kind_y"][z] == 4).all() and (e["kind_y"][o] == 1).all() and (e["kind_y"][d] == 2).all()
    x = torch.from_numpy(c["x"])
    ref = (x / torch.norm(x, p=2, dim=1, keepdim=True)).numpy()
    # torch agrees on the zero row on any device; a host torch.norm sums squares in a wider type than float32, so the
    # overflowing and the denormal row are pinned by the float32 expression (what the reference's device reduction does)
    assert (O.kind(ref)[z] == e["kind_y"][z]).all()
    assert (e["kind_dx"][z] == 4).all() and (e["kind_dx"][o] == 1).all() and (e["kind_dx"][d] == 3).all()
    y, dx = r_l2(c)
    ry, rd = K.check_l2(c, y, dx)
    WORST["y_l2"], WORST["dx_l2"] = max(WORST.get("y_l2", 0), ry), max(WORST.get("dx_l2", 0), rd)
    if c["c"] > 1:
        assert _rejected(lambda: K.check_l2(c, *r_l2(c, "l2_once"))), "l2_once not rejected"


# mutant -> the case named to reject it
MUTANTS = {
    "noclamp": "seg-2-700",            # last block not clamped to the segment's end
    "stop32": "blk33-n8193-c5",        # combine loop stops at 32 blocks
    "unroll7": "blk31-n7936-c68",      # inner unroll one short
    "blk0_row0": "seg-ragged",         # blk0 taken as row0 / 256
    "seg0_stats": "seg-last",          # segment s normalised with segment 0's statistics
    "total_n": "seg-middle",           # the total n used as a segment's n
    "running_biased": "n2-c68",        # biased variance into running_var
    "running_last": "seg-700-2",       # running statistics from the last segment only
    "counter1": "seg-32",              # counter += 1
    "dgamma_seg0": "seg-mult256",      # dgamma / dbeta from segment 0 only
    "mask_ge": "n256-c60",             # ReLU mask y >= 0 (every masked element has y == 0 there: any case rejects it)
    "leaky_mask_ge": "n256-c60",       # LeakyReLU mask y >= 0: differs at the planted y == 0 alone
    "leaky_side": "n3-c3",             # LeakyReLU slope applied on the wrong side
    "noclamp_var": "negvar-c8",        # variance not clamped
    "dead_column": "n3-c3",            # a dead column of a live quad written
    "fp32acc": "n300-c252",            # float32 accumulation of the statistics (|mean| / std = 1e3 in column 0)
}


@pytest.mark.parametrize("mut", list(MUTANTS))
def test_mutant_is_rejected_by_its_named_case(mut):
    case = K.NORM[MUTANTS[mut]]
    _restate_case(case)                                        # the restatement itself passes there
    assert _rejected(lambda: _restate_case(case, mut)), f"mutant {mut} passes {case['name']}"
    print(f"mutant {mut} rejected by {case['name']}")


def test_compare_rows_fails_nan_against_finite():
    one = np.ones((2, 2))
    assert O.compare_rows(one, one, one)[0] == 0
    bad = one.copy()
    bad[1, 0] = NAN
    assert O.compare_rows(bad, one, one * 1e30) == (np.inf, (1, 0))
    bad[1, 0] = np.inf
    assert O.compare_rows(bad, one, one * np.inf)[0] == np.inf
    assert O.compare_rows(one * 1.5, one, one * 0)[1] == (0, 0)


def test_mean_over_std_table():
    """the issue's table: worst |float32 form - float64| at |mean| / std = 10 .. 1e4 (n = 3000, std = 1, eps = 1e-5) for both
    apply forms; each stays inside its bound and the scale/shift form is the worse by about 2x, not by orders"""
    rng = np.random.default_rng(5)
    base = rng.standard_normal((3000, 1))
    for ratio in (10.0, 100.0, 1000.0, 10000.0):
        x = (base + ratio).astype(F32)
        case = {"name": f"ratio{ratio:g}", "x": x, "offs": [0, 3000], "n": 3000, "c": 1, "eps": K.EPS, "slope": 0.0, "layout": "contig",
                "res_in": None, "gamma": np.ones(1, F32), "beta": np.zeros(1, F32), "rm": np.zeros(1, F32), "rv": np.ones(1, F32),
                "momentum": 0.0, "count": 0}
        ref = O.norm_act(x, [0, 3000], K.EPS)
        fused = r_inst(case, 0, False)["y_in"]
        sub = r_bn_fwd(case, False, False)["y_bn"]
        ef, es = np.abs(fused - ref).max(), np.abs(sub - ref).max()
        bf = O.bound_norm_act(x, [0, 3000], K.EPS, form="scaleshift")
        bs = O.bound_norm_act(x, [0, 3000], K.EPS, form="subtract")
        onepass = abs(K.one_pass_var(x[:, 0], "scalar") - x.astype(np.float64).var()) / x.astype(np.float64).var()
        print(f"|mean|/std {ratio:g}: fused {ef:.1e} (ratio {np.max(np.abs(fused - ref) / bf):.2f}), subtract-first {es:.1e} "
              f"(ratio {np.max(np.abs(sub - ref) / bs):.2f}), one-pass variance off by {onepass:.0e}")
        assert (np.abs(fused - ref) <= bf).all() and (np.abs(sub - ref) <= bs).all()
        assert ef < 8 * es + 1e-6


def test_zz_print_worst_restatement_ratios():
    print("worst restatement / bound:", {k: round(v, 3) for k, v in sorted(WORST.items())})
    assert all(v <= 1.0 for v in WORST.values())
