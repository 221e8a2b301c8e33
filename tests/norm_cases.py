"""Named inputs for the normalisation kernels (apr_amd/csrc/norm.hip), each with the fact it plants;
tests/test_norm_oracle_cpu.py confirms every fact on the host.  numpy only, everything from small integer seeds.

Kernel constants the cases are built around:
* statistics are fp64 partial sums per 256-row block of a segment, combined per column by 4 thread groups: group g takes
  blocks g, g + 4, .., g + 28, then g + 32, ..: the loop has one trip up to 32 blocks, two from 33, three from 65; its 8-way
  unrolled inner stride 4 is full only when the trip has 32 blocks left.
* segments: blk0[s + 1] = blk0[s] + ceil(rows / 256); at most 32; the grids are sized by the longest segment; segment 0's
  first workgroups walk all segments for the running statistics and dgamma / dbeta.
* every kernel has a 16-byte form (c % 4 == 0, every leading dimension % 4 == 0, every base pointer 16-byte aligned) and a
  4-byte form; a workgroup owns 64 columns = 16 column quads.
* apr_affine_act / apr_act_backward launch at most 8192 blocks of 256 threads and stride over 2 097 152 elements.
* apr_l2_normalize[_backward]: one wave per row, 4 rows per block, ceil(c / 64) passes per lane.

A layout maps a tensor's role to (extra floats per row, base offset in floats); roles: x, res, y (the forward's output),
dy, yb (y as the backward reads it), dx, dres.  Every output lives in a NaN-filled buffer.

Values of a `special` case (c >= 8): column 0 has |mean| / std = 1e3, column 1 is constant, column 2 is zero, column 3 has
gamma = 0, column 4 a negative gamma, column 6 is scaled by 1e-18 and column 7 by 1e18.  Rows 0 and n - 1 plant y == 0:
under apr_bn_train_fwd in the constant column (res = -beta: (z - mean) is exactly 0), under the instance norm in the zero
column (res = 0: 0 * scale + (-0 * scale) is exactly 0; the constant column is NOT exactly 0 there).
Every other pre-activation is at least 4 bounds away from 0 (`decision-safe`): the residual is pushed where it is not.
"""
import numpy as np

import norm_oracle as O

F32 = np.float32
EPS = 1e-5
SLOPE = 0.1
MOMENTUM = 0.05
SWEEP = 8192 * 256

LAYOUTS = {
    "contig": {},
    "slice4": {r: (4, 0) for r in ("x", "res", "y", "dy", "yb", "dx", "dres")},
    "ld1": {r: (1, 0) for r in ("x", "res", "y", "dy", "yb", "dx", "dres")},
    "off1": {r: (4, 1) for r in ("x", "res", "y", "dy", "yb", "dx", "dres")},
    "off2": {r: (4, 2) for r in ("x", "res", "y", "dy", "yb", "dx", "dres")},
    "off3": {r: (4, 3) for r in ("x", "res", "y", "dy", "yb", "dx", "dres")},
    "xoff1": {"x": (4, 1)},
    "res_mis": {"res": (4, 1)},
    "y_mis": {"y": (4, 2)},
    "y_ld": {"y": (8, 0), "dx": (8, 0)},
    "dy_mis": {"dy": (4, 3)},
    "yb_mis": {"yb": (4, 1)},
    "dres_mis": {"dres": (4, 2)},
    "dx_mis": {"dx": (4, 1)},
}


def lay(case, role):
    return LAYOUTS[case["layout"]].get(role, (0, 0))


def _safe_residual(x, offs, gamma, beta, res, form, keep):
    """push the residual where the pre-activation is within 4 bounds of 0 (not at the planted zeros `keep`)"""
    res = res.copy()
    for _ in range(4):
        v = O.pre_activation(x, offs, EPS, gamma, beta, res)
        bd = O.bound_norm_act(x, offs, EPS, gamma, beta, res, 0, 0.0, form)
        bad = (np.abs(v) < 4 * bd) & ~keep
        if not bad.any():
            break
        res[bad] = (res[bad].astype(np.float64) + np.where(v[bad] < 0, -1.0, 1.0) * 16 * bd[bad]).astype(F32)
    return res


def build(name, fact, seed, offs, c, layout="contig", special=None, negvar=False, inst_only=False):
    rng = np.random.default_rng(seed)
    offs = [int(v) for v in offs]
    n = offs[-1]
    special = (c >= 8) if special is None else special
    x = (rng.standard_normal((n, c)) * rng.uniform(0.5, 3, c) + rng.uniform(-2, 2, c)).astype(F32)
    gamma = rng.uniform(0.5, 1.5, c).astype(F32)
    beta = rng.uniform(-0.5, 0.5, c).astype(F32)
    if special:
        x[:, 0] = (rng.standard_normal(n) + 1000.0).astype(F32)
        x[:, 1] = F32(1.75)
        x[:, 2] = 0
        gamma[3], gamma[4] = 0.0, -1.25
        x[:, 6] = (x[:, 6].astype(np.float64) * 1e-18).astype(F32)
        x[:, 7] = (x[:, 7].astype(np.float64) * 1e18).astype(F32)
    if negvar:
        x[:, 5] = negvar_column(n)
    res = rng.standard_normal((n, c)).astype(F32)
    res_in = rng.standard_normal((n, c)).astype(F32)
    keep_bn = np.zeros((n, c), bool)
    keep_in = np.zeros((n, c), bool)
    if special:
        for r in (0, n - 1):
            res[r, 1] = -beta[1]
            keep_bn[r, 1] = True
            res_in[r, 2] = 0
            keep_in[r, 2] = True
    case = {"name": name, "fact": fact, "n": n, "c": c, "offs": offs, "layout": layout, "x": x, "gamma": gamma, "beta": beta,
            "eps": EPS, "slope": SLOPE, "momentum": MOMENTUM, "special": special, "negvar": negvar, "inst_only": inst_only,
            "dy": rng.standard_normal((n, c)).astype(F32), "rm": rng.standard_normal(c).astype(F32),
            "rv": rng.uniform(0.5, 2, c).astype(F32), "count": int(rng.integers(0, 1000)),
            "zero_bn": keep_bn, "zero_in": keep_in}
    if not inst_only:
        case["res"] = _safe_residual(x, offs, gamma, beta, res, "subtract", keep_bn)
    case["res_in"] = _safe_residual(x, offs, None, None, res_in, "scaleshift", keep_in)
    return case


# ------------------------------------------------------------------------- the kernels' own order inside a block
LANES = {"vec": 64, "scalar": 16, "bn_bwd": 16, "norm_bwd": 4}


def block_sum(rows, form, dtype=np.float64):
    """the sum of one block's rows [<= 256, c] in the order of the partial kernels: lane l adds rows l, l + L, l + 2 L, ..
    in ascending order (rows past the block's end add 0), then the L lane sums are added in ascending lane order.
    L = 64 on k_bn_partial's 16-byte form (rows rl + 64 u, then the 64-step chain through LDS), 16 on its 4-byte form (rows
    ty + 128 k + 16 u, then 16 steps) and in k_bn_train_bwd_partial (rows rl + 64 k + 16 u), 4 in k_norm_bwd_partial."""
    L = LANES[form]
    rows = np.asarray(rows, dtype)
    pad = np.zeros((O.ROWS,) + rows.shape[1:], dtype)
    pad[:len(rows)] = rows
    lanes = pad.reshape((O.ROWS // L, L) + rows.shape[1:])
    s = np.zeros_like(lanes[0])
    for k in range(O.ROWS // L):
        s = (s + lanes[k]).astype(dtype)
    t = np.zeros_like(s[0])
    for l in range(L):
        t = (t + s[l]).astype(dtype)
    return t


def x_form(c, layout):
    """the form k_bn_partial takes: 16-byte iff c % 4 == 0, ld % 4 == 0 and the base is 16-byte aligned"""
    extra, off = LAYOUTS[layout].get("x", (0, 0))
    return "vec" if c % 4 == 0 and extra % 4 == 0 and off % 4 == 0 else "scalar"


def combine(p, stop32=False, unroll=8, dtype=np.float64):
    """the stride-32 / inner-stride-4 combine of k_bn_finish, k_norm_apply and column_sums over the block partials p"""
    nblk = len(p)
    grp = []
    for g in range(4):
        s = dtype(0.0)
        for b0 in range(g, nblk, 32):
            for u in range(unroll):
                b = b0 + 4 * u
                if b < nblk:
                    s = dtype(s + dtype(p[b]))
            if stop32:
                break
        grp.append(s)
    return dtype(dtype(dtype(grp[0] + grp[1]) + grp[2]) + grp[3])


def one_pass_var(col, form="vec", fused=False):
    """the kernels' fp64 one-pass variance of one column in their order: block sums as block_sum, the combine, then
    sum x^2 / n - m * m -- with the product rounded on its own, or (fused) inside one multiply-add, which the compiler may
    choose: both are restated, exactly, so that a case can hold under either"""
    from fractions import Fraction
    col = np.asarray(col, np.float64)
    n = len(col)
    nb = O.cdiv(n, O.ROWS)
    pa = [float(block_sum(col[b * O.ROWS:(b + 1) * O.ROWS, None], form)[0]) for b in range(nb)]
    pq = [float(block_sum(col[b * O.ROWS:(b + 1) * O.ROWS, None] ** 2, form)[0]) for b in range(nb)]
    m = float(combine(pa)) / n
    e2 = float(combine(pq)) / n
    return float(Fraction(e2) - Fraction(m) * Fraction(m)) if fused else e2 - m * m


_NEGVAR = {}


def negvar_column(n):
    """a column V ~ 2e6 .. 9e6, constant but for one row one ulp up (true variance ~ 2e-17 V^2, far below the 1e-16 V^2 the
    fp64 one-pass form loses), whose one-pass variance is below -2 eps in the order of BOTH forms of k_bn_partial and with
    the last product fused or not.  Searched over seeds."""
    if n not in _NEGVAR:
        found = None
        for seed in range(4000):
            rng = np.random.default_rng(9000 + seed)
            col = np.full(n, F32(rng.uniform(2e6, 9e6)), F32)
            r = int(rng.integers(n))
            col[r] = np.nextafter(col[r], F32(np.inf))
            if all(one_pass_var(col, form, fused) < -2 * EPS for form in ("vec", "scalar") for fused in (False, True)):
                found = col
                break
        _NEGVAR[n] = found
    assert _NEGVAR[n] is not None, f"no negative one-pass variance found for n = {n}"
    return _NEGVAR[n]


# --------------------------------------------------------------------------------------------------------- the cases
def _ragged32():
    rows = np.random.default_rng(32).integers(2, 121, 32)      # 2 .. 300 rows, under 3000 in all
    rows[3], rows[17], rows[31] = 2, 300, 257
    return [0] + [int(v) for v in np.cumsum(rows)]


def _ragged32_inst():
    o = _ragged32()
    return o[:6] + [o[5] + 1] + [v + 1 for v in o[6:-1]]        # 32 segments, the sixth of 1 row


def _all():
    cases = []
    add = lambda *a, **k: cases.append(build(*a, **k))
    # rows per segment x widths x layouts (one segment)
    add("n1-c5", "1 row: variance 0, rstd = 1 / sqrt(eps) (instance norm only)", 1, [0, 1], 5, inst_only=True)
    add("n1-c64", "1 row on the 16-byte form (instance norm only)", 2, [0, 1], 64, inst_only=True)
    add("n2-c1", "2 rows, 1 column", 3, [0, 2], 1)
    add("n2-c68", "2 rows; 68 = a second workgroup with one live quad", 4, [0, 2], 68)
    add("n3-c3", "3 rows, 3 columns, ld = c + 1", 5, [0, 3], 3, "ld1")
    add("n255-c4", "one row short of a block; one live quad", 6, [0, 255], 4)
    add("n256-c60", "exactly one block; 15 live quads and a dead one", 7, [0, 256], 60, "slice4")
    add("n257-c63", "one row into the second block; 4-byte form", 8, [0, 257], 63)
    add("n511-c64", "two blocks less a row; base offset by 1 float with c % 4 == 0", 9, [0, 511], 64, "off1")
    add("n513-c65", "three blocks; one column into the second workgroup", 10, [0, 513], 65)
    add("n257-c129", "129 columns: three workgroups", 11, [0, 257], 129, "ld1")
    add("n300-c252", "252: the last workgroup has 15 live quads; base offset by 2 floats", 12, [0, 300], 252, "off2")
    add("n300-c258", "258: 4-byte form, 2 live columns in the fifth workgroup", 13, [0, 300], 258)
    add("n300-c260", "260: one live quad in the fifth workgroup; base offset by 3 floats", 14, [0, 300], 260, "off3")
    add("n513-c68-xoff", "only the input misaligned", 15, [0, 513], 68, "xoff1")
    add("n513-c68-res", "only the residual misaligned", 16, [0, 513], 68, "res_mis")
    add("n513-c68-y", "only the output misaligned", 17, [0, 513], 68, "y_mis")
    add("n513-c68-yld", "a strided, aligned output (ldy = c + 8)", 18, [0, 513], 68, "y_ld")
    add("n513-c68-dy", "only dy misaligned (backward)", 19, [0, 513], 68, "dy_mis")
    add("n513-c68-yb", "only the mask's y misaligned (backward)", 20, [0, 513], 68, "yb_mis")
    add("n513-c68-dres", "only dres misaligned (backward)", 21, [0, 513], 68, "dres_mis")
    add("n513-c68-dx", "only dx misaligned (backward)", 22, [0, 513], 68, "dx_mis")
    add("negvar-c8", "column 5 (constant but for one ulp in one row) has a one-pass fp64 variance below -2 eps in the 16-byte form's order: the clamp", 23, [0, 700], 8, negvar=True)
    add("negvar-c8-ld1", "the same column in the 4-byte form's order of rows: negative there too", 24, [0, 700], 8, "ld1", negvar=True)
    # segments
    add("seg-2-700", "a 2-row segment next to one of three blocks", 30, [0, 2, 702], 68)
    add("seg-700-2", "the short segment last", 31, [0, 700, 702], 5)
    add("seg-last", "the longest segment last: the grids are sized by it", 32, [0, 100, 357, 1157], 60, "slice4")
    add("seg-middle", "the longest segment in the middle", 33, [0, 257, 1300, 1310], 65)
    add("seg-mult256", "every size a multiple of 256", 34, [0, 256, 1024, 1536], 64)
    add("seg-ragged", "no size a multiple of 256", 35, [0, 255, 512, 1025, 1282], 12, "ld1")
    add("seg-32", "32 segments of 2 .. 300 rows (kMaxSeg)", 36, _ragged32(), 68)
    add("seg-32-c5", "32 segments on the 4-byte form", 37, _ragged32(), 5)
    add("seg-32-one", "32 segments, one of a single row (instance norm only)", 38, _ragged32_inst(), 12, inst_only=True)
    # block counts at the combine loop's edges
    for k, (rows, what) in enumerate([(31 * 256, "31 blocks: the inner unroll's last slot is empty in three groups"),
                                      (32 * 256 + 1, "33 blocks: a second trip of one block"),
                                      (33 * 256, "33 full blocks"), (64 * 256, "64 blocks: two full trips"),
                                      (65 * 256 + 1, "66 blocks: a third trip")]):
        add(f"blk{O.nblocks(rows)}-n{rows}-c5", what + "; 4-byte form", 40 + k, [0, rows], 5, special=False)
        add(f"blk{O.nblocks(rows)}-n{rows}-c68", what + "; 16-byte form", 50 + k, [0, rows], 68, special=False)
    add("seg-blk33-last", "a 3-row segment, then one of 33 blocks: blk0 = 1 for the long one", 60, [0, 3, 3 + 32 * 256 + 1], 5,
        special=False)
    return {c["name"]: c for c in cases}


NORM = _all()
BN = {k: v for k, v in NORM.items() if not v["inst_only"]}
SMALL = {k: v for k, v in NORM.items() if v["n"] <= 3000}

REFUSED_OFFSETS = {
    "33 segments": list(range(0, 34 * 3, 3)),
    "offsets not ending at n": [0, 10, 19],
    "an empty segment": [0, 10, 10, 20],
}


# -------------------------------------------------------------------------------------------------------- grid stride
def build_stride(name, total, c, seed):
    """apr_affine_act / apr_act_backward past one sweep of 8192 x 256 threads.  The pre-activation is built to be a target of
    magnitude 0.5 .. 2 (decision-safe), exactly 0 at the planted elements: SWEEP (the first of the second sweep; the middle
    one of a total below a sweep) and the last; there x = 0 and res = -shift."""
    assert total % c == 0
    n = total // c
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, c)).astype(F32)
    scale = rng.uniform(0.5, 1.5, c).astype(F32)
    shift = rng.uniform(-0.5, 0.5, c).astype(F32)
    target = rng.uniform(0.5, 2, (n, c)) * np.where(rng.random((n, c)) < 0.5, -1.0, 1.0)
    res = (target - (x.astype(np.float64) * scale + shift)).astype(F32)
    planted = [SWEEP if total > SWEEP else total // 2, total - 1]
    for t in planted:
        r, j = divmod(t, c)
        x[r, j] = 0
        res[r, j] = -shift[j]
    return {"name": name, "n": n, "c": c, "x": x, "scale": scale, "shift": shift, "res": res, "planted": planted,
            "dy": rng.standard_normal((n, c)).astype(F32), "slope": SLOPE}


_STRIDE = {}


def stride_case(name):
    """totals: one sweep + 64 and two sweeps + 5 elements, rounded up to a multiple of c (2 * SWEEP + 5 is no multiple of
    5, SWEEP + 64 neither), at c = 64 and c = 5"""
    if name not in _STRIDE:
        total, c, seed = {"sweep1-c64": (SWEEP + 64, 64, 70), "sweep1-c5": (SWEEP + 64, 5, 72),
                          "sweep2-c64": (2 * SWEEP + 5, 64, 73), "sweep2-c5": (2 * SWEEP + 5, 5, 71)}[name]
        _STRIDE[name] = build_stride(name, O.cdiv(total, c) * c, c, seed)
    return _STRIDE[name]


STRIDE_NAMES = ("sweep1-c64", "sweep1-c5", "sweep2-c64", "sweep2-c5")


# ----------------------------------------------------------------------------------------------------------- L2 rows
L2_ZERO, L2_OVER, L2_DENORM = 1, 4, 6


def build_l2(name, c, seed, layout="contig"):
    """9 rows = three blocks of 4 waves, the last with one live wave.  Row 1 is zero, row 4 has squares that overflow
    float32 (|x| ~ 1e20), row 6 is denormal (|x| ~ 1e-40, squares underflow to 0); x and dy are positive there so that the
    float32 expression's signs do not depend on the order of the sums.  Row 8 is scaled by 1e-10, row 7 by 1e15."""
    rng = np.random.default_rng(seed)
    n = 9
    x = rng.standard_normal((n, c)).astype(F32)
    dy = rng.standard_normal((n, c)).astype(F32)
    x[L2_ZERO] = 0
    x[L2_OVER] = (rng.uniform(1, 3, c) * 1e20).astype(F32)
    x[L2_DENORM] = (rng.uniform(1, 3, c) * 1e-40).astype(F32)
    dy[[L2_OVER, L2_DENORM]] = np.abs(dy[[L2_OVER, L2_DENORM]]) + F32(0.5)
    x[7] = (x[7].astype(np.float64) * 1e15).astype(F32)
    x[8] = (x[8].astype(np.float64) * 1e-10).astype(F32)
    return {"name": name, "n": n, "c": c, "x": x, "dy": dy, "layout": layout, "special_rows": (L2_ZERO, L2_OVER, L2_DENORM)}


L2 = {c["name"]: c for c in [
    build_l2("l2-c1", 1, 80), build_l2("l2-c3", 3, 81, "ld1"), build_l2("l2-c5", 5, 82), build_l2("l2-c63", 63, 83),
    build_l2("l2-c64", 64, 84, "off1"), build_l2("l2-c65", 65, 85), build_l2("l2-c129", 129, 86, "ld1"),
    build_l2("l2-c512", 512, 87, "slice4"), build_l2("l2-c516", 516, 88)]}


# ------------------------------------------------------------------------------------- what every output is held to
_EXPECT = {}


def _memo(key, fn):
    if key not in _EXPECT:
        _EXPECT[key] = fn()
    return _EXPECT[key]


def expect_stats(case):
    """apr_bn_stats / apr_col_sums / apr_norm_params over ALL rows of the case as one segment -> {name: (ref, bound)}"""
    def make():
        x, n = case["x"], case["n"]
        b = O.stat_bounds(x, O.one(n), case["eps"])
        sc, sh = O.norm_params(x, case["eps"])
        bsc, bsh = O.bound_norm_params(x, case["eps"])
        return {"mean": (b["mean"][0], b["bm"][0]), "var": (b["var"][0], b["bv"][0]),
                "colsum": (O.col_sums(x), O.bound_col_sums(x)), "scale": (sc, bsc), "shift": (sh, bsh)}
    return _memo((case["name"], "stats"), make)


def expect_inst(case, mode, with_res, segmented=True):
    def make():
        offs = case["offs"] if segmented else O.one(case["n"])
        res = case["res_in"] if with_res else None
        return {"y_in": (O.norm_act(case["x"], offs, case["eps"], None, None, res, mode, case["slope"]),
                         O.bound_norm_act(case["x"], offs, case["eps"], None, None, res, mode, case["slope"], "scaleshift"))}
    return _memo((case["name"], "inst", mode, with_res, segmented), make)


def expect_act_in(case):
    """apr_act_backward (LeakyReLU) behind the instance norm: the mask is the oracle's y; at the planted y == 0 the gradient
    takes the slope"""
    def make():
        y = expect_inst(case, 2, True)["y_in"][0]
        return {"dz_in": (O.act_backward(case["dy"], y, 2, case["slope"]), O.bound_act_backward(case["dy"], y, 2, case["slope"]))}
    return _memo((case["name"], "actin"), make)


def expect_bn_fwd(case, relu, with_res):
    def make():
        x, offs, eps = case["x"], case["offs"], case["eps"]
        res = case["res"] if with_res else None
        b = O.stat_bounds(x, offs, eps)
        rm, rv, cnt = O.running(case["rm"], case["rv"], case["count"], x, offs, eps, case["momentum"])
        em, ev = O.bound_running(case["rm"], case["rv"], x, offs, eps, case["momentum"])
        return {"y_bn": (O.norm_act(x, offs, eps, case["gamma"], case["beta"], res, int(relu)),
                         O.bound_norm_act(x, offs, eps, case["gamma"], case["beta"], res, int(relu), 0.0, "subtract")),
                "save_mean": (b["mean"], b["bm"]), "save_rstd": (b["rstd"], b["rstd"] * b["R"]),
                "run_mean": (rm, em), "run_var": (rv, ev), "count": cnt}
    return _memo((case["name"], "bnf", relu, with_res), make)


def given_stats(case, offs=None):
    """the float32 statistics handed to the backward kernels: the oracle's own, rounded"""
    m, _, r = O.seg_stats(case["x"], case["offs"] if offs is None else offs, case["eps"])
    return m.astype(F32), r.astype(F32)


def expect_bn_bwd(case, relu):
    """backward of apr_bn_train_fwd with the residual: the mask is the ORACLE's y (decision-safe: the kernel's agrees)"""
    def make():
        x, offs, eps = case["x"], case["offs"], case["eps"]
        y = O.norm_act(x, offs, eps, case["gamma"], case["beta"], case["res"], int(relu))
        g = O.act_backward(case["dy"], y, int(relu))
        mean, rstd = given_stats(case)
        dx, dg, db = O.norm_backward(x, g, offs, mean, rstd, case["gamma"])
        bdx, bdg, bdb = O.bound_norm_backward(x, g, offs, mean, rstd, case["gamma"])
        return {"y": y.astype(F32), "dx": (dx, bdx), "dres": (g, np.zeros_like(g)), "dgamma": (dg, bdg), "dbeta": (db, bdb)}
    return _memo((case["name"], "bnb", relu), make)


def expect_norm_bwd(case, with_gamma):
    """apr_norm_backward over all rows as one segment, dy taken as it is"""
    def make():
        x, n = case["x"], case["n"]
        mean, rstd = given_stats(case, O.one(n))
        gam = case["gamma"] if with_gamma else None
        dx, dg, db = O.norm_backward(x, case["dy"], O.one(n), mean, rstd, gam)
        bdx, bdg, bdb = O.bound_norm_backward(x, case["dy"], O.one(n), mean, rstd, gam, chain=True)
        return {"mean": mean, "rstd": rstd, "dx": (dx, bdx), "dgamma": (dg, bdg), "dbeta": (db, bdb)}
    return _memo((case["name"], "nb", with_gamma), make)


def expect_affine(case, mode):
    def make():
        a = (case["x"], case["scale"], case["shift"], case["res"], mode, case["slope"])
        y = O.affine_act(*a)
        return {"y_aff": (y, O.bound_affine_act(*a)),
                "dz": (O.act_backward(case["dy"], y, mode, case["slope"]), O.bound_act_backward(case["dy"], y, mode, case["slope"]))}
    return _memo((case["name"], "aff", mode), make)


def expect_l2(case):
    def make():
        x, dy = case["x"], case["dy"]
        return {"y_l2": (O.l2_normalize(x), O.bound_l2(x)), "dx_l2": (O.l2_backward(x, dy), O.bound_l2_backward(x, dy)),
                "kind_y": O.kind(O.l2_f32(x)), "kind_dx": O.kind(O.l2_backward_f32(x, dy))}
    return _memo((case["name"], "l2"), make)


def check_l2(case, y, dx):
    """normal rows against oracle and bound; the special rows agree in KIND with the float32 expression
    -> (ratio y, ratio dx) over the normal rows"""
    e = expect_l2(case)
    normal = np.array([r for r in range(case["n"]) if r not in case["special_rows"]])
    sp = np.array(case["special_rows"])
    ry, at = O.compare_rows(y[normal], e["y_l2"][0][normal], e["y_l2"][1][normal])
    assert ry <= 1.0, (case["name"], "y_l2", ry, at)
    rd, at = O.compare_rows(dx[normal], e["dx_l2"][0][normal], e["dx_l2"][1][normal])
    assert rd <= 1.0, (case["name"], "dx_l2", rd, at)
    assert (O.kind(y)[sp] == e["kind_y"][sp]).all(), (case["name"], "kind of y", O.kind(y)[sp], e["kind_y"][sp])
    assert (O.kind(dx)[sp] == e["kind_dx"][sp]).all(), (case["name"], "kind of dx", O.kind(dx)[sp], e["kind_dx"][sp])
    return ry, rd


GIVEN = ("y", "mean", "rstd")       # inputs that a backward's expectation carries along as plain arrays: not outputs


def check(what, got, expect, worst=None, absent=()):
    """every (ref, bound) entry of `expect` against got[name], element by element -> {name: ratio}; asserts ratio <= 1.
    An expected quantity that `got` lacks fails, unless the caller names it in `absent` (an output the call did not ask for)."""
    out = {}
    for key, val in expect.items():
        if key in GIVEN and not isinstance(val, tuple):
            continue
        if key in absent:
            assert key not in got, (what, key, "named absent but present")
            continue
        assert key in got, (what, key, "missing from the outputs")
        if not isinstance(val, tuple):
            assert int(got[key]) == int(val), (what, key, got[key], val)
            continue
        g = np.asarray(got[key], np.float64).reshape(np.shape(val[0]))
        ratio, at = O.compare_rows(g, val[0], val[1])
        out[key] = ratio
        if worst is not None:
            worst[key] = max(worst.get(key, 0.0), ratio if np.isfinite(ratio) else 1e30)
        assert ratio <= 1.0, (what, key, ratio, at, None if at is None else (float(g[at]), float(np.asarray(val[0])[at]),
                                                                               float(np.asarray(val[1])[at])))
    return out
