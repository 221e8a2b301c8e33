"""Float64 statement of the normalisation kernels (apr_amd/csrc/norm.hip) and the per-element float32 bounds they are held to.
numpy only: no torch, no GPU.  tests/norm_cases.py builds the named inputs, tests/test_norm_oracle_cpu.py shows on the host that
a float32 restatement in the kernels' own order stays inside the bounds and that one-rule mutants of it do not,
tests/test_norm_edges_gpu.py holds the kernels to the same bounds.

The operations
--------------
rows x [n, c]; segments offs = [0, ..., n]; per segment s and column j, over the segment's n_s rows
  m = sum x / n_s,   var = sum (x - m)^2 / n_s (two passes, biased),   rstd = 1 / sqrt(var + eps)
  y = act((x - m) * rstd * gamma + beta + res)             act: 0 none, 1 ReLU, 2 LeakyReLU(slope)
  running: for s in order  rm <- rm (1 - mom) + m_s mom,  rv <- rv (1 - mom) + var_s n_s / (n_s - 1) mom;  counter += nseg
  backward with g = act'(y) dy  (mask read off the forward's OUTPUT: y > 0):
      k1 = mean g,  k2 = mean g xhat,  dx = gamma rstd (g - k1 - xhat k2),  dres = g,
      dgamma = sum over ALL segments of g xhat,  dbeta = sum over all segments of g
eps and slope are the float32 values the library receives.

The bounds (u = 2^-24, one float32 rounding; every term is named where it is added)
---------------------------------------------------------------------------------
The kernels sum x and x^2 in fp64: 256-row block partials, combined per column in a fixed tree.  An element takes part in
at most D = DEPTH0 + ceil(nblk / 4) additions (68 inside a block on the 16-byte form, 4 + 8 * ceil(nblk / 32) <= nblk / 4 + 12
in the combine), so in ANY order of that depth
  |s - sum x| <= D 2^-53 sum |x|,     |s2 - sum x^2| <= D 2^-53 sum x^2              (x^2 is exact in fp64)
* mean:  bm = u |m| + D 2^-53 E|x| + 2^-149                (the float32 rounding of the stored mean, then the sums)
* var:   the one-pass E[x^2] - m^2 loses  canc = 2 (D + 3) 2^-53 E[x^2]  absolutely (both terms are <= E[x^2], the
         division, the square and the difference round once each), then one float32 rounding:
         bv = u var + canc + 2^-149
* rstd:  relative  R = (bv + u (var + eps)) / (2 (var + eps)) + 3 u   (d rstd / rstd = -dv / 2(v + eps); the float32 sum
         v + eps, the square root and the division: correctly rounded on the device, 3 u allows each one full u)
         canc / (var + eps) is the issue's "2^-53 * (terms summed) * E[x^2] / var" term.
* apply, subtract-first (apr_bn_train_fwd, ops.NormFunction):  a = (x - m) rstd gamma
         |gamma| rstd bm                      the stored mean's rounding: ulp(mean) * rstd * |gamma|
       + |a| (R + 2 u)                        rstd, the float32 product rstd * gamma, the float32 difference x - mean
       + 2 u (|a| + |beta| + |res|)           the multiply-add, the residual add
       + u |y|                                LeakyReLU's product
* apply, scale/shift (apr_instance_norm_act[_seg], apr_norm_params): shift = fl(-mean * scale) adds
         u |m| rstd                           the rounding of the shift itself: the 2x of the issue's table
  to the same terms (gamma = 1).
* backward: xhat is formed in float32 from the GIVEN mean / rstd: ex = rstd dm + |xhat| (Rr + 2 u)   (dm, Rr: how far the
  given statistics are from the oracle's; 0 when the test hands the kernel the oracle's own float32 values)
         e1 = u |k1| + Db 2^-53 mean |g|                              k1 stored in float32
         e2 = mean(|g| ex) + u |k2| + Db 2^-53 mean |g xhat|          k2 likewise, through the float32 xhat
         bdx = |gamma| rstd (e1 + |xhat| e2 + ex |k2| + 2 u (|g| + |k1| + |xhat k2|)) + (3 u + Rr) |dx|
         bdgamma = sum |g| ex + u |dgamma| + Db 2^-53 sum |g xhat|,   bdbeta = u |dbeta| + Db 2^-53 sum |g|
  with Db = DEPTH0 + nblk (apr_norm_backward combines its blocks in one chain).
* L2 rows: the float32 sum of squares of c terms takes P = ceil(c / 64) multiply-adds per lane and 6 butterfly steps:
  relative (P + 6) u; see bound_l2 / bound_l2_backward.
"""
import numpy as np

U = 2.0 ** -24
U53 = 2.0 ** -53
TINY = 2.0 ** -149
ROWS = 256
DEPTH0 = 80
MAX_SEG = 32


def _f64(*arrays):
    return tuple(np.asarray(a, np.float64) for a in arrays)


def cdiv(a, b):
    return -(-int(a) // int(b))


def nblocks(n):
    return cdiv(n, ROWS)


def one(n):
    return [0, int(n)]


# ------------------------------------------------------------------------------------------------------- statistics
def seg_stats(x, offs, eps):
    """-> mean, var, rstd, each [nseg, c] (two-pass, biased)"""
    x = np.asarray(x, np.float64)
    eps = float(np.float32(eps))
    nseg = len(offs) - 1
    mean = np.empty((nseg, x.shape[1]))
    var = np.empty_like(mean)
    for s in range(nseg):
        seg = x[offs[s]:offs[s + 1]]
        mean[s] = seg.mean(0)
        var[s] = ((seg - mean[s]) ** 2).mean(0)
    with np.errstate(divide="ignore"):
        rstd = 1.0 / np.sqrt(var + eps)
    return mean, var, rstd


def stat_bounds(x, offs, eps):
    """-> dict of [nseg, c] arrays: bm (mean), bv (var), R (relative, rstd), Ex2, absm"""
    x = np.asarray(x, np.float64)
    eps = float(np.float32(eps))
    mean, var, rstd = seg_stats(x, offs, eps)
    nseg = len(offs) - 1
    bm, bv, R = np.empty_like(mean), np.empty_like(mean), np.empty_like(mean)
    for s in range(nseg):
        seg = x[offs[s]:offs[s + 1]]
        D = DEPTH0 + cdiv(nblocks(len(seg)), 4)
        ex2 = (seg * seg).mean(0)
        bm[s] = U * np.abs(mean[s]) + D * U53 * np.abs(seg).mean(0) + TINY      # stored mean's rounding; the fp64 sums
        canc = 2.0 * (D + 3) * U53 * ex2                                           # one-pass cancellation
        bv[s] = U * var[s] + canc + TINY                                           # stored variance's rounding
        with np.errstate(divide="ignore", invalid="ignore"):
            R[s] = np.where(var[s] + eps > 0, (bv[s] + U * (var[s] + eps)) / (2.0 * (var[s] + eps)), np.inf) + 3 * U
    return {"bm": bm, "bv": bv, "R": R, "mean": mean, "var": var, "rstd": rstd}


def col_sums(x):
    return np.asarray(x, np.float64).sum(0)


def bound_col_sums(x):
    x = np.asarray(x, np.float64)
    D = DEPTH0 + cdiv(nblocks(len(x)), 4)
    return U * np.abs(x.sum(0)) + D * U53 * np.abs(x).sum(0) + TINY


def norm_params(x, eps):
    """(scale, shift) of apr_norm_params: rstd, -mean * rstd"""
    mean, _, rstd = seg_stats(x, one(len(x)), eps)
    return rstd[0], -mean[0] * rstd[0]


def bound_norm_params(x, eps):
    b = stat_bounds(x, one(len(x)), eps)
    r, m = b["rstd"][0], np.abs(b["mean"][0])
    return r * b["R"][0], r * b["bm"][0] + m * r * (b["R"][0] + U) + TINY


# -------------------------------------------------------------------------------------------------------- activation
def act(v, mode, slope=0.0):
    v = np.asarray(v, np.float64)
    if mode == 1:
        return np.maximum(v, 0.0)
    if mode == 2:
        return np.where(v > 0, v, v * float(np.float32(slope)))
    return v


def act_backward(dy, y, mode, slope=0.0):
    """dz = dy where y > 0 (or mode 0), dy * slope (mode 2) or 0 (mode 1) elsewhere: y == 0 takes the `elsewhere` side"""
    dy, y = _f64(dy, y)
    if mode == 0:
        return dy.copy()
    return np.where(y > 0, dy, dy * float(np.float32(slope)) if mode == 2 else 0.0)


def bound_act_backward(dy, y, mode, slope=0.0):
    dy, y = _f64(dy, y)
    if mode != 2:
        return np.zeros_like(dy)
    return np.where(y > 0, 0.0, U * np.abs(dy * float(np.float32(slope))) + TINY)    # the one float32 product


def affine_act(x, scale, shift, res, mode, slope=0.0):
    v = np.asarray(x, np.float64)
    if scale is not None:
        v = v * np.asarray(scale, np.float64)
    if shift is not None:
        v = v + np.asarray(shift, np.float64)
    if res is not None:
        v = v + np.asarray(res, np.float64)
    return act(v, mode, slope)


def bound_affine_act(x, scale, shift, res, mode, slope=0.0):
    """product, two sums, LeakyReLU's product: one u each on the magnitudes they round"""
    x = np.asarray(x, np.float64)
    xs = np.abs(x * (1.0 if scale is None else np.asarray(scale, np.float64)))
    sh = np.zeros(x.shape[1]) if shift is None else np.abs(np.asarray(shift, np.float64))
    rs = 0.0 if res is None else np.abs(np.asarray(res, np.float64))
    y = np.abs(affine_act(x, scale, shift, res, mode, slope))
    return 2 * U * (xs + sh + rs) + U * (xs + y) + TINY


# ----------------------------------------------------------------------------------------------------------- forward
def _rows_of(v, offs, s):
    return None if v is None else np.asarray(v, np.float64)[offs[s]:offs[s + 1]]


def pre_activation(x, offs, eps, gamma=None, beta=None, res=None):
    """(x - m) rstd gamma + beta + res per segment, float64"""
    x = np.asarray(x, np.float64)
    mean, _, rstd = seg_stats(x, offs, eps)
    g = np.ones(x.shape[1]) if gamma is None else np.asarray(gamma, np.float64)
    b = np.zeros(x.shape[1]) if beta is None else np.asarray(beta, np.float64)
    v = np.empty_like(x)
    for s in range(len(offs) - 1):
        a, e = offs[s], offs[s + 1]
        v[a:e] = (x[a:e] - mean[s]) * rstd[s] * g + b
    if res is not None:
        v = v + np.asarray(res, np.float64)
    return v


def norm_act(x, offs, eps, gamma=None, beta=None, res=None, mode=0, slope=0.0):
    return act(pre_activation(x, offs, eps, gamma, beta, res), mode, slope)


def bound_norm_act(x, offs, eps, gamma=None, beta=None, res=None, mode=0, slope=0.0, form="subtract"):
    """form "subtract": (x - mean) * (rstd gamma) + beta;  "scaleshift": x * scale + shift with shift = fl(-mean * scale)"""
    assert form in ("subtract", "scaleshift")
    x = np.asarray(x, np.float64)
    b = stat_bounds(x, offs, eps)
    g = np.ones(x.shape[1]) if gamma is None else np.abs(np.asarray(gamma, np.float64))
    be = np.zeros(x.shape[1]) if beta is None else np.abs(np.asarray(beta, np.float64))
    r = 0.0 if res is None else np.abs(np.asarray(res, np.float64))
    y = np.abs(norm_act(x, offs, eps, gamma, beta, res, mode, slope))
    out = np.empty_like(x)
    for s in range(len(offs) - 1):
        a, e = offs[s], offs[s + 1]
        rstd, m = b["rstd"][s], b["mean"][s]
        an = np.abs(x[a:e] - m) * rstd * g
        t = g * rstd * b["bm"][s]                                   # ulp(mean) * rstd * |gamma|
        t = t + an * (b["R"][s] + 2 * U)                            # rstd, rstd * gamma, x - mean
        if form == "scaleshift":
            t = t + U * np.abs(m) * rstd                            # the rounding of shift = -mean * scale
        out[a:e] = t + 2 * U * (an + be)
    return out + 2 * U * r + U * y + TINY


def pre_margin(x, offs, eps, gamma=None, beta=None, res=None, form="subtract"):
    """|pre-activation| / bound: a case is decision-safe when this is > 1 (or the pre-activation is an exact planted 0)"""
    v = pre_activation(x, offs, eps, gamma, beta, res)
    bd = bound_norm_act(x, offs, eps, gamma, beta, res, 0, 0.0, form)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(v) / bd


def running(rm, rv, count, x, offs, eps, momentum):
    """-> rm, rv, count after the segments' forward calls in order"""
    rm, rv = _f64(rm, rv)
    mean, var, _ = seg_stats(x, offs, eps)
    mom = float(np.float32(momentum))
    for s in range(len(offs) - 1):
        ns = offs[s + 1] - offs[s]
        rm = rm * (1.0 - mom) + mean[s] * mom
        rv = rv * (1.0 - mom) + var[s] * (ns / (ns - 1.0) if ns > 1 else 1.0) * mom
    return rm, rv, int(count) + len(offs) - 1


def bound_running(rm, rv, x, offs, eps, momentum):
    """E <- E (1 - mom) + mom * (statistic's bound) + 4 u (|r| |1 - mom| + |stat| mom): 1 - mom, two products, the sum;
    the unbiased variance adds three roundings (two int -> float, the quotient, the product: 4 u var) before n / (n - 1)"""
    rm, rv = _f64(rm, rv)
    b = stat_bounds(x, offs, eps)
    mom = float(np.float32(momentum))
    em, ev = np.zeros_like(rm), np.zeros_like(rv)
    for s in range(len(offs) - 1):
        ns = offs[s + 1] - offs[s]
        k = ns / (ns - 1.0) if ns > 1 else 1.0
        unb = b["var"][s] * k
        em = em * abs(1 - mom) + mom * b["bm"][s] + 4 * U * (np.abs(rm) * abs(1 - mom) + np.abs(b["mean"][s]) * mom) + TINY
        ev = ev * abs(1 - mom) + mom * (b["bv"][s] + 4 * U * b["var"][s]) * k + 4 * U * (np.abs(rv) * abs(1 - mom) + unb * mom) + TINY
        rm = rm * (1.0 - mom) + b["mean"][s] * mom
        rv = rv * (1.0 - mom) + unb * mom
    return em, ev


# ---------------------------------------------------------------------------------------------------------- backward
def norm_backward(x, g, offs, mean, rstd, gamma=None):
    """g: the gradient behind the activation (already masked).  mean / rstd [nseg, c]: the statistics HANDED to the
    backward.  -> dx, dgamma, dbeta (float64)"""
    x, g, mean, rstd = _f64(x, g, mean, rstd)
    gam = np.ones(x.shape[1]) if gamma is None else np.asarray(gamma, np.float64)
    dx = np.empty_like(x)
    dg, db = np.zeros(x.shape[1]), np.zeros(x.shape[1])
    for s in range(len(offs) - 1):
        a, e = offs[s], offs[s + 1]
        xh = (x[a:e] - mean[s]) * rstd[s]
        k1, k2 = g[a:e].mean(0), (g[a:e] * xh).mean(0)
        dx[a:e] = gam * rstd[s] * (g[a:e] - k1 - xh * k2)
        dg += (g[a:e] * xh).sum(0)
        db += g[a:e].sum(0)
    return dx, dg, db


def bound_norm_backward(x, g, offs, mean, rstd, gamma=None, dm=None, Rr=None, chain=False):
    """dm [nseg, c] / Rr [nseg, c]: bounds on |given mean - `mean`| and the relative error of the given rstd (None: 0).
    chain: apr_norm_backward's single chain over the blocks (depth nblk) instead of the stride-32 tree"""
    x, g, mean, rstd = _f64(x, g, mean, rstd)
    gam = np.ones(x.shape[1]) if gamma is None else np.abs(np.asarray(gamma, np.float64))
    dx, _, _ = norm_backward(x, g, offs, mean, rstd, gamma)
    bdx = np.empty_like(x)
    bdg, bdb = np.zeros(x.shape[1]), np.zeros(x.shape[1])
    dg, db = np.zeros(x.shape[1]), np.zeros(x.shape[1])
    for s in range(len(offs) - 1):
        a, e = offs[s], offs[s + 1]
        nb = nblocks(e - a)
        Db = DEPTH0 + (nb if chain else cdiv(nb, 4))
        d = 0.0 if dm is None else np.asarray(dm, np.float64)[s]
        rr = 0.0 if Rr is None else np.asarray(Rr, np.float64)[s]
        xh = np.abs((x[a:e] - mean[s]) * rstd[s])
        ag = np.abs(g[a:e])
        ex = rstd[s] * d + xh * (rr + 2 * U)
        k1, k2 = np.abs(g[a:e].mean(0)), np.abs((g[a:e] * (x[a:e] - mean[s]) * rstd[s]).mean(0))
        e1 = U * k1 + Db * U53 * ag.mean(0) + TINY
        e2 = (ag * ex).mean(0) + U * k2 + Db * U53 * (ag * xh).mean(0) + TINY
        bdx[a:e] = gam * rstd[s] * (e1 + xh * e2 + ex * k2 + 2 * U * (ag + k1 + xh * k2)) + (3 * U + rr) * np.abs(dx[a:e]) + TINY
        bdg += (ag * ex).sum(0) + Db * U53 * (ag * xh).sum(0)
        bdb += Db * U53 * ag.sum(0)
        dg += (g[a:e] * (x[a:e] - mean[s]) * rstd[s]).sum(0)
        db += g[a:e].sum(0)
    return bdx, bdg + U * np.abs(dg) + TINY, bdb + U * np.abs(db) + TINY


# ------------------------------------------------------------------------------------------------------- L2 per row
def l2_normalize(x):
    x = np.asarray(x, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return x / np.sqrt((x * x).sum(1, keepdims=True))


def bound_l2(x):
    """sum of squares in float32: P multiply-adds per lane + 6 butterfly steps, relative (P + 6) u on ss, half of it on the
    norm; the square root and the division one u each (2 u allowed each)"""
    x = np.asarray(x, np.float64)
    P = cdiv(x.shape[1], 64)
    return np.abs(l2_normalize(x)) * (0.5 * (P + 6) * U + 4 * U) + TINY


def l2_backward(x, dy):
    """dx = (dy - y (y . dy)) / |x|"""
    x, dy = _f64(x, dy)
    with np.errstate(divide="ignore", invalid="ignore"):
        nrm = np.sqrt((x * x).sum(1, keepdims=True))
        y = x / nrm
        return (dy - y * (y * dy).sum(1, keepdims=True)) / nrm


def bound_l2_backward(x, dy):
    """k = (x . dy) / |x|^2:  ek = (P + 6) u sum |x dy| / ss + |k| ((P + 6) u + 4 u)   (the dot, then ss, nrm * nrm, the
    quotient);  dx = (dy - x k) / nrm:  (|x| ek + 2 u |x k| + u |dy - x k|) / nrm + |dx| (0.5 (P + 6) u + 3 u)"""
    x, dy = _f64(x, dy)
    P = cdiv(x.shape[1], 64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ss = (x * x).sum(1, keepdims=True)
        nrm = np.sqrt(ss)
        k = (x * dy).sum(1, keepdims=True) / ss
        ek = (P + 6) * U * np.abs(x * dy).sum(1, keepdims=True) / ss + np.abs(k) * ((P + 6) * U + 4 * U)
        dx = l2_backward(x, dy)
        return (np.abs(x) * ek + 2 * U * np.abs(x * k) + U * np.abs(dy - x * k)) / nrm + np.abs(dx) * (0.5 * (P + 6) * U + 3 * U) + TINY


def l2_f32(x):
    """the reference's float32 expression x / norm(x) (FCGF's final row normalisation) restated in float32: what a zero
    row (0 / 0 = NaN), a row whose squares overflow (x / inf = 0) and a row of denormals (squares underflow: x / 0 = inf)
    yield.  Only the KIND of each element is taken from this."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        ss = np.zeros(len(x), np.float32)
        for j in range(x.shape[1]):
            ss = (ss + x[:, j] * x[:, j]).astype(np.float32)
        return x / np.sqrt(ss)[:, None]


def l2_backward_f32(x, dy):
    """the kernel's float32 expression (dy - x k) / nrm, k = (x . dy) / (nrm * nrm), for the kind of the special rows"""
    x, dy = np.asarray(x, np.float32), np.asarray(dy, np.float32)
    with np.errstate(all="ignore"):
        ss = np.zeros(len(x), np.float32)
        dot = np.zeros(len(x), np.float32)
        for j in range(x.shape[1]):
            ss = (ss + x[:, j] * x[:, j]).astype(np.float32)
            dot = (dot + x[:, j] * dy[:, j]).astype(np.float32)
        nrm = np.sqrt(ss)
        k = dot / (nrm * nrm)
        return (dy - x * k[:, None]) / nrm[:, None]


def kind(a):
    """0 finite non-zero, 1 zero, 2 +inf, 3 -inf, 4 NaN"""
    a = np.asarray(a, np.float64)
    return np.where(np.isnan(a), 4, np.where(a == np.inf, 2, np.where(a == -np.inf, 3, np.where(a == 0, 1, 0))))


# ----------------------------------------------------------------------------------------------------------- compare
def compare_rows(got, ref, bound):
    """-> (worst |got - ref| / bound, first offending index or None).  Where the bound is 0 the value must be equal; a NaN or
    inf in `got` against a finite reference always fails (ratio inf), whatever the bound."""
    got, ref, bound = _f64(got, ref, bound)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.size == 0:
        return 0.0, None
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(got - ref)
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(got) & np.isfinite(ref), ratio, np.inf)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    bad = np.argwhere(ratio > 1.0)
    first = None if len(bad) == 0 else tuple(int(v) for v in bad[0])
    return float(ratio.max()), first
