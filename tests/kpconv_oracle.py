"""Float64 NumPy statement of the rigid KPConv (apr_amd/csrc/kpconv.hip), of the reverse neighbour table
(apr_amd/csrc/revtable.hip) and of the neighbour pools, with per-element error bounds for a float32 evaluation.
numpy only, no torch.

Contract, as the kernels state it
---------------------------------
q [nq, 3], s [ns, 3], nbr [nq, H] integers, x [ns, cin], kp [15, 3], extent > 0.
* A neighbour is REAL iff 0 <= nbr[q, h] < ns.  Every other value (ns, negatives, anything > ns) is a padding entry: zero
  feature row, zero influence, not counted.  (The reference only ever produces ns.)
* w[q, k, h] = max(0, 1 - |s[nbr[q, h]] - q - kp[k]| / extent) for a real neighbour, 0 for padding.
* num[q] = max(1, #{h real : sum_c x[nbr[q, h], c] > 0}): the float64 feature sum, strictly positive; it does not depend
  on w (a neighbour beyond every kernel point still counts) and a support listed twice counts twice.
* wf[q, k * cin + c] = (1 / num[q]) * sum_h w[q, k, h] * x[nbr[q, h], c];   out = wf @ W.reshape(15 * cin, cout).
* backward (num and w are piecewise constant in x): with dwf = d_out @ W.reshape(15 * cin, cout)^T,
  contrib[q * H + h, c] = (1 / num[q]) * sum_k w[q, k, h] * dwf[q, k * cin + c]  for a real neighbour (the kernels leave
  the rows of padding neighbours untouched; here they are 0), d_x[r] = sum of the contrib rows that point at r,
  d_W = wf^T @ d_out.
* reverse table: the flat positions t = q * H + h sorted by the row they point at (stable: ascending t inside a row),
  padding positions last; start[r] .. start[r + 1] is the run of row r, start[ns] = number of real entries.
* pools: x_pad = x plus a zero shadow row that every padding entry addresses; max_pool takes the maximum over h and the
  FIRST h that attains it; its gradient goes to that neighbour alone (to nobody when it is a shadow entry);
  closest_pool takes h = 0.

Error bounds (u = 2^-24 unit roundoff, eps32 = 2 u; every basic fp32 operation rounds once, relative error <= u)
-------------------------------------------------------------------------------------------------------------
Influence.  With D = s - q and e = D - kp:  fl(D) is off by <= u |D| per component, fl(e) by <= u (|e| + |D|) in norm.
d2 = ex^2 + ey^2 + ez^2 is a sum of three positive products (three roundings at most on any path: relative 3 u), the
square root halves that and rounds (an implementation within 1 ulp: 2 u): the computed distance d' differs from
d = |e| by <= u (|e| + |D|) + 3.5 u d.  t = d' * fl(1 / extent) adds 2 u d / extent, w' = fl(1 - t) adds u w:
    |w' - w| <= u (6.5 d + |D|) / extent + u w <= 7.5 u (|D| + |kp|) / extent + u w         (d <= |D| + |kp|)
           = eps32 * (B_W * geo + w / 2),    B_W = 3.75,    geo[q, k, h] = (|s - q| + |kp[k]|) / extent.
The absolute error of w does NOT shrink with w: next to the edge of a kernel point's ball it is all there is.  The clamp
max(0, .) cannot enlarge it, but it decides which terms exist: fp32 may see a small positive w where the exact one is 0
as long as d < extent * (1 + M).  Next to the edge |D| <= extent + |kp| and the error of t is
u (6.5 d + |D|) / extent <= u (7.5 + |kp| / extent) <= 9 u for |kp| <= sqrt(3), extent = 1.2; M = 2^-20 = 16 u covers it.
Beyond that distance the computed w is 0 exactly, as the true one.

wf.  sum_h w' x over n non-zero terms (n[q, k] = #{h real : d < extent (1 + M)}; zero terms add exactly), in any order, fused
or not: <= n u sum |w' x| (n fused steps, or one product rounding and n - 1 additions).  The factor 1 / num:
fl(1 / num) and one product, 2 u.  Together with the u w of the influence itself the relative part is (n + 3) u = eps32 * A, A = (n + 3) / 2:
    |wf' - wf| <= eps32 * ( A * sum_h w |x|  +  B_W * sum_{h real} geo |x| [d < extent (1 + M)] ) / num * (1 + 2^-10)
the last factor for the products of two errors.  A and B_W come from the count of rounding steps above, not from any
kernel; a bound of 0 (no neighbour inside any ball, or zero features) means the value must be exactly 0.

contrib.  g = fl(dwf * fl(1 / num)): 2 u; sum over the m[q, h] <= 15 kernel points with d < extent (1 + M): m u.
    |contrib' - contrib| <= eps32 * sum_k ( (m + 3) / 2 * w + B_W * geo [d < extent (1 + M)] ) |dwf| / num * (1 + 2^-10)

d_x.  The rows of a support point are added one after the other (n_r rows: n_r - 1 roundings, n_r for an atomic add into
a zeroed row - the first is exact as well): the sum of the rows' bounds plus (n_r - 1) u sum_rows (|contrib| + bound).
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)      # 2^-23
B_W = 3.75
M_EDGE = 2.0 ** -20
SECOND_ORDER = 1.0 + 2.0 ** -10
KP = 15


def _f64(*arrays):
    return [np.asarray(a, np.float64) for a in arrays]


def real_mask(nbr, ns):
    nbr = np.asarray(nbr, np.int64)
    return (nbr >= 0) & (nbr < ns)


def geometry(q, s, nbr, kp, extent):
    """-> w [nq, 15, H], d [nq, 15, H] (distance to the kernel point; arbitrary for padding), real [nq, H],
    idx [nq, H] (0 for padding), dist [nq, H] = |s - q|."""
    q, s, kp = _f64(q, s, kp)
    real = real_mask(nbr, len(s))
    idx = np.where(real, np.asarray(nbr, np.int64), 0)
    diff = s[idx] - q[:, None, :]                                              # [nq, H, 3]
    d = np.linalg.norm(diff[:, None, :, :] - kp[None, :, None, :], axis=-1)    # [nq, 15, H]
    w = np.maximum(0.0, 1.0 - d / float(extent)) * real[:, None, :]
    return w, d, real, idx, np.linalg.norm(diff, axis=-1)


def neighbour_count(nbr, x):
    x, = _f64(x)
    real = real_mask(nbr, len(x))
    idx = np.where(real, np.asarray(nbr, np.int64), 0)
    raw = (real & (x.sum(1)[idx] > 0)).sum(1)
    return np.maximum(raw, 1).astype(np.float64), raw


def weighted(q, s, nbr, x, kp, extent):
    """-> wf [nq, 15 * cin], num [nq], w [nq, 15, H]"""
    x, = _f64(x)
    w, _, real, idx, _ = geometry(q, s, nbr, kp, extent)
    num, _ = neighbour_count(nbr, x)
    xg = x[idx] * real[:, :, None]
    wf = np.einsum("qkh,qhc->qkc", w, xg) / num[:, None, None]
    return wf.reshape(len(wf), -1), num, w


def forward(q, s, nbr, x, kp, extent, W):
    W, = _f64(W)
    wf, _, _ = weighted(q, s, nbr, x, kp, extent)
    return wf @ W.reshape(-1, W.shape[-1])


def contrib(q, s, nbr, x, kp, extent, dwf):
    """dwf [nq, 15 * cin] -> [nq * H, cin]; the rows of padding neighbours are 0"""
    dwf, = _f64(dwf)
    nq, H = np.asarray(nbr).shape
    w, _, _, _, _ = geometry(q, s, nbr, kp, extent)
    num, _ = neighbour_count(nbr, x)
    g = dwf.reshape(nq, KP, -1) / num[:, None, None]
    return np.einsum("qkh,qkc->qhc", w, g).reshape(nq * H, -1)


def scatter_rows(rows, nbr, ns):
    """sum of the rows [nq * H, c] per support row they point at -> [ns, c]"""
    flat = np.asarray(nbr, np.int64).reshape(-1)
    real = (flat >= 0) & (flat < ns)
    out = np.zeros((ns, rows.shape[1]), np.float64)
    np.add.at(out, flat[real], rows[real])
    return out


def d_x_from_dwf(q, s, nbr, x, kp, extent, dwf):
    return scatter_rows(contrib(q, s, nbr, x, kp, extent, dwf), nbr, len(np.asarray(s)))


def d_x(q, s, nbr, x, kp, extent, W, d_out):
    W, d_out = _f64(W, d_out)
    return d_x_from_dwf(q, s, nbr, x, kp, extent, d_out @ W.reshape(-1, W.shape[-1]).T)


def d_W(q, s, nbr, x, kp, extent, d_out):
    d_out, = _f64(d_out)
    wf, _, _ = weighted(q, s, nbr, x, kp, extent)
    return (wf.T @ d_out).reshape(KP, -1, d_out.shape[1])


# ----------------------------------------------------------------------------------------------------------- bounds
def _edge_terms(q, s, nbr, kp, extent):
    w, d, real, idx, dist = geometry(q, s, nbr, kp, extent)
    kp, = _f64(kp)
    inside = real[:, None, :] & (d < float(extent) * (1.0 + M_EDGE))           # [nq, 15, H]
    geo = (dist[:, None, :] + np.linalg.norm(kp, axis=1)[None, :, None]) / float(extent)
    return w, inside, geo * inside, real, idx


def bound_weighted(q, s, nbr, x, kp, extent):
    """per-element bound [nq, 15 * cin] of |fp32 wf - wf| (derivation: module docstring)"""
    x, = _f64(x)
    w, inside, geo, real, idx = _edge_terms(q, s, nbr, kp, extent)
    num, _ = neighbour_count(nbr, x)
    ax = np.abs(x[idx]) * real[:, :, None]                                     # [nq, H, cin]
    a = (inside.sum(2) + 3.0) / 2.0                                            # [nq, 15]
    rel = a[:, :, None] * np.einsum("qkh,qhc->qkc", w, ax)
    edge = B_W * np.einsum("qkh,qhc->qkc", geo, ax)
    b = EPS32 * SECOND_ORDER * (rel + edge) / num[:, None, None]
    return b.reshape(len(b), -1)


def bound_contrib(q, s, nbr, x, kp, extent, dwf):
    """per-element bound [nq * H, cin] of the contribution rows (0 for padding rows)"""
    dwf, = _f64(dwf)
    nq, H = np.asarray(nbr).shape
    w, inside, geo, _, _ = _edge_terms(q, s, nbr, kp, extent)
    num, _ = neighbour_count(nbr, x)
    ag = np.abs(dwf.reshape(nq, KP, -1))
    a = (inside.sum(1) + 3.0) / 2.0                                            # [nq, H]
    rel = a[:, :, None] * np.einsum("qkh,qkc->qhc", w, ag)
    edge = B_W * np.einsum("qkh,qkc->qhc", geo, ag)
    return (EPS32 * SECOND_ORDER * (rel + edge) / num[:, None, None]).reshape(nq * H, -1)


def bound_dx(q, s, nbr, x, kp, extent, dwf):
    """per-element bound [ns, cin] of d_x summed from fp32 contribution rows in any order"""
    ns = len(np.asarray(s))
    rows = np.abs(contrib(q, s, nbr, x, kp, extent, dwf))
    bc = bound_contrib(q, s, nbr, x, kp, extent, dwf)
    flat = np.asarray(nbr, np.int64).reshape(-1)
    n_rows = np.bincount(flat[(flat >= 0) & (flat < ns)], minlength=ns).astype(np.float64)
    summed = scatter_rows(rows + bc, nbr, ns)
    return scatter_rows(bc, nbr, ns) + 0.5 * EPS32 * np.maximum(n_rows - 1.0, 0.0)[:, None] * summed


def compare_rows(got, ref, bound):
    """-> (worst |got - ref| / bound, first offending (row, col) or None).  Where the bound is 0 the value must be equal
    (ratio inf otherwise); a NaN (or inf) in `got` always fails."""
    got, ref, bound = _f64(got, ref, bound)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    if ratio.size == 0:
        return 0.0, None
    bad = np.argwhere(ratio > 1.0)
    first = None if len(bad) == 0 else tuple(int(v) for v in bad[0])
    return float(ratio.max()), first


# ---------------------------------------------------------------------------------------------------- reverse table
def reverse_table(nbr, ns):
    """-> rev_t i32 [nq * H], start i32 [ns + 1]"""
    flat = np.asarray(nbr, np.int64).reshape(-1)
    key = np.where((flat >= 0) & (flat < ns), flat, ns)
    rev_t = np.argsort(key, kind="stable").astype(np.int32)
    start = np.searchsorted(key[rev_t], np.arange(ns + 1), side="left").astype(np.int32)
    return rev_t, start


# ------------------------------------------------------------------------------------------------------------ pools
def _padded(x, inds):
    x, = _f64(x)
    ns = len(x)
    inds = np.asarray(inds, np.int64)
    real = (inds >= 0) & (inds < ns)
    return np.concatenate([x, np.zeros((1, x.shape[1]))], 0)[np.where(real, inds, ns)], real       # [nq, H, c]


def max_pool(x, inds):
    """-> out [nq, c], amax [nq, c] (the first h that attains the maximum)"""
    g, _ = _padded(x, inds)
    return g.max(1), g.argmax(1)


def closest_pool(x, inds):
    g, _ = _padded(x, inds[:, :1])
    return g[:, 0]


def max_pool_grad(x, inds, dout):
    dout, = _f64(dout)
    ns, c = np.asarray(x).shape
    _, amax = max_pool(x, inds)
    inds = np.asarray(inds, np.int64)
    tgt = np.take_along_axis(inds, amax, axis=1)                                # [nq, c]
    dx = np.zeros((ns, c))
    for col in range(c):
        ok = (tgt[:, col] >= 0) & (tgt[:, col] < ns)
        np.add.at(dx[:, col], tgt[ok, col], dout[ok, col])
    return dx


def closest_pool_grad(x, inds, dout):
    dout, = _f64(dout)
    ns, c = np.asarray(x).shape
    first = np.asarray(inds, np.int64)[:, 0]
    ok = (first >= 0) & (first < ns)
    dx = np.zeros((ns, c))
    np.add.at(dx, first[ok], dout[ok])
    return dx
