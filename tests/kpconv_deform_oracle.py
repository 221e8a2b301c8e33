"""Float64 NumPy statement of the deformable / modulated KPConv (apr_amd/csrc/kpconv_deform.hip; the reference is
Predator_APR/models/blocks.py:229-374 with deformable=True), with its intermediates and per-element error bounds for a
float32 evaluation.  numpy only.  The rigid pieces (offset_conv, the scatter over the neighbour table, compare_rows) come
from tests/kpconv_oracle.py.

Contract
--------
q [nq, 3], s [ns, 3], nbr [nq, H], x [ns, cin], dkp [nq, 15, 3], mod [nq, 15] or None (= 1), extent > 0.
* real neighbour iff 0 <= nbr < ns; padding: zero features, the point (1e6, 1e6, 1e6).
* D[q, h] = s[nbr] - q (padding: 1e6 - q), diff[q, h, k] = D - dkp[q, k], d2 = |diff|^2, d = sqrt(d2),
  w[q, k, h] = max(0, 1 - d / extent) for real neighbours, 0 for padding.
* min_d2[q, k] = min over all H slots of d2 (padding included).
* in_range[q, h] = real and d2[q, h, k] < extent^2 for some k;  num[q] = max(1, #{h in range : sum_c x[nbr, c] > 0}).
* S[q, k, c] = sum_h w x[nbr] / num;  wf[q, k cin + c] = mod[q, k] S[q, k, c];  out = wf @ W.reshape(15 cin, cout).
* backward, dwf = d_out @ W2^T, num and in_range constant:
  contrib[(q, h), c] = sum_k mod w dwf[q, k, c] / num (real; padding rows 0 here, untouched by the kernel),
  P[q, h, k] = <x[nbr[q, h]], dwf[q, k, :]>,  d_mod[q, k] = sum_h w P / num,
  d_dkp[q, k] = mod / num * sum_{h real, 0 < d < extent} diff / (d extent) * P       (d = 0 contributes 0: the reference
  gives NaN there), d_W = wf^T d_out.
* the module chain: of = rigid KPConv(x; W_off) + b_off; offsets = of[:, :45].reshape(-1, 15, 3); dkp = kp + extent *
  offsets; mod = 2 sigmoid(of[:, 45:]) when modulated.  d_of[:, :45] = extent * d_dkp, d_of[:, 45:] = d_mod * mod * (1 -
  mod / 2); d_b_off = column sums; d_W_off and the second part of d_x through the rigid backward.

Error bounds (u = 2^-24, eps32 = 2 u; the counting of tests/kpconv_oracle.py, section 22 of DESIGN)
----------------------------------------------------------------------------------------------
The cases keep |d / extent - 1| >= 1e-3 for every real (q, h, k): a float32 d differs from d by at most
u (|D| + 4.5 d) (section 22), far below that margin, so in_range, the count and the set of non-zero influences are the same
in float32 and here.
Influence: |w' - w| <= eps32 (B_W geo + w / 2), geo = (|D| + |dkp[q, k]|) / extent: section 22 with |dkp| for |kp|.
wf: section 22's (n + 3) u for the sum over n terms, fl(1 / num) and its product, and ONE MORE eps32 for the product with
mod:  |wf' - wf| <= eps32 |mod| ((n + 3) / 2 + 1) sum_h w |x| + B_W sum_h geo |x| [inside]) / num (1 + 2^-10).
min_d2: a component of diff is off by <= u (|e_i| + |D_i|) (two subtractions), its square by twice that times |e_i|, the
three products and two additions add 3 u d2:  b_h = u (2 sum_i |e_i| (|e_i| + |D_i|) + 3 d2) (1 + 2^-10).  The minimum of
perturbed values moves by at most the largest b_h among the slots that can become the minimum (d2_h - b_h <= min_h (d2_h
+ b_h)).
contrib: g = fl(dwf fl(mod fl(1 / num))): 3 u; the sum over the m kernel points inside: m u; the influence's own u w:
  |contrib' - contrib| <= eps32 sum_k |mod| ((m + 4) / 2 w + B_W geo [inside]) |dwf| / num (1 + 2^-10).
P: a sum of cin products in any order, fused or not: |P' - P| <= cin u Pabs, Pabs = sum_c |x| |dwf|.
d_mod: terms w' P' (one product each), n of them in any order, fl(1 / num) and its product:
  |d_mod' - d_mod| <= ( sum_h (eps32 (B_W geo + w / 2) |P| + w cin u Pabs) + (n + 3) u sum_h w |P| ) / num (1 + 2^-10).
d_dkp, PER TERM (the terms carry 1 / d): t_i = e_i P / (d extent).  e_i is off by u (|e_i| + |D_i|); d' by
u (|e| + |D|) + 3.5 u d (section 22); d extent, the division and the product with e_i round once each (3 u):
  b_t,i = u ( (|e_i| + |D_i|) |P| / (d extent) + |e_i| / (d extent) (((|e| + |D|) / d + 6.5) |P| + cin Pabs) ).
The n terms are summed in some order (n u) and scaled by fl(mod fl(1 / num)) with one product (3 u):
  |d_dkp' - d_dkp| <= |mod| / num ( sum_h b_t + (n + 3) u sum_h |t| ) (1 + 2^-10).
The cases keep d >= 0.05 extent for every in-ball triple, so (|e| + |D|) / d stays below ~100.
"""
import numpy as np

import kpconv_oracle as O

EPS32, B_W, M_EDGE, SECOND_ORDER, KP = O.EPS32, O.B_W, O.M_EDGE, O.SECOND_ORDER, O.KP
U = EPS32 / 2.0
SHADOW = 1e6
MUTANTS = ("rigid_count", "count_no_sum", "min_no_pad", "no_mod", "mod_before_count", "offsets_unscaled", "ddkp_sign",
           "ddkp_no_num", "ddkp_no_mod", "drop_k14", "drop_h64")


def _f64(*a):
    return [np.asarray(v, np.float64) for v in a]


def geometry(q, s, nbr, dkp, extent, mutant=None):
    """-> dict of real [nq, H], idx, D [nq, H, 3], diff [nq, H, 15, 3], d2 / d [nq, H, 15], w [nq, 15, H], in_range [nq, H]"""
    q, s, dkp = _f64(q, s, dkp)
    real = O.real_mask(nbr, len(s))
    if mutant == "drop_h64":
        real = real & (np.arange(real.shape[1])[None, :] < 64)
    idx = np.where(real, np.asarray(nbr, np.int64), 0)
    D = np.where(real[:, :, None], s[idx], SHADOW) - q[:, None, :]
    diff = D[:, :, None, :] - dkp[:, None, :, :]
    d2 = (diff ** 2).sum(-1)
    d = np.sqrt(d2)
    w = (np.maximum(0.0, 1.0 - d / float(extent)) * real[:, :, None]).transpose(0, 2, 1)
    if mutant == "drop_k14":
        w = w.copy()
        w[:, 14, :] = 0.0
    in_range = real & (d2 < float(extent) ** 2).any(-1)
    return dict(real=real, idx=idx, D=D, diff=diff, d2=d2, d=d, w=w, in_range=in_range)


def count(g, x, mod=None, mutant=None, extent=None):
    """-> num [nq] (floored at 1), raw count"""
    x, = _f64(x)
    pos = x.sum(1)[g["idx"]] > 0
    sel = g["in_range"]
    if mutant == "rigid_count":
        sel = g["real"]
    if mutant == "count_no_sum":
        pos = np.ones_like(pos)
    if mutant == "mod_before_count" and mod is not None:
        sel = g["real"] & ((g["d2"] < float(extent) ** 2) & (np.asarray(mod)[:, None, :] != 0)).any(-1)
    raw = (sel & pos).sum(1)
    return np.maximum(raw, 1).astype(np.float64), raw


def _mod(mod, nq, mutant=None):
    if mod is None or mutant == "no_mod":
        return np.ones((nq, KP))
    return np.asarray(mod, np.float64)


def min_d2(q, s, nbr, dkp, extent, mutant=None):
    g = geometry(q, s, nbr, dkp, extent)
    d2 = g["d2"]
    if mutant == "min_no_pad":
        d2 = np.where(g["real"][:, :, None], d2, np.inf)
    return d2.min(1)


def weighted(q, s, nbr, x, dkp, mod, extent, mutant=None):
    """-> wf [nq, 15 cin], S [nq, 15, cin], num [nq], geometry dict"""
    x, = _f64(x)
    g = geometry(q, s, nbr, dkp, extent, mutant)
    num, _ = count(g, x, mod, mutant, extent)
    xg = x[g["idx"]] * g["real"][:, :, None]
    S = np.einsum("qkh,qhc->qkc", g["w"], xg) / num[:, None, None]
    wf = _mod(mod, len(S), mutant)[:, :, None] * S
    return wf.reshape(len(wf), -1), S, num, g


def forward(q, s, nbr, x, dkp, mod, extent, W, mutant=None):
    W, = _f64(W)
    wf, _, _, _ = weighted(q, s, nbr, x, dkp, mod, extent, mutant)
    return wf @ W.reshape(-1, W.shape[-1]), min_d2(q, s, nbr, dkp, extent, mutant)


def contrib(q, s, nbr, x, dkp, mod, extent, dwf, mutant=None):
    dwf, = _f64(dwf)
    nq, H = np.asarray(nbr).shape
    g = geometry(q, s, nbr, dkp, extent, mutant)
    num, _ = count(g, x, mod, mutant, extent)
    gg = dwf.reshape(nq, KP, -1) * _mod(mod, nq, mutant)[:, :, None] / num[:, None, None]
    return np.einsum("qkh,qkc->qhc", g["w"], gg).reshape(nq * H, -1)


def d_x(q, s, nbr, x, dkp, mod, extent, dwf, mutant=None):
    return O.scatter_rows(contrib(q, s, nbr, x, dkp, mod, extent, dwf, mutant), nbr, len(np.asarray(s)))


def _products(g, x, dwf):
    """P [nq, H, 15], Pabs [nq, H, 15]"""
    x, dwf = _f64(x, dwf)
    nq = len(dwf)
    xg = x[g["idx"]] * g["real"][:, :, None]
    dk = dwf.reshape(nq, KP, -1)
    return np.einsum("qhc,qkc->qhk", xg, dk), np.einsum("qhc,qkc->qhk", np.abs(xg), np.abs(dk))


def _ddkp_terms(g, P, extent):
    """t [nq, H, 15, 3] (0 outside 0 < d < extent or for padding), the mask of the terms that exist"""
    d = g["d"]
    live = g["real"][:, :, None] & (d > 0) & (d < float(extent))
    safe = np.where(live, d, 1.0)
    t = g["diff"] * (P / (safe * float(extent)) * live)[..., None]
    return t, live


def d_geom(q, s, nbr, x, dkp, mod, extent, dwf, mutant=None):
    """-> d_dkp [nq, 15, 3], d_mod [nq, 15]"""
    g = geometry(q, s, nbr, dkp, extent, mutant)
    num, _ = count(g, x, mod, mutant, extent)
    P, _ = _products(g, x, dwf)
    m = _mod(mod, len(num), mutant)
    dm = np.einsum("qkh,qhk->qk", g["w"], P) / num[:, None]
    t, _ = _ddkp_terms(g, P, extent)
    dd = t.sum(1)
    if mutant == "drop_k14":
        dd[:, 14] = 0.0
    if mutant != "ddkp_no_num":
        dd = dd / num[:, None, None]
    if mutant != "ddkp_no_mod":
        dd = dd * m[:, :, None]
    if mutant == "ddkp_sign":
        dd = -dd
    return dd, dm


def d_W(q, s, nbr, x, dkp, mod, extent, d_out, mutant=None):
    d_out, = _f64(d_out)
    wf, _, _, _ = weighted(q, s, nbr, x, dkp, mod, extent, mutant)
    return (wf.T @ d_out).reshape(KP, -1, d_out.shape[1])


def deformed_points(kp, offsets, extent, mutant=None):
    """dkp = kp + extent * offsets (blocks.py:258, 279)"""
    kp, offsets = _f64(kp, offsets)
    return kp[None] + (1.0 if mutant == "offsets_unscaled" else float(extent)) * offsets


def chain(q, s, nbr, x, kp, extent, W, W_off, b_off, modulated, d_out=None, mutant=None, kp_off=None):
    """The module: offset_conv -> dkp, mod -> deformed convolution, and the gradients of sum(out * d_out).  kp_off: the
    kernel points of offset_conv (the reference draws a rotation of its own for them, kernel_points.py), default kp."""
    kp, W, W_off, b_off = _f64(kp, W, W_off, b_off)
    kp_off = kp if kp_off is None else np.asarray(kp_off, np.float64)
    of = O.forward(q, s, nbr, x, kp_off, extent, W_off) + b_off
    nq = len(of)
    offsets = of[:, :45].reshape(nq, KP, 3)
    dkp = deformed_points(kp, offsets, extent, mutant)
    mod = 2.0 / (1.0 + np.exp(-of[:, 45:])) if modulated else None
    out, md = forward(q, s, nbr, x, dkp, mod, extent, W, mutant)
    res = dict(out=out, min_d2=md, deformed_KP=dkp, offset_features=of, mod=mod)
    if d_out is None:
        return res
    d_out, = _f64(d_out)
    dwf = d_out @ W.reshape(-1, W.shape[-1]).T
    dd, dm = d_geom(q, s, nbr, x, dkp, mod, extent, dwf, mutant)
    d_of = np.zeros_like(of)
    d_of[:, :45] = float(extent) * dd.reshape(nq, 45)
    if modulated:
        d_of[:, 45:] = dm * mod * (1.0 - mod / 2.0)
    res.update(d_x=d_x(q, s, nbr, x, dkp, mod, extent, dwf, mutant) + O.d_x(q, s, nbr, x, kp_off, extent, W_off, d_of),
               d_W=d_W(q, s, nbr, x, dkp, mod, extent, d_out, mutant), d_W_off=O.d_W(q, s, nbr, x, kp_off, extent, d_of),
               d_b_off=d_of.sum(0), d_dkp=dd, d_mod=dm)
    return res


# ----------------------------------------------------------------------------------------------------------- bounds
def margins(q, s, nbr, dkp, extent):
    """-> (min over real triples of |d / extent - 1|, min over in-ball triples of d / extent)"""
    g = geometry(q, s, nbr, dkp, extent)
    real = np.broadcast_to(g["real"][:, :, None], g["d"].shape)
    r = g["d"] / float(extent)
    edge = np.abs(r - 1.0)[real].min() if real.any() else np.inf
    ball = real & (r < 1.0)
    return float(edge), float(r[ball].min()) if ball.any() else np.inf


def _edge(g, dkp, extent):
    dkp, = _f64(dkp)
    inside = (g["real"][:, :, None] & (g["d"] < float(extent) * (1.0 + M_EDGE))).transpose(0, 2, 1)      # [nq, 15, H]
    dist = np.linalg.norm(g["D"], axis=-1)
    geo = (dist[:, None, :] + np.linalg.norm(dkp, axis=-1)[:, :, None]) / float(extent) * inside
    return inside, geo


def bound_weighted(q, s, nbr, x, dkp, mod, extent):
    x, = _f64(x)
    g = geometry(q, s, nbr, dkp, extent)
    inside, geo = _edge(g, dkp, extent)
    num, _ = count(g, x)
    ax = np.abs(x[g["idx"]]) * g["real"][:, :, None]
    a = (inside.sum(2) + 3.0) / 2.0 + 1.0
    rel = a[:, :, None] * np.einsum("qkh,qhc->qkc", g["w"], ax)
    edge = B_W * np.einsum("qkh,qhc->qkc", geo, ax)
    b = EPS32 * SECOND_ORDER * np.abs(_mod(mod, len(num)))[:, :, None] * (rel + edge) / num[:, None, None]
    return b.reshape(len(b), -1)


def bound_min_d2(q, s, nbr, dkp, extent):
    g = geometry(q, s, nbr, dkp, extent)
    e, D = np.abs(g["diff"]), np.abs(g["D"])[:, :, None, :]
    b = U * SECOND_ORDER * (2.0 * (e * (e + D)).sum(-1) + 3.0 * g["d2"])           # [nq, H, 15]
    hi = (g["d2"] + b).min(1, keepdims=True)
    cand = g["d2"] - b <= hi
    return np.where(cand, b, 0.0).max(1)


def bound_contrib(q, s, nbr, x, dkp, mod, extent, dwf):
    dwf, = _f64(dwf)
    nq, H = np.asarray(nbr).shape
    g = geometry(q, s, nbr, dkp, extent)
    inside, geo = _edge(g, dkp, extent)
    num, _ = count(g, x)
    ag = np.abs(dwf.reshape(nq, KP, -1)) * np.abs(_mod(mod, nq))[:, :, None]
    a = (inside.sum(1) + 4.0) / 2.0                                                # [nq, H]
    rel = a[:, :, None] * np.einsum("qkh,qkc->qhc", g["w"], ag)
    edge = B_W * np.einsum("qkh,qkc->qhc", geo, ag)
    return (EPS32 * SECOND_ORDER * (rel + edge) / num[:, None, None]).reshape(nq * H, -1)


def bound_dx(q, s, nbr, x, dkp, mod, extent, dwf):
    ns = len(np.asarray(s))
    rows = np.abs(contrib(q, s, nbr, x, dkp, mod, extent, dwf))
    bc = bound_contrib(q, s, nbr, x, dkp, mod, extent, dwf)
    flat = np.asarray(nbr, np.int64).reshape(-1)
    n_rows = np.bincount(flat[(flat >= 0) & (flat < ns)], minlength=ns).astype(np.float64)
    summed = O.scatter_rows(rows + bc, nbr, ns)
    return O.scatter_rows(bc, nbr, ns) + 0.5 * EPS32 * np.maximum(n_rows - 1.0, 0.0)[:, None] * summed


def bound_d_geom(q, s, nbr, x, dkp, mod, extent, dwf):
    """-> bound of d_dkp [nq, 15, 3], bound of d_mod [nq, 15]"""
    x, = _f64(x)
    cin = x.shape[1]
    g = geometry(q, s, nbr, dkp, extent)
    inside, geo = _edge(g, dkp, extent)
    num, _ = count(g, x)
    P, Pabs = _products(g, x, dwf)
    w = g["w"].transpose(0, 2, 1)                                                   # [nq, H, 15]
    n = inside.sum(2)                                                              # [nq, 15]
    ew = EPS32 * (B_W * geo.transpose(0, 2, 1) + w / 2.0)
    bm = ((ew * np.abs(P) + w * cin * U * Pabs).sum(1) + (n + 3.0) * U * (w * np.abs(P)).sum(1)) / num[:, None] * SECOND_ORDER
    t, live = _ddkp_terms(g, P, extent)
    d = np.where(live, g["d"], 1.0)
    e, D = np.abs(g["diff"]), np.abs(g["D"])[:, :, None, :]
    en, Dn = g["d"], np.linalg.norm(g["D"], axis=-1)[:, :, None]
    de = (d * float(extent))[..., None]
    bt = U * ((e + D) * np.abs(P)[..., None] / de
              + e / de * (((en + Dn) / d + 6.5) * np.abs(P) + cin * Pabs)[..., None]) * live[..., None]
    nl = live.sum(1)                                                               # [nq, 15]
    bd = (bt.sum(1) + ((nl + 3.0) * U)[..., None] * np.abs(t).sum(1)) * (np.abs(_mod(mod, len(num))) / num[:, None])[..., None] \
        * SECOND_ORDER
    return bd, bm


compare_rows = O.compare_rows
