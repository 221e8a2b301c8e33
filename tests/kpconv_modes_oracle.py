"""Float64 NumPy statement of KPConv's influence functions and aggregation modes (apr_kpconv_*_mode; the reference is
Predator_APR/models/blocks.py:61-68, 284-372), for rigid and deformed layers, with per-element error bounds for a float32
evaluation.  numpy only.  Geometry, products, scatter and compare_rows come from tests/kpconv_oracle.py and
tests/kpconv_deform_oracle.py.

Contract
--------
One statement serves both kinds of layer: KPq [nq, 15, 3] are the query's kernel points -- the rigid kernel_points repeated
(`rigid(kp, nq)`) or the deformed ones --, `deformable` says which rules apply.  mode = (influence, closest).
* d2[q, h, k] = |s[nbr[q, h]] - q - KPq[q, k]|^2; a padding slot (nbr outside 0 .. ns - 1) is the point (1e6, 1e6, 1e6) with
  a zero feature row.
* influence 0 constant: w = 1;  1 linear: w = max(0, 1 - sqrt(d2) / extent);  2 gaussian: w = exp(-d2 / (2 sigma^2 + 1e-9)),
  sigma = 0.3 extent, not clipped.
* closest: w[q, k, h] is kept for k = argmin_k d2[q, h, k] alone (the lowest k on an exact tie); the mask is a constant.
* who takes part: rigid -- every real neighbour; deformable -- the real neighbours with d2 < extent^2 for some k (in range).
  For the linear influence the filter changes nothing.  num: rigid max(1, #{real, feature sum > 0}); deformable max(1,
  #{in range, feature sum > 0}).  min_d2 as in the deform oracle.
* wf[q, k cin + c] = mod[q, k] / num[q] * sum_h w x[nbr];  out = wf @ W2;  contrib[(q, h), c] = sum_k mod w dwf[q, k, c] / num;
  P[q, h, k] = <x[nbr], dwf[q, k]>;  d_mod = sum_h w P / num;
  d_dkp: linear as the deform oracle (0 < d < extent; masked by the one-hot);  gaussian mod / num * sum_h w 2 diff / (2
  sigma^2 + 1e-9) P (w carries the filter and the mask);  constant exactly 0.

Error bounds (u = 2^-24, eps32 = 2 u; counted as sections 22 and 32 of DESIGN count them; section 34)
-----------------------------------------------------------------------------------------------
The cases keep the decisions exact: |d / extent - 1| >= 1e-3 on deformed layers (in range, count), and for closest the two
smallest d2 of every real (q, h) at least 1e-3 extent^2 apart (the float32 d2 is off by parts in 10^7) but for one planted
exact tie in dyadic coordinates.
Influence, absolute error e_w of a term that exists:
  constant  0.
  linear    eps32 (B_W geo + w / 2)                                             (section 22)
  gaussian  the argument a = d2 / den, den = fl(2 sigma^2 + 1e-9).  d2' is off by b_d2 = u (2 sum_i |e_i| (|e_i| + |D_i|) +
            3 d2) (section 32, min_d2); den by 3 u relative (float(extent) entering sigma: 2 u, the rounding of den: u), the
            division rounds once: |a' - a| <= da = b_d2 / den + 4 u a.  exp amplifies the RELATIVE error of a by a itself:
            |exp(-a') - exp(-a)| <= w expm1(da).  expf adds E_EXP eps32 w (E_EXP: its own error in units of eps32 |w|, an
            upper bound of the ulp; measured).  Where w or its float32 value lies under the smallest normal number
            (2^-126: the far support at (9, 9, 9)) the result may be denormal or flushed: an ABSOLUTE term 2^-125.
            e_w = (w expm1(da) + E_EXP eps32 w) (1 + 2^-10) + 2^-125.
wf:       eps32 |mod| (A sum_h w |x| + sum_h e_w' |x|) / num (1 + 2^-10), A = (n + 3) / 2 (+ 1 on a deformed layer: the product
          with mod), n = the terms that exist, e_w' = e_w without the w / 2 that A already holds (linear) or e_w / eps32.
contrib:  the same with the m kernel points of a (q, h) that exist: A = (m + 3) / 2 (+ 1 / 2 deformed).
d_x:      the rows' bounds plus (n_r - 1) u sum (|row| + bound)                    (section 22).
d_mod:    (sum_h (e_w |P| + w cin u Pabs) + (n + 3) u sum_h w |P|) / num (1 + 2^-10)     (section 32).
d_dkp:    linear: section 32's per-term bound over the terms the mask keeps.  constant: 0 (the value must be exactly 0).
          gaussian, per term t_i = w c e_i P, c = 2 / den (4 u: den's 3 u and the division), two products (2 u), e_i off by
          u (|e_i| + |D_i|), P by cin u Pabs:
            b_t,i = c (e_w |e_i| |P| + w u (|e_i| + |D_i|) |P| + w |e_i| cin u Pabs + 6 u w |e_i| |P|),
          summed over n terms and scaled by fl(mod fl(1 / num)): |mod| / num (sum_h b_t + (n + 3) u sum_h |t|) (1 + 2^-10).
"""
import numpy as np

import kpconv_deform_oracle as DO
import kpconv_oracle as O

EPS32, B_W, M_EDGE, SECOND_ORDER, KP, U = O.EPS32, O.B_W, O.M_EDGE, O.SECOND_ORDER, O.KP, O.EPS32 / 2.0
CONSTANT, LINEAR, GAUSSIAN = 0, 1, 2
MODES = [(CONSTANT, 0), (CONSTANT, 1), (LINEAR, 0), (LINEAR, 1), (GAUSSIAN, 0), (GAUSSIAN, 1)]
NEW_MODES = [m for m in MODES if m != (LINEAR, 0)]
NAMES = {0: "constant", 1: "linear", 2: "gaussian"}
# expf's own error in units of eps32 |w|: twice the worst figure measured on the MI355X over 2^20 arguments in [0, 110]
# (0.6757 at argument 40.16; scripts/kpconv_modes_expf.py).  No document shipped with ROCm states one.
E_EXP = 2 * 0.6757
ABS_EXP = 2.0 ** -125
MUTANTS = ("gauss_sigma_extent", "gauss_clipped", "const_out_of_range", "closest_last_tie", "closest_grad_unmasked",
           "ddkp_gauss_half", "const_ddkp_linear")
_f64 = DO._f64


def mode_name(mode):
    return f"{NAMES[mode[0]]}-{'closest' if mode[1] else 'sum'}"


def rigid(kp, nq):
    """the rigid kernel points as every query's own"""
    return np.broadcast_to(np.asarray(kp, np.float64)[None], (nq, KP, 3)).copy()


def gauss_den(extent, mutant=None):
    sigma = float(extent) if mutant == "gauss_sigma_extent" else 0.3 * float(extent)
    return 2.0 * sigma ** 2 + 1e-9


def geometry(q, s, nbr, KPq, extent, mode, deformable, mutant=None):
    """the deform oracle's geometry plus: take [nq, H] (who takes part), cl [nq, H] (closest kernel point), keep [nq, H, 15]
    (take and the one-hot), w [nq, 15, H] (the mode's influences, 0 where nothing is kept)"""
    inf, closest = mode
    g = DO.geometry(q, s, nbr, KPq, extent)
    take = g["in_range"] if (deformable and mutant != "const_out_of_range") else g["real"]
    d2, d = g["d2"], g["d"]
    if mutant == "closest_last_tie":
        cl = KP - 1 - np.argmin(d2[:, :, ::-1], axis=-1)
    else:
        cl = np.argmin(d2, axis=-1)
    keep = np.broadcast_to(take[:, :, None], d2.shape).copy()
    if closest:
        keep &= np.arange(KP)[None, None, :] == cl[:, :, None]
    if inf == CONSTANT:
        w = np.ones_like(d2)
    elif inf == LINEAR:
        w = np.maximum(0.0, 1.0 - d / float(extent))
    else:
        w = np.exp(-d2 / gauss_den(extent, mutant))
        if mutant == "gauss_clipped" and not deformable:
            w = w * (d < float(extent))
    g.update(take=take, cl=cl, keep=keep, w=(w * keep).transpose(0, 2, 1), mode=mode, deformable=deformable)
    return g


def count(g, nbr, x):
    if g["deformable"]:
        return DO.count(g, x)[0]
    return O.neighbour_count(nbr, x)[0]


def _mod(mod, nq):
    return np.ones((nq, KP)) if mod is None else np.asarray(mod, np.float64)


def weighted(q, s, nbr, x, KPq, mod, extent, mode, deformable, mutant=None):
    """-> wf [nq, 15 cin], num, geometry"""
    x, = _f64(x)
    g = geometry(q, s, nbr, KPq, extent, mode, deformable, mutant)
    num = count(g, nbr, x)
    xg = x[g["idx"]] * g["real"][:, :, None]
    S = np.einsum("qkh,qhc->qkc", g["w"], xg) / num[:, None, None]
    wf = _mod(mod, len(S))[:, :, None] * S
    return wf.reshape(len(wf), -1), num, g


def min_d2(q, s, nbr, KPq, extent):
    return DO.min_d2(q, s, nbr, KPq, extent)


def forward(q, s, nbr, x, KPq, mod, extent, W, mode, deformable, mutant=None):
    W, = _f64(W)
    return weighted(q, s, nbr, x, KPq, mod, extent, mode, deformable, mutant)[0] @ W.reshape(-1, W.shape[-1])


def contrib(q, s, nbr, x, KPq, mod, extent, dwf, mode, deformable, mutant=None):
    dwf, = _f64(dwf)
    nq, H = np.asarray(nbr).shape
    g = geometry(q, s, nbr, KPq, extent, mode, deformable, mutant)
    num = count(g, nbr, x)
    gg = dwf.reshape(nq, KP, -1) * _mod(mod, nq)[:, :, None] / num[:, None, None]
    return np.einsum("qkh,qkc->qhc", g["w"], gg).reshape(nq * H, -1)


def d_x(q, s, nbr, x, KPq, mod, extent, dwf, mode, deformable, mutant=None):
    return O.scatter_rows(contrib(q, s, nbr, x, KPq, mod, extent, dwf, mode, deformable, mutant), nbr, len(np.asarray(s)))


def _ddkp_terms(g, P, extent, mutant=None):
    """t [nq, H, 15, 3]: the terms of d_dkp before mod / num, and the mask of the terms that exist"""
    inf, closest = g["mode"]
    keep = g["keep"]
    if inf == CONSTANT and mutant != "const_ddkp_linear":
        return np.zeros(g["diff"].shape), np.zeros(keep.shape, bool)
    if inf == GAUSSIAN:
        c = (1.0 if mutant == "ddkp_gauss_half" else 2.0) / gauss_den(extent)
        w = g["w"].transpose(0, 2, 1)
        return g["diff"] * (w * c * P)[..., None], keep
    t, live = DO._ddkp_terms(g, P, extent)
    mask = np.ones_like(keep) if (mutant == "closest_grad_unmasked" or not closest) else keep
    if inf == CONSTANT:      # the mutant: the linear formula on what a constant layer keeps
        mask = keep
    return t * mask[..., None], live & mask


def d_geom(q, s, nbr, x, KPq, mod, extent, dwf, mode, mutant=None):
    """deformed layers -> d_dkp [nq, 15, 3], d_mod [nq, 15]"""
    g = geometry(q, s, nbr, KPq, extent, mode, True, mutant)
    num = count(g, nbr, x)
    P, _ = DO._products(g, x, dwf)
    dm = np.einsum("qkh,qhk->qk", g["w"], P) / num[:, None]
    t, _ = _ddkp_terms(g, P, extent, mutant)
    dd = t.sum(1) * (_mod(mod, len(num)) / num[:, None])[:, :, None]
    return dd, dm


def d_W(q, s, nbr, x, KPq, mod, extent, d_out, mode, deformable, mutant=None):
    d_out, = _f64(d_out)
    wf = weighted(q, s, nbr, x, KPq, mod, extent, mode, deformable, mutant)[0]
    return (wf.T @ d_out).reshape(KP, -1, d_out.shape[1])


def chain(q, s, nbr, x, kp, extent, W, mode, d_out=None, W_off=None, b_off=None, modulated=False, kp_off=None, mutant=None):
    """The module.  W_off None: a rigid layer.  Otherwise offset_conv (a rigid layer of the same mode) -> dkp, mod -> the
    deformed convolution; with d_out the gradients of sum(out * d_out).  kp_off: offset_conv's own kernel points."""
    kp, W = _f64(kp, W)
    nq = len(np.asarray(q))
    W2 = W.reshape(-1, W.shape[-1])
    if W_off is None:
        K = rigid(kp, nq)
        res = dict(out=forward(q, s, nbr, x, K, None, extent, W, mode, False, mutant))
        if d_out is not None:
            d_out, = _f64(d_out)
            res.update(d_x=d_x(q, s, nbr, x, K, None, extent, d_out @ W2.T, mode, False, mutant),
                       d_W=d_W(q, s, nbr, x, K, None, extent, d_out, mode, False, mutant))
        return res
    W_off, b_off = _f64(W_off, b_off)
    K_off = rigid(kp if kp_off is None else kp_off, nq)
    of = forward(q, s, nbr, x, K_off, None, extent, W_off, mode, False, mutant) + b_off
    dkp = DO.deformed_points(kp, of[:, :45].reshape(nq, KP, 3), extent)
    mod = 2.0 / (1.0 + np.exp(-of[:, 45:])) if modulated else None
    res = dict(out=forward(q, s, nbr, x, dkp, mod, extent, W, mode, True, mutant), min_d2=min_d2(q, s, nbr, dkp, extent),
               deformed_KP=dkp, offset_features=of, mod=mod)
    if d_out is None:
        return res
    d_out, = _f64(d_out)
    dwf = d_out @ W2.T
    dd, dm = d_geom(q, s, nbr, x, dkp, mod, extent, dwf, mode, mutant)
    d_of = np.zeros_like(of)
    d_of[:, :45] = float(extent) * dd.reshape(nq, 45)
    if modulated:
        d_of[:, 45:] = dm * mod * (1.0 - mod / 2.0)
    W_off2 = W_off.reshape(-1, W_off.shape[-1])
    res.update(d_x=d_x(q, s, nbr, x, dkp, mod, extent, dwf, mode, True, mutant)
               + d_x(q, s, nbr, x, K_off, None, extent, d_of @ W_off2.T, mode, False, mutant),
               d_W=d_W(q, s, nbr, x, dkp, mod, extent, d_out, mode, True, mutant),
               d_W_off=d_W(q, s, nbr, x, K_off, None, extent, d_of, mode, False, mutant), d_b_off=d_of.sum(0), d_dkp=dd, d_mod=dm)
    return res


# ----------------------------------------------------------------------------------------------------------- margins
def closest_margin(q, s, nbr, KPq, extent, exempt=()):
    """min over the real (q, h) outside `exempt` of (second smallest d2 - smallest d2) / extent^2"""
    g = DO.geometry(q, s, nbr, KPq, extent)
    two = np.sort(g["d2"], axis=-1)[:, :, :2]
    gap = (two[:, :, 1] - two[:, :, 0]) / float(extent) ** 2
    ok = g["real"].copy()
    for row, h in exempt:
        ok[row, h] = False
    return float(gap[ok].min()) if ok.any() else np.inf


# ------------------------------------------------------------------------------------------------------------ bounds
def _influence_error(g, KPq, extent):
    """-> (w [nq, H, 15], e_w: the absolute error of a float32 influence where the term exists, e_sum: e_w without the
    eps32 w / 2 that the sums' factor A already holds (linear), lives: the terms that may be non-zero in float32)"""
    inf, _ = g["mode"]
    keep = g["keep"]
    w = g["w"].transpose(0, 2, 1)
    if inf == CONSTANT:
        return w, np.zeros_like(w), np.zeros_like(w), keep
    if inf == LINEAR:
        KPq, = _f64(KPq)
        lives = keep & g["real"][:, :, None] & (g["d"] < float(extent) * (1.0 + M_EDGE))
        dist = np.linalg.norm(g["D"], axis=-1)
        geo = (dist[:, :, None] + np.linalg.norm(KPq, axis=-1)[:, None, :]) / float(extent)
        return w, EPS32 * (B_W * geo + w / 2.0) * lives, EPS32 * B_W * geo * lives, lives
    den = gauss_den(extent)
    e, D = np.abs(g["diff"]), np.abs(g["D"])[:, :, None, :]
    b_d2 = U * (2.0 * (e * (e + D)).sum(-1) + 3.0 * g["d2"])
    da = np.where(keep, b_d2 / den + 4.0 * U * g["d2"] / den, 0.0)      # (a padding slot's d2 ~ 3e12 is nobody's argument)
    e_w =((w * np.expm1(da) + E_EXP * EPS32 * w) * SECOND_ORDER + ABS_EXP) * keep
    return w, e_w, e_w, keep


def bound_weighted(q, s, nbr, x, KPq, mod, extent, mode, deformable):
    x, = _f64(x)
    g = geometry(q, s, nbr, KPq, extent, mode, deformable)
    w, _, e_w, lives = _influence_error(g, KPq, extent)
    num = count(g, nbr, x)
    ax = np.abs(x[g["idx"]]) * g["real"][:, :, None]
    a = (lives.sum(1) + 3.0) / 2.0 + (1.0 if deformable else 0.0)                  # [nq, 15]
    rel = EPS32 * a[:, :, None] * np.einsum("qhk,qhc->qkc", w, ax)
    edge = np.einsum("qhk,qhc->qkc", e_w, ax)
    b = SECOND_ORDER * np.abs(_mod(mod, len(num)))[:, :, None] * (rel + edge) / num[:, None, None]
    return b.reshape(len(b), -1)


def bound_contrib(q, s, nbr, x, KPq, mod, extent, dwf, mode, deformable):
    dwf, = _f64(dwf)
    nq, H = np.asarray(nbr).shape
    g = geometry(q, s, nbr, KPq, extent, mode, deformable)
    w, _, e_w, lives = _influence_error(g, KPq, extent)
    num = count(g, nbr, x)
    ag = np.abs(dwf.reshape(nq, KP, -1)) * np.abs(_mod(mod, nq))[:, :, None]
    a = (lives.sum(2) + (4.0 if deformable else 3.0)) / 2.0                         # [nq, H]
    rel = EPS32 * a[:, :, None] * np.einsum("qhk,qkc->qhc", w, ag)
    edge = np.einsum("qhk,qkc->qhc", e_w, ag)
    return (SECOND_ORDER * (rel + edge) / num[:, None, None]).reshape(nq * H, -1)


def bound_dx(q, s, nbr, x, KPq, mod, extent, dwf, mode, deformable):
    ns = len(np.asarray(s))
    rows = np.abs(contrib(q, s, nbr, x, KPq, mod, extent, dwf, mode, deformable))
    bc = bound_contrib(q, s, nbr, x, KPq, mod, extent, dwf, mode, deformable)
    flat = np.asarray(nbr, np.int64).reshape(-1)
    n_rows = np.bincount(flat[(flat >= 0) & (flat < ns)], minlength=ns).astype(np.float64)
    summed = O.scatter_rows(rows + bc, nbr, ns)
    return O.scatter_rows(bc, nbr, ns) + 0.5 * EPS32 * np.maximum(n_rows - 1.0, 0.0)[:, None] * summed


def bound_d_geom(q, s, nbr, x, KPq, mod, extent, dwf, mode):
    """-> bound of d_dkp [nq, 15, 3], bound of d_mod [nq, 15]"""
    x, = _f64(x)
    cin = x.shape[1]
    inf, _ = mode
    g = geometry(q, s, nbr, KPq, extent, mode, True)
    w, e_w, _, lives = _influence_error(g, KPq, extent)
    num = count(g, nbr, x)
    P, Pabs = DO._products(g, x, dwf)
    n = lives.sum(1)                                                               # [nq, 15]
    bm = ((e_w * np.abs(P) + w * cin * U * Pabs).sum(1) + (n + 3.0) * U * (w * np.abs(P)).sum(1)) / num[:, None] * SECOND_ORDER
    scale = (np.abs(_mod(mod, len(num))) / num[:, None])[..., None] * SECOND_ORDER
    t, live = _ddkp_terms(g, P, extent)
    e, D = np.abs(g["diff"]), np.abs(g["D"])[:, :, None, :]
    if inf == CONSTANT:
        return np.zeros(t.sum(1).shape), bm
    if inf == GAUSSIAN:
        c = 2.0 / gauss_den(extent)
        aP = np.abs(P)[..., None]
        bt = c * (e_w[..., None] * e * aP + w[..., None] * U * (e + D) * aP + (w * cin * U * Pabs)[..., None] * e
                  + 6.0 * U * w[..., None] * e * aP) * live[..., None]
    else:
        d = np.where(live, g["d"], 1.0)
        en, Dn = g["d"], np.linalg.norm(g["D"], axis=-1)[:, :, None]
        de = (d * float(extent))[..., None]
        bt = U * ((e + D) * np.abs(P)[..., None] / de
                  + e / de * (((en + Dn) / d + 6.5) * np.abs(P) + cin * Pabs)[..., None]) * live[..., None]
    nl = live.sum(1)
    bd = (bt.sum(1) + ((nl + 3.0) * U)[..., None] * np.abs(t).sum(1)) * scale
    return bd, bm


compare_rows = O.compare_rows
