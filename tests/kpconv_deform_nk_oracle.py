"""Float64 NumPy statement of the deformable / modulated KPConv with ANY kernel-point count (apr_kpconv_deform_weighted_nk,
apr_kpconv_deform_dfeat_contrib_nk, apr_kpconv_deform_dgeom_nk; apr_amd/csrc/kpconv_deform_nk.hip), every influence and both
aggregations, with per-element error bounds for a float32 evaluation, a plain float32 evaluation in the kernels' order and
its one-rule mutants.  numpy only.

The contract is tests/kpconv_modes_oracle.py's for a deformed layer with K = dkp.shape[1] in place of its 15 and 45:
dkp [nq, K, 3] are the query's own kernel points, mod [nq, K] or None, mode = (influence, closest).
* d2[q, h, k] = |s[nbr[q, h]] - q - dkp[q, k]|^2; a padding slot (nbr outside 0 .. ns - 1) is the point (1e6, 1e6, 1e6) with a
  zero feature row.  min_d2[q, k] = min over ALL H slots of d2.
* in range: real and d2 < extent^2 for some k.  Only the neighbours in range take part (for the linear influence the filter
  changes nothing) and num = max(1, #{in range, feature sum > 0}).
* influence 0 constant w = 1; 1 linear w = max(0, 1 - sqrt(d2) / extent); 2 gaussian w = exp(-d2 / (2 (0.3 extent)^2 + 1e-9)).
  closest keeps w for k = argmin_k d2 alone, the lowest k on an exact tie; the mask is a constant of the graph.
* wf[q, k cin + c] = mod[q, k] / num[q] sum_h w x[nbr];  contrib[(q, h), c] = sum_k mod w dwf[q, k, c] / num;
  P[q, h, k] = <x[nbr], dwf[q, k]>;  d_mod = sum_h w P / num;  d_dkp: linear mod / num sum_{0 < d < extent} diff / (d extent) P
  (masked by the one-hot; d = 0 contributes 0), gaussian mod / num sum_h w 2 diff / (2 sigma^2 + 1e-9) P, constant exactly 0.
* the module `chain`: offset_conv (a rigid layer with K kernel points and (p_dim + 1 when modulated) K outputs:
  tests/kpconv_nk_oracle.py) -> dkp = kp + extent offsets, mod = 2 sigmoid -> the deformed convolution, and the gradients of
  sum(out * d_out).

Error bounds: the derivations of tests/kpconv_modes_oracle.py and tests/kpconv_deform_oracle.py (their docstrings; DESIGN
sections 22, 32, 34) count roundings per term and per sum -- A = (n + 3) / 2 (+ 1 for the product with mod) with n the terms
that exist, the influence's own error per term, (n_r - 1) u for the rows' sum, cin u Pabs for a product P -- and no step of
them depends on K.  They are restated here with K from dkp.shape[1]; tests/test_kpconv_deform_nk_oracle_cpu.py holds every
statement and every bound to kpconv_modes_oracle at K = 15 in all six modes.
"""
import numpy as np

import kpconv_modes_oracle as MO
import kpconv_nk_oracle as NO
import kpconv_oracle as O

EPS32, B_W, M_EDGE, SECOND_ORDER, U = O.EPS32, O.B_W, O.M_EDGE, O.SECOND_ORDER, O.EPS32 / 2.0
E_EXP, ABS_EXP = MO.E_EXP, MO.ABS_EXP
CONSTANT, LINEAR, GAUSSIAN = 0, 1, 2
MODES = MO.MODES
DEFAULT = (LINEAR, 0)
SHADOW = 1e6
mode_name = MO.mode_name
gauss_den = MO.gauss_den
compare_rows = O.compare_rows
F32 = np.float32
MUTANTS = ("inrange_tile0_only", "min_rows_ge16_dropped", "mod_stride_15", "tiles_swapped", "tie_high", "count_rigid")


def _f64(*arrays):
    return [np.asarray(a, np.float64) for a in arrays]


def geometry(q, s, nbr, dkp, extent, mode=DEFAULT):
    """-> dict: real, idx, in_range, cl [nq, H]; D [nq, H, 3]; diff [nq, H, K, 3]; d2, d [nq, H, K]; keep [nq, H, K] (in range
    and, with closest, the one-hot); w [nq, K, H] (the mode's influences, 0 where nothing is kept)"""
    inf, closest = mode
    q, s, dkp = _f64(q, s, dkp)
    K = dkp.shape[1]
    real = O.real_mask(nbr, len(s))
    idx = np.where(real, np.asarray(nbr, np.int64), 0)
    D = np.where(real[:, :, None], s[idx], SHADOW) - q[:, None, :]
    diff = D[:, :, None, :] - dkp[:, None, :, :]
    d2 = (diff ** 2).sum(-1)
    d = np.sqrt(d2)
    in_range = real & (d2 < float(extent) ** 2).any(-1)
    cl = np.argmin(d2, axis=-1)
    keep = np.broadcast_to(in_range[:, :, None], d2.shape).copy()
    if closest:
        keep &= np.arange(K)[None, None, :] == cl[:, :, None]
    if inf == CONSTANT:
        w = np.ones_like(d2)
    elif inf == LINEAR:
        w = np.maximum(0.0, 1.0 - d / float(extent))
    else:
        w = np.exp(-d2 / gauss_den(extent))
    return dict(real=real, idx=idx, D=D, diff=diff, d2=d2, d=d, in_range=in_range, cl=cl, keep=keep,
                w=(w * keep).transpose(0, 2, 1), mode=mode, K=K)


def count(g, x):
    """-> num [nq] (floored at 1), raw count"""
    x, = _f64(x)
    raw = (g["in_range"] & (x.sum(1)[g["idx"]] > 0)).sum(1)
    return np.maximum(raw, 1).astype(np.float64), raw


def _mod(mod, nq, K):
    return np.ones((nq, K)) if mod is None else np.asarray(mod, np.float64)


def weighted(q, s, nbr, x, dkp, mod, extent, mode=DEFAULT):
    """-> wf [nq, K cin], num, geometry"""
    x, = _f64(x)
    g = geometry(q, s, nbr, dkp, extent, mode)
    num, _ = count(g, x)
    xg = x[g["idx"]] * g["real"][:, :, None]
    S = np.einsum("qkh,qhc->qkc", g["w"], xg) / num[:, None, None]
    wf = _mod(mod, len(S), g["K"])[:, :, None] * S
    return wf.reshape(len(wf), -1), num, g


def min_d2(q, s, nbr, dkp, extent):
    return geometry(q, s, nbr, dkp, extent)["d2"].min(1)


def forward(q, s, nbr, x, dkp, mod, extent, W, mode=DEFAULT):
    W, = _f64(W)
    return weighted(q, s, nbr, x, dkp, mod, extent, mode)[0] @ W.reshape(-1, W.shape[-1])


def contrib(q, s, nbr, x, dkp, mod, extent, dwf, mode=DEFAULT):
    """dwf [nq, K cin] -> [nq * H, cin]; the rows of padding neighbours are 0"""
    dwf, = _f64(dwf)
    nq, H = np.asarray(nbr).shape
    g = geometry(q, s, nbr, dkp, extent, mode)
    num, _ = count(g, x)
    gg = dwf.reshape(nq, g["K"], -1) * _mod(mod, nq, g["K"])[:, :, None] / num[:, None, None]
    return np.einsum("qkh,qkc->qhc", g["w"], gg).reshape(nq * H, -1)


def d_x(q, s, nbr, x, dkp, mod, extent, dwf, mode=DEFAULT):
    return O.scatter_rows(contrib(q, s, nbr, x, dkp, mod, extent, dwf, mode), nbr, len(np.asarray(s)))


def _products(g, x, dwf):
    """P [nq, H, K], Pabs [nq, H, K]"""
    x, dwf = _f64(x, dwf)
    xg = x[g["idx"]] * g["real"][:, :, None]
    dk = dwf.reshape(len(dwf), g["K"], -1)
    return np.einsum("qhc,qkc->qhk", xg, dk), np.einsum("qhc,qkc->qhk", np.abs(xg), np.abs(dk))


def _ddkp_terms(g, P, extent):
    """t [nq, H, K, 3]: the terms of d_dkp before mod / num, and the mask of the terms that exist"""
    inf, closest = g["mode"]
    keep = g["keep"]
    if inf == CONSTANT:
        return np.zeros(g["diff"].shape), np.zeros(keep.shape, bool)
    if inf == GAUSSIAN:
        w = g["w"].transpose(0, 2, 1)
        return g["diff"] * (w * (2.0 / gauss_den(extent)) * P)[..., None], keep
    d = g["d"]
    live = g["real"][:, :, None] & (d > 0) & (d < float(extent))
    if closest:
        live = live & keep
    safe = np.where(live, d, 1.0)
    return g["diff"] * (P / (safe * float(extent)) * live)[..., None], live


def d_geom(q, s, nbr, x, dkp, mod, extent, dwf, mode=DEFAULT):
    """-> d_dkp [nq, K, 3], d_mod [nq, K]"""
    g = geometry(q, s, nbr, dkp, extent, mode)
    num, _ = count(g, x)
    P, _ = _products(g, x, dwf)
    dm = np.einsum("qkh,qhk->qk", g["w"], P) / num[:, None]
    t, _ = _ddkp_terms(g, P, extent)
    dd = t.sum(1) * (_mod(mod, len(num), g["K"]) / num[:, None])[:, :, None]
    return dd, dm


def d_W(q, s, nbr, x, dkp, mod, extent, d_out, mode=DEFAULT):
    d_out, = _f64(d_out)
    wf = weighted(q, s, nbr, x, dkp, mod, extent, mode)[0]
    return (wf.T @ d_out).reshape(np.asarray(dkp).shape[1], -1, d_out.shape[1])


def chain(q, s, nbr, x, kp, extent, W, W_off, b_off, modulated, mode=DEFAULT, d_out=None, kp_off=None):
    """The module: offset_conv (a rigid layer of the same mode; kp_off: its own kernel points, default kp) -> dkp, mod -> the
    deformed convolution; with d_out the gradients of sum(out * d_out)."""
    kp, W, W_off, b_off = _f64(kp, W, W_off, b_off)
    kp_off = kp if kp_off is None else np.asarray(kp_off, np.float64)
    K, nq = len(kp), len(np.asarray(q))
    n3 = 3 * K
    W2 = W.reshape(-1, W.shape[-1])
    of = NO.forward(q, s, nbr, x, kp_off, extent, W_off, mode) + b_off
    dkp = kp[None] + float(extent) * of[:, :n3].reshape(nq, K, 3)
    mod = 2.0 / (1.0 + np.exp(-of[:, n3:])) if modulated else None
    res = dict(out=forward(q, s, nbr, x, dkp, mod, extent, W, mode), min_d2=min_d2(q, s, nbr, dkp, extent), deformed_KP=dkp,
               offset_features=of, mod=mod)
    if d_out is None:
        return res
    d_out, = _f64(d_out)
    dwf = d_out @ W2.T
    dd, dm = d_geom(q, s, nbr, x, dkp, mod, extent, dwf, mode)
    d_of = np.zeros_like(of)
    d_of[:, :n3] = float(extent) * dd.reshape(nq, n3)
    if modulated:
        d_of[:, n3:] = dm * mod * (1.0 - mod / 2.0)
    W_off2 = W_off.reshape(-1, W_off.shape[-1])
    res.update(d_x=d_x(q, s, nbr, x, dkp, mod, extent, dwf, mode)
               + NO.d_x_from_dwf(q, s, nbr, x, kp_off, extent, d_of @ W_off2.T, mode),
               d_W=d_W(q, s, nbr, x, dkp, mod, extent, d_out, mode), d_W_off=NO.d_W(q, s, nbr, x, kp_off, extent, d_of, mode),
               d_b_off=d_of.sum(0), d_dkp=dd, d_mod=dm)
    return res


# ----------------------------------------------------------------------------------------------------------- margins
def margins(q, s, nbr, dkp, extent):
    """-> (min over real triples of |d / extent - 1|, min over in-ball triples of d / extent)"""
    g = geometry(q, s, nbr, dkp, extent)
    real = np.broadcast_to(g["real"][:, :, None], g["d"].shape)
    r = g["d"] / float(extent)
    edge = np.abs(r - 1.0)[real].min() if real.any() else np.inf
    ball = real & (r < 1.0)
    return float(edge), float(r[ball].min()) if ball.any() else np.inf


def closest_margin(q, s, nbr, dkp, extent, exempt=()):
    """min over the real (q, h) outside `exempt` of (second smallest d2 - smallest d2) / extent^2 (inf for K = 1)"""
    g = geometry(q, s, nbr, dkp, extent)
    if g["K"] < 2:
        return np.inf
    two = np.sort(g["d2"], axis=-1)[:, :, :2]
    gap = (two[:, :, 1] - two[:, :, 0]) / float(extent) ** 2
    ok = g["real"].copy()
    for row, h in exempt:
        ok[row, h] = False
    return float(gap[ok].min()) if ok.any() else np.inf


# ------------------------------------------------------------------------------------------------------------ bounds
def _influence_error(g, dkp, extent):
    """-> (w [nq, H, K], e_w: the absolute error of a float32 influence where the term exists, e_sum: e_w without the
    eps32 w / 2 that the sums' factor A already holds (linear), lives: the terms that may be non-zero in float32)"""
    inf, _ = g["mode"]
    keep = g["keep"]
    w = g["w"].transpose(0, 2, 1)
    if inf == CONSTANT:
        return w, np.zeros_like(w), np.zeros_like(w), keep
    if inf == LINEAR:
        dkp, = _f64(dkp)
        lives = keep & g["real"][:, :, None] & (g["d"] < float(extent) * (1.0 + M_EDGE))
        dist = np.linalg.norm(g["D"], axis=-1)
        geo = (dist[:, :, None] + np.linalg.norm(dkp, axis=-1)[:, None, :]) / float(extent)
        return w, EPS32 * (B_W * geo + w / 2.0) * lives, EPS32 * B_W * geo * lives, lives
    den = gauss_den(extent)
    e, D = np.abs(g["diff"]), np.abs(g["D"])[:, :, None, :]
    b_d2 = U * (2.0 * (e * (e + D)).sum(-1) + 3.0 * g["d2"])
    da = np.where(keep, b_d2 / den + 4.0 * U * g["d2"] / den, 0.0)      # (a padding slot's d2 ~ 3e12 is nobody's argument)
    e_w = ((w * np.expm1(da) + E_EXP * EPS32 * w) * SECOND_ORDER + ABS_EXP) * keep
    return w, e_w, e_w, keep


def bound_weighted(q, s, nbr, x, dkp, mod, extent, mode=DEFAULT):
    x, = _f64(x)
    g = geometry(q, s, nbr, dkp, extent, mode)
    w, _, e_w, lives = _influence_error(g, dkp, extent)
    num, _ = count(g, x)
    ax = np.abs(x[g["idx"]]) * g["real"][:, :, None]
    a = (lives.sum(1) + 3.0) / 2.0 + 1.0                                            # [nq, K]
    rel = EPS32 * a[:, :, None] * np.einsum("qhk,qhc->qkc", w, ax)
    edge = np.einsum("qhk,qhc->qkc", e_w, ax)
    b = SECOND_ORDER * np.abs(_mod(mod, len(num), g["K"]))[:, :, None] * (rel + edge) / num[:, None, None]
    return b.reshape(len(b), -1)


def bound_min_d2(q, s, nbr, dkp, extent):
    g = geometry(q, s, nbr, dkp, extent)
    e, D = np.abs(g["diff"]), np.abs(g["D"])[:, :, None, :]
    b = U * SECOND_ORDER * (2.0 * (e * (e + D)).sum(-1) + 3.0 * g["d2"])           # [nq, H, K]
    hi = (g["d2"] + b).min(1, keepdims=True)
    cand = g["d2"] - b <= hi
    return np.where(cand, b, 0.0).max(1)


def bound_contrib(q, s, nbr, x, dkp, mod, extent, dwf, mode=DEFAULT):
    dwf, = _f64(dwf)
    nq, H = np.asarray(nbr).shape
    g = geometry(q, s, nbr, dkp, extent, mode)
    w, _, e_w, lives = _influence_error(g, dkp, extent)
    num, _ = count(g, x)
    ag = np.abs(dwf.reshape(nq, g["K"], -1)) * np.abs(_mod(mod, nq, g["K"]))[:, :, None]
    a = (lives.sum(2) + 4.0) / 2.0                                                  # [nq, H]
    rel = EPS32 * a[:, :, None] * np.einsum("qhk,qkc->qhc", w, ag)
    edge = np.einsum("qhk,qkc->qhc", e_w, ag)
    return (SECOND_ORDER * (rel + edge) / num[:, None, None]).reshape(nq * H, -1)


def bound_dx(q, s, nbr, x, dkp, mod, extent, dwf, mode=DEFAULT):
    ns = len(np.asarray(s))
    rows = np.abs(contrib(q, s, nbr, x, dkp, mod, extent, dwf, mode))
    bc = bound_contrib(q, s, nbr, x, dkp, mod, extent, dwf, mode)
    flat = np.asarray(nbr, np.int64).reshape(-1)
    n_rows = np.bincount(flat[(flat >= 0) & (flat < ns)], minlength=ns).astype(np.float64)
    summed = O.scatter_rows(rows + bc, nbr, ns)
    return O.scatter_rows(bc, nbr, ns) + 0.5 * EPS32 * np.maximum(n_rows - 1.0, 0.0)[:, None] * summed


def bound_d_geom(q, s, nbr, x, dkp, mod, extent, dwf, mode=DEFAULT):
    """-> bound of d_dkp [nq, K, 3], bound of d_mod [nq, K]"""
    x, = _f64(x)
    cin = x.shape[1]
    inf, _ = mode
    g = geometry(q, s, nbr, dkp, extent, mode)
    w, e_w, _, lives = _influence_error(g, dkp, extent)
    num, _ = count(g, x)
    P, Pabs = _products(g, x, dwf)
    n = lives.sum(1)                                                               # [nq, K]
    bm = ((e_w * np.abs(P) + w * cin * U * Pabs).sum(1) + (n + 3.0) * U * (w * np.abs(P)).sum(1)) / num[:, None] * SECOND_ORDER
    scale = (np.abs(_mod(mod, len(num), g["K"])) / num[:, None])[..., None] * SECOND_ORDER
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


# ------------------------------------------------------------------------- a plain float32 evaluation and its mutants
def _swap16(K):
    perm = np.arange(K)
    for k in range(K):
        if k < 16 and k + 16 < K:
            perm[k], perm[k + 16] = k + 16, k
    return perm


def eval32(q, s, nbr, x, dkp, mod, extent, dwf, mode=DEFAULT, mutant=None):
    """The statement with every operation in float32, in the kernels' order where NumPy lets one choose (neighbours in slot
    order, kernel points ascending, the factor mod * (1 / num) applied last) -> dict(wf, min_d2, contrib, d_mod, d_dkp).
    mutant: one rule changed --
      inrange_tile0_only     a slot's in-range flag looks at kernel points 0 .. 15 only (the OR over both tiles forgotten)
      min_rows_ge16_dropped  min_d2 rows 16 .. K - 1 are never reduced: they keep the first tile's value
      mod_stride_15          mod is addressed as q * 15 + k instead of q * K + k
      tiles_swapped          kernel point k trades places with k +- 16 where both exist
      tie_high               an exact tie for the closest kernel point goes to the HIGHER index
      count_rigid            num counts every real neighbour with a positive feature sum (the rigid rule)"""
    inf, closest = mode
    q, s, dkp, x, dwf = (np.asarray(a, F32) for a in (q, s, dkp, x, dwf))
    nq, H = np.asarray(nbr).shape
    K, cin = dkp.shape[1], x.shape[1]
    ext = F32(extent)
    m = np.ones((nq, K), F32) if mod is None else np.asarray(mod, F32)
    if mutant == "mod_stride_15" and mod is not None:
        flat = np.concatenate([m.reshape(-1), np.ones(nq * 15 + K, F32)])
        m = np.stack([flat[r * 15:r * 15 + K] for r in range(nq)])
    real = O.real_mask(nbr, len(s))
    idx = np.where(real, np.asarray(nbr, np.int64), 0)
    D = (np.where(real[:, :, None], s[idx], F32(SHADOW)) - q[:, None, :]).astype(F32)
    e = (D[:, :, None, :] - dkp[:, None, :, :]).astype(F32)
    d2 = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).astype(F32)
    assert d2.dtype == F32
    md = d2.min(1)
    if mutant == "min_rows_ge16_dropped":
        md = md.copy()
        md[:, 16:] = md[:, :max(K - 16, 0)]
    lim = 16 if mutant == "inrange_tile0_only" else K
    in_range = real & (d2[:, :, :lim] < ext * ext).any(-1)
    d = np.sqrt(d2).astype(F32)
    if inf == CONSTANT:
        w = np.ones_like(d2)
    elif inf == LINEAR:
        w = np.maximum(F32(1) - d * (F32(1) / ext), F32(0)).astype(F32)
    else:
        w = np.exp(-d2 / F32(gauss_den(extent))).astype(F32)
    take = real if inf == LINEAR else in_range
    keep = np.broadcast_to(take[:, :, None], d2.shape).copy()
    if closest:
        cl = (K - 1 - np.argmin(d2[:, :, ::-1], axis=-1)) if mutant == "tie_high" else np.argmin(d2, axis=-1)
        keep &= np.arange(K)[None, None, :] == cl[:, :, None]
    w = (w * keep).astype(F32)                                                       # [nq, H, K]
    pos = x.astype(np.float64).sum(1)[idx] > 0
    cnt = ((real if mutant == "count_rigid" else in_range) & pos).sum(1)
    inv = (F32(1) / np.maximum(cnt, 1).astype(F32)).astype(F32)
    f = (m * inv[:, None]).astype(F32)                                               # [nq, K]
    xg = (x[idx] * real[:, :, None]).astype(F32)
    wk = w[:, :, _swap16(K)] if mutant == "tiles_swapped" else w
    wf = (np.einsum("qhk,qhc->qkc", wk, xg).astype(F32) * f[:, :, None]).astype(F32)
    g3 = (dwf.reshape(nq, K, cin) * f[:, :, None]).astype(F32)
    rows = np.einsum("qhk,qkc->qhc", wk, g3).astype(F32)
    P = np.einsum("qhc,qkc->qhk", xg, dwf.reshape(nq, K, cin)).astype(F32)
    dm = ((wk * P).sum(1, dtype=F32) * inv[:, None]).astype(F32)
    if inf == CONSTANT:
        dd = np.zeros((nq, K, 3), F32)
    elif inf == GAUSSIAN:
        coef = (wk * F32(F32(2) / F32(gauss_den(extent))) * P).astype(F32)
        dd = ((e * coef[..., None]).sum(1, dtype=F32) * f[:, :, None]).astype(F32)
    else:
        live = (wk > 0) & (d > 0)
        coef = np.where(live, P / np.where(live, d * ext, F32(1)), F32(0)).astype(F32)
        dd = ((e * coef[..., None]).sum(1, dtype=F32) * f[:, :, None]).astype(F32)
    return dict(wf=wf.reshape(nq, K * cin), min_d2=md, contrib=rows.reshape(nq * H, cin), d_mod=dm, d_dkp=dd, real=real)
