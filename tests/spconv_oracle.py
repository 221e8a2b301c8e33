"""Float64 statement of the sparse-convolution family (apr_amd/csrc/spconv.hip, spconv_ws.hip, spconv_os.hip,
spconv_bigk.hip, dense.hip, dense_rows.hip, spconv_bwd.hip) and the per-element float32 bounds its kernels are held to.
numpy only: no torch, no GPU.  tests/spconv_cases.py builds the named inputs, tests/test_spconv_oracle_cpu.py checks this
oracle against a triple loop and against oracle/me_oracle.py and shows that the cases reject one-rule mutants of the
kernels' structure, tests/test_spconv_edges_gpu.py holds the kernels to the bounds.

The operations
--------------
x [n_in, cin], W [K, cin, cout], nbr int32 [n_out, K] (-1 = no neighbour; None = the identity map, K = 1), dy [n_out, cout]
  forward          out[j] = act((sum_k [nbr[j,k] >= 0] x[nbr[j,k]] W[k]) * scale + shift + res[j]),  act = ReLU or none,
                   then optionally out[j] / |out[j]|_2
  kernel gradient  dW[k]  = sum_j [nbr[j,k] >= 0] x[nbr[j,k]]^T dy[j]
  input gradient   dx[i]  = sum over (j, k) with nbr[j,k] = i of dy[j] W[k]^T
The input gradient is stated over the FORWARD table.  The library computes it as a forward conv of dy over a reverse table
with flipped / transposed weights; none of those three enters here, so a wrong reverse map, flip or transpose shows.

The bounds (u = 2^-24, one float32 rounding; gamma(d) = d u / (1 - d u); every term is named where it is added)
----------------------------------------------------------------------------------------------------------------
An output element is a sum of n = a cin products, a = the row's active offsets.  A float32 sum of products in ANY
order in which no term passes through more than d roundings is within gamma(d) sum |x| |W| of the exact sum; zero terms
(padded pairs, padded channels, absent triple slots) add nothing.  d = (products of the chain) + (partial adds), per kernel:
  pairs      k_spconv_pairs    n + a ceil(cin / 32) + 3    every (offset, chunk) item's 16 x CN result is added into a
                                                            wave-private tile, the 4 tiles are summed in the epilogue
  mfma       k_spconv_mfma     n                            one accumulator through every offset and chunk
  smallcin   k_spconv_smallcin n                            one fma chain
  generic    k_spconv_generic  n                            one fma chain
  bigk       k_spconv_bigk     n + a ceil(cin / 32) + 3    the pairs kernel's structure over K <= 125
  dense      k_dense_gemm      n                            one accumulator over the chunks of cin
  ws         k_ws_gemm + k_ws_reduce          n + a        a product row per pair (one chain over cin), <= a adds in the reduce
The kernels on the bf16 3-way split (bf3.h) cut x = h + m + l and W = h' + m' + l' by truncation, exactly; of the nine
cross terms they keep six (h h', h m', m h', h l', l h', m m') and drop m l', l m', l l'.  The dropped terms are computed
here from the actual pieces,  drop = sum |m| |l'| + |l| |m'| + |l| |l'|,  the kept ones are exact products of bf16 values
summed in float32:  gamma(6 n + adds) kept,  kept = sum of the six |piece| |piece'| products.  adds per kernel:
  ws_bf3     k_ws_gemm_bf3 + k_ws_reduce      a            as ws
  ws3        k_ws3_gemm_bf3 + k_ws_reduce     9            a product row per triple entry, 9 ids per row in the reduce
  os         k_os_conv                        a            the accumulator row leaves and re-enters LDS once per offset (exact);
                                                            counted as adds all the same
  dense_bf3  k_dense_gemm_bf3                 0
  dense_rows k_dense_rows_bf3                 0
  wgrad_bf3  k_wgrad_bf3 + k_wgrad_reduce_work   n = pairs of offset k, adds = the offset's splits (S_all or S_c)
  wgrad_partial  k_wgrad_partial + k_wgrad_reduce  float32 MFMA: n = pairs of offset k, adds = the 512-row chunks
The epilogue (v * scale, + shift, + res) rounds once per step, each on the magnitude it produces (_step); ReLU is
1-Lipschitz and passes the bound through.  Row normalisation: an error e on the row moves y = v / |v| by at most
(e + |y| sum |y| e) / |v|, to which tests/norm_oracle.py's bound_l2 term of the float32 normalisation itself is added.
The bounds are worst-case: random data sits one to two decades below them (DESIGN 33 has the measured ratios).
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149

FP32_KERNELS = ("pairs", "mfma", "smallcin", "generic", "bigk", "dense", "ws")
BF3_KERNELS = ("ws_bf3", "ws3", "os", "dense_bf3", "dense_rows")


def cdiv(a, b):
    return -(-int(a) // int(b))


def gamma(d):
    d = np.asarray(d, np.float64)
    return d * U / (1.0 - d * U)


def identity_map(n):
    return np.arange(n, dtype=np.int32)[:, None]


def _table(nbr, n_out):
    return identity_map(n_out) if nbr is None else np.asarray(nbr)


# ------------------------------------------------------------------------------------------------------- the operations
def contract(x, nbr, W, n_out=None):
    """sum_k [nbr[j,k] >= 0] x[nbr[j,k]] W[k]  in float64 -> [n_out, cout]"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    nbr = _table(nbr, n_out if n_out is not None else len(x))
    out = np.zeros((nbr.shape[0], W.shape[2]))
    for k in range(nbr.shape[1]):
        j = np.nonzero(nbr[:, k] >= 0)[0]
        if len(j):
            out[j] += x[nbr[j, k]] @ W[k]
    return out


def epilogue(acc, scale=None, shift=None, res=None, relu=False):
    v = np.asarray(acc, np.float64)
    if scale is not None:
        v = v * np.asarray(scale, np.float64)
    if shift is not None:
        v = v + np.asarray(shift, np.float64)
    if res is not None:
        v = v + np.asarray(res, np.float64)
    return np.maximum(v, 0.0) + 0.0 * v if relu else v      # 0 * v keeps a NaN a NaN under the maximum


def l2_rows(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        return v / np.sqrt((v * v).sum(1, keepdims=True))


def conv_forward(x, nbr, W, scale=None, shift=None, res=None, relu=False, l2norm=False, n_out=None):
    v = epilogue(contract(x, nbr, W, n_out), scale, shift, res, relu)
    return l2_rows(v) if l2norm else v


def conv_wgrad(x, nbr, dy):
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    nbr = _table(nbr, len(dy))
    dw = np.zeros((nbr.shape[1], x.shape[1], dy.shape[1]))
    for k in range(nbr.shape[1]):
        j = np.nonzero(nbr[:, k] >= 0)[0]
        if len(j):
            dw[k] = x[nbr[j, k]].T @ dy[j]
    return dw


def conv_dx(dy, nbr, W, n_in):
    """from the forward table: dx[i] = sum over (j, k) with nbr[j,k] = i of dy[j] W[k]^T"""
    dy, W = np.asarray(dy, np.float64), np.asarray(W, np.float64)
    nbr = _table(nbr, len(dy))
    dx = np.zeros((n_in, W.shape[1]))
    for k in range(nbr.shape[1]):
        j = np.nonzero(nbr[:, k] >= 0)[0]
        if len(j):
            np.add.at(dx, nbr[j, k], dy[j] @ W[k].T)
    return dx


# ------------------------------------------------------------------------------------------------------------ the split
def split3(a):
    """bf3.h's split of float32 values: h, m, l as float64 arrays, each the top 8 significant bits of what is left
    (truncation); h + m + l == a exactly"""
    a = np.ascontiguousarray(a, np.float32)

    def top(v):
        return (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    with np.errstate(invalid="ignore"):
        h = top(a)
        r = (a - h).astype(np.float32)
        m = top(r)
        l = top((r - m).astype(np.float32))
    return h.astype(np.float64), m.astype(np.float64), l.astype(np.float64)


def _abs_products(a, nbr_like, b, fp32):
    """(kept, drop) magnitudes of sum over the table of |a| |b| -- for the fp32 kernels kept = sum |a| |b|, drop = 0;
    for the split kernels from the actual pieces.  a [rows, ca], b [K, ca, cb], gathered through nbr_like"""
    if fp32:
        return contract(np.abs(np.asarray(a, np.float64)), nbr_like, np.abs(np.asarray(b, np.float64))), 0.0
    ah, am, al = (np.abs(p) for p in split3(a))
    bh, bm, bl = (np.abs(p) for p in split3(b))
    kept = contract(ah, nbr_like, bh + bm + bl) + contract(am, nbr_like, bh + bm) + contract(al, nbr_like, bh)
    drop = contract(am, nbr_like, bl) + contract(al, nbr_like, bm + bl)
    return kept, drop


def _step(t, e):
    """one more float32 rounding, on a value |t| known to within e"""
    return e + U * (np.abs(t) + e)


def _adds(kernel, active, cin):
    if kernel in ("pairs", "bigk"):
        return active * cdiv(cin, 32) + 3          # one add into the private tile per (offset, chunk) item; 4 tiles
    if kernel in ("ws", "ws_bf3", "os"):
        return active                               # product rows of the row's offsets / the accumulator's round trips
    if kernel == "ws3":
        return 9 + 0 * active                       # nine triple ids per row
    return 0 * active                               # one chain


def forward_bound(kernel, x, nbr, W, scale=None, shift=None, res=None, relu=False, l2norm=False, n_out=None):
    """per-element bound on |kernel's out - conv_forward(...)|, [n_out, cout]; NaN where the oracle is NaN"""
    assert kernel in FP32_KERNELS + BF3_KERNELS, kernel
    fp32 = kernel in FP32_KERNELS
    W = np.asarray(W, np.float64)
    cin = W.shape[1]
    tbl = _table(nbr, n_out if n_out is not None else len(x))
    active = (tbl >= 0).sum(1).astype(np.float64)[:, None]
    kept, drop = _abs_products(x, tbl, W, fp32)
    depth = (1 if fp32 else 6) * active * cin + _adds(kernel, active, cin)
    e = gamma(depth) * kept + drop                          # the accumulation, then the dropped cross terms
    t = contract(x, tbl, W)
    if scale is not None:
        s = np.asarray(scale, np.float64)
        t, e = t * s, e * np.abs(s)
        e = _step(t, e)                                     # the product with scale
    if shift is not None:
        t = t + np.asarray(shift, np.float64)
        e = _step(t, e)                                     # + shift
    if res is not None:
        t = t + np.asarray(res, np.float64)
        e = _step(t, e)                                     # + residual
    if relu:
        t = np.maximum(t, 0.0) + 0.0 * t                    # 1-Lipschitz: e passes through
    if l2norm:
        with np.errstate(divide="ignore", invalid="ignore"):
            nrm = np.sqrt((t * t).sum(1, keepdims=True))
            y = t / nrm
            e = (e + np.abs(y) * (np.abs(y) * e).sum(1, keepdims=True)) / nrm      # the row's error through v / |v|
            P = cdiv(t.shape[1], 64)
            e = e + np.abs(y) * (0.5 * (P + 6) * U + 4 * U)                        # norm_oracle.bound_l2's term
    return e + TINY


def wgrad_bound(kernel, x, nbr, dy, splits):
    """per element of dW[k], relative to sum_j |x| |dy| over the offset's pairs; kernel 'wgrad_bf3' / 'wgrad_partial';
    splits [K]: partial sums per offset that the reduce kernel adds"""
    assert kernel in ("wgrad_bf3", "wgrad_partial")
    tbl = _table(nbr, len(dy))
    K = tbl.shape[1]
    x32, dy32 = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(dy, np.float32)
    out = np.zeros((K, x32.shape[1], dy32.shape[1]))
    for k in range(K):
        j = np.nonzero(tbl[:, k] >= 0)[0]
        if not len(j):
            continue                                         # an empty offset is exactly zero
        a, b = x32[tbl[j, k]], dy32[j]
        if kernel == "wgrad_partial":
            kept, drop, per = np.abs(a.astype(np.float64)).T @ np.abs(b.astype(np.float64)), 0.0, 1
        else:
            ah, am, al = (np.abs(p) for p in split3(a))
            bh, bm, bl = (np.abs(p) for p in split3(b))
            kept = ah.T @ (bh + bm + bl) + am.T @ (bh + bm) + al.T @ bh
            drop = am.T @ bl + al.T @ (bm + bl)
            per = 6
        out[k] = gamma(per * len(j) + int(splits[k])) * kept + drop      # the chains, the reduce's adds; the dropped terms
    return out + TINY


def dx_bound(kernel, dy, nbr, W, n_in):
    """the input gradient is a forward conv of dy (kernel as in forward_bound) whose row i has as many active offsets as
    (j, k) pairs reference i; its magnitudes come from the forward table like conv_dx itself"""
    assert kernel in FP32_KERNELS + BF3_KERNELS, kernel
    fp32 = kernel in FP32_KERNELS
    dy32, W32 = np.ascontiguousarray(dy, np.float32), np.ascontiguousarray(W, np.float32)
    tbl = _table(nbr, len(dy32))
    cout = W32.shape[2]
    refs = np.bincount(tbl[tbl >= 0].ravel(), minlength=n_in).astype(np.float64)[:, None]
    if fp32:
        kept, drop = conv_dx(np.abs(dy32), tbl, np.abs(W32), n_in), 0.0
    else:
        ah, am, al = (np.abs(p) for p in split3(dy32))
        bh, bm, bl = (np.abs(p) for p in split3(W32))
        kept = conv_dx(ah, tbl, bh + bm + bl, n_in) + conv_dx(am, tbl, bh + bm, n_in) + conv_dx(al, tbl, bh, n_in)
        drop = conv_dx(am, tbl, bl, n_in) + conv_dx(al, tbl, bm + bl, n_in)
    depth = (1 if fp32 else 6) * refs * cout + _adds(kernel, refs, cout)
    return gamma(depth) * kept + drop + TINY


# ------------------------------------------------------------------------------------------------------------ comparing
def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the finite elements of ref; the NaN patterns must be equal"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape == np.broadcast(ref, bound).shape
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "NaN pattern differs from the oracle's"
    if nan.all():
        return 0.0
    with np.errstate(invalid="ignore"):
        return float(np.max((np.abs(got - ref) / bound)[~nan]))
