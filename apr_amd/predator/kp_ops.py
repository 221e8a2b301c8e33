"""Tensor-level wrappers of the KPConv / overlap-attention kernels (all libapr_hip.so calls)."""
from __future__ import annotations

import ctypes as C
import math
import os

import torch

from .. import _lib, ops
from .._lib import check, ptr, stream


PROFILE = None   # set to a list to collect (N, H, cin, cout, K, start event, end event) per KPConv layer


def kpconv_profile_summary(records):
    """Algorithmic bytes / FLOP (bytes = 4*N*H*(3+cin) + 8*N*H + 4*N*cout; FLOP = 2*N*H*K*(3+cin) +
    2*N*K*cin*cout) and summed HIP-event time of the recorded KPConv layers."""
    torch.cuda.synchronize()
    tot = dict(launches=0, bytes=0.0, flops=0.0, ms=0.0)
    for (n, h, cin, cout, k, e0, e1) in records:
        tot["launches"] += 1
        tot["bytes"] += 4.0 * n * h * (3 + cin) + 8.0 * n * h + 4.0 * n * cout
        tot["flops"] += 2.0 * n * h * k * (3 + cin) + 2.0 * n * k * cin * cout
        tot["ms"] += e0.elapsed_time(e1)
    return tot


def tracking(*tensors):
    """Autograd is recording and one of the tensors / parameters takes part: the modules then run differentiable torch
    ops (the reference's own formulation) instead of the forward-only HIP kernels."""
    return torch.is_grad_enabled() and any(t is not None and torch.is_tensor(t) and t.requires_grad for t in tensors)


def gather_pad(x, inds):
    """x[inds] where index len(x) addresses an appended zero row (blocks.py:71-102 `gather` on the padded tensor)."""
    return torch.cat((x, torch.zeros_like(x[:1])), 0)[inds.long()]


def instance_norm_rows(x, eps):
    mu = x.mean(0, keepdim=True)
    var = x.var(0, unbiased=False, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps)


def _act(y, leaky, relu):
    if leaky is not None:
        return torch.nn.functional.leaky_relu(y, leaky)
    return torch.relu(y) if relu else y


def _i32(t, name):
    if t.dtype != torch.int32:
        t = t.to(torch.int32)
    if not t.is_cuda:
        raise _lib.AprHipError(f"{name}: need a GPU index tensor")
    return t.contiguous()


def linear(x, wp_info, shift=None, relu=False, out=None):
    """x [N,cin] @ W (packed by `pack_linear`) (+ shift) -> [N,cout] on the MFMA GEMM path.

    Channel counts that are not multiples of 32 (the decoder's 1282->129, 641->64, 320->34, the 256->1 score
    head) run zero-padded: W is padded once at pack time, x / shift per call; the result is a column slice.
    """
    wp, cin, cout, cin_p, cout_p, w_bf3 = wp_info
    if cin_p != cin or x.stride(0) % 4 != 0 or x.data_ptr() % 16 != 0:
        x = torch.nn.functional.pad(x, (0, cin_p - cin))
    if cout_p == cout:
        if w_bf3 is not None and DENSE_BF3 and (out is None or (out.stride(0) % 4 == 0 and out.data_ptr() % 16 == 0)) \
                and (shift is None or shift.data_ptr() % 16 == 0):
            # fp32-equivalent contraction on the bf16 MFMA (apr_dense_gemm_bf3): 1.5-1.7x the exact-fp32 kernel
            return ops.dense_gemm_bf3(x, w_bf3, cin_p, cout_p, shift=shift, relu=relu, out=out)
        return ops.spconv(x, None, 1, cin_p, cout_p, wp, shift=shift, relu=relu, out=out, n_out=x.shape[0])
    if shift is not None:
        shift = torch.nn.functional.pad(shift.view(-1), (0, cout_p - cout))
    y = ops.spconv(x, None, 1, cin_p, cout_p, wp, shift=shift, relu=relu, n_out=x.shape[0])[:, :cout]
    if out is not None:
        out.copy_(y)
        return out
    return y


def linear_norm_act(x, wp_info, eps=1e-5, leaky=None, relu=False, residual=None, segments=None, out=None):
    """act(instance_norm(x @ W) (+ residual)) in two launches (apr_dense_gemm_bf3_norm_act: the GEMM leaves its tiles'
    column sums behind, the apply kernel normalises in place) when both widths are multiples of 64; `linear` +
    `instance_norm_act` (three launches) otherwise.  `segments`: row offsets of the stacked scan pairs."""
    wp, cin, cout, cin_p, cout_p, w_bf3 = wp_info
    ok = (w_bf3 is not None and DENSE_BF3 and cin_p == cin and cout_p == cout and x.dim() == 2 and x.is_contiguous()
          and x.data_ptr() % 16 == 0 and not tracking(x, residual))
    if not ok:
        y = linear(x, wp_info)
        return instance_norm_act(y, eps=eps, leaky=leaky, relu=relu, residual=residual, out=out, segments=segments)
    n = x.shape[0]
    if out is None:
        out = torch.empty((n, cout), dtype=torch.float32, device=x.device)
    out, ldo = ops._rows(out, "linear_norm_act.out")
    ldr = 0
    if residual is not None:
        residual, ldr = ops._rows(residual, "linear_norm_act.residual")
    nseg = 0 if segments is None or len(segments) <= 2 else len(segments) - 1
    offs = (C.c_int64 * (nseg + 1))(*[int(v) for v in segments]) if nseg else None
    lib = _lib.load()
    sb = int(lib.apr_dense_gemm_bf3_norm_scratch_bytes(n, cout, max(nseg, 1)))
    scratch = torch.empty(sb, dtype=torch.uint8, device=x.device)
    mode = 2 if leaky is not None else int(bool(relu))
    check(lib.apr_dense_gemm_bf3_norm_act(ptr(x), x.stride(0), n, cin, cout, ptr(w_bf3), float(eps), ptr(residual), ldr, mode,
                                          float(leaky or 0.0), ptr(out), ldo, offs, nseg, ptr(scratch), sb, stream()))
    return out


class LinearFunction(torch.autograd.Function):
    """y = x @ W^T (nn.Linear without bias; KPFCNN's unary / bottleneck layers, Predator_APR/models/blocks.py:499-504) with
    forward, d x and d W on the HIP kernels: y and d x = dy @ W through the dense GEMM (`linear`), d W = dy^T x through
    apr_spconv_wgrad with the identity map (deterministic chunked reduction)."""

    @staticmethod
    def forward(ctx, x, weight, wp_info, bias=None):
        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        return linear(x, wp_info, shift=None if bias is None else bias.detach())

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        cout, cin = weight.shape
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = linear(dy, pack_linear(weight.detach()))          # [N, cout] @ [cout, cin]
        if ctx.needs_input_grad[1]:
            dw = ops.spconv_wgrad(x, dy, None, 1, cin, cout)[0].t()  # (x^T dy)^T
        if len(ctx.needs_input_grad) > 3 and ctx.needs_input_grad[3]:
            db = ops.col_sums(dy)                                  # the bias gradient: column sums, fp64 partials in fixed order
        return dx, dw, None, db


class LinearReluFunction(torch.autograd.Function):
    """relu(x @ W^T + b): nn.Linear followed by nn.ReLU as the NPR decoders stack them (Predator_APR/models/mlp.py:122-127,
    FCGF_APR/model/mlp.py:16-24).  Forward = the dense GEMM with the bias and the ReLU in its epilogue; backward =
    apr_act_backward on the saved output, then LinearFunction's three products."""

    @staticmethod
    def forward(ctx, x, weight, wp_info, bias):
        x = x.contiguous()
        y = linear(x, wp_info, shift=None if bias is None else bias.detach(), relu=True).contiguous()   # padded widths: a slice
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        dy = dy.contiguous()
        n, c = y.shape
        dz = torch.empty_like(dy)
        check(_lib.load().apr_act_backward(ptr(dy), c, ptr(y), c, n, c, 1, 0.0, ptr(dz), c, stream()))
        cout, cin = weight.shape
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = linear(dz, pack_linear(weight.detach()))
        if ctx.needs_input_grad[1]:
            dw = ops.spconv_wgrad(x, dz, None, 1, cin, cout)[0].t()
        if ctx.needs_input_grad[3]:
            db = ops.col_sums(dz)
        return dx, dw, None, db


def linear_train(x, weight, wp_info, bias=None):
    """The tracked (training) form of a Linear / 1x1 convolution on rows: forward, d x, d W (and d bias) on the HIP kernels
    (LinearFunction)."""
    if HIP_TRAIN_LINEAR and x.shape[0] > 0 and x.dim() == 2:      # any width: `linear` pads to the GEMM's granule
        return LinearFunction.apply(x, weight, wp_info, bias)
    return torch.nn.functional.linear(x, weight, bias)


HIP_TRAIN_LINEAR = os.environ.get("APR_HIP_TRAIN_LINEAR", "1") != "0"   # A/B switch: 0 = torch's Linear in training
HIP_TRAIN_NORM = os.environ.get("APR_HIP_TRAIN_NORM", "1") != "0"   # A/B switch: 0 = torch ops for the training-mode norms
DENSE_BF3 = os.environ.get("APR_DENSE_BF3", "1") != "0"     # A/B switch: 0 keeps every Linear on the exact-fp32 MFMA


def pack_linear(w_in_out, bf3=True):
    """[cin, cout] weight -> (packed, cin, cout, cin_padded, cout_padded, bf16 3-way split image or None).
    The split image exists when both padded channel counts are multiples of 64 (apr_dense_gemm_bf3)."""
    w = w_in_out.detach().to(torch.float32)
    cin, cout = w.shape
    cin_p, cout_p = (cin + 31) // 32 * 32, (cout + 31) // 32 * 32
    if (cin_p, cout_p) != (cin, cout):
        w = torch.nn.functional.pad(w, (0, cout_p - cout, 0, cin_p - cin))
    w = w.contiguous()
    w_bf3 = ops.pack_weights_bf3(w[None]) if (bf3 and DENSE_BF3 and cin_p % 64 == 0 and cout_p % 64 == 0) else None
    return ops.pack_weights(w), cin, cout, cin_p, cout_p, w_bf3


def row_sums(x):
    x, ld = ops._rows(x, "row_sums.x")
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    check(_lib.load().apr_row_sums(ptr(x), ld, x.shape[0], x.shape[1], ptr(out), stream()))
    return out


INFLUENCES = {"constant": 0, "linear": 1, "gaussian": 2}      # KP_influence -> the `influence` argument of the *_mode entries
AGGREGATIONS = {"sum": 0, "closest": 1}                        # aggregation_mode -> `closest`
DEFAULT_MODE = (1, 0)      # linear influence, sum aggregation: the entry points without a mode


def kpconv_mode(KP_influence, aggregation_mode):
    """(KP_influence, aggregation_mode) of the reference's KPConv -> (influence, closest); ValueError with the reference's
    messages (blocks.py:337, 345) for anything else."""
    if KP_influence not in INFLUENCES:
        raise ValueError('Unknown influence function type (config.KP_influence)')
    if aggregation_mode not in AGGREGATIONS:
        raise ValueError("Unknown convolution mode. Should be 'closest' or 'sum'")
    return INFLUENCES[KP_influence], AGGREGATIONS[aggregation_mode]


def influence_torch(sq, extent, mode):
    """The influences of blocks.py:320-345 on torch ops: sq [n, h, k] squared distances -> w [n, h, k].  Linear takes
    sqrt(max(d2, 1e-30)): a zero geometry gradient for a neighbour exactly on a kernel point, as the kernels give; the
    one-hot of the closest kernel point is a constant of the graph.  (The in-range filter of a deformable layer is the
    caller's: it zeroes the features of the neighbours outside every ball.)"""
    influence, closest = mode
    if influence == 0:
        w = torch.ones_like(sq)
    elif influence == 1:
        w = torch.clamp(1 - torch.sqrt(torch.clamp(sq, min=1e-30)) / extent, min=0.0)
    else:
        sigma = extent * 0.3
        w = torch.exp(-sq / (2 * sigma ** 2 + 1e-9))
    if closest:
        w = w * torch.nn.functional.one_hot(torch.argmin(sq, dim=2), sq.shape[2]).to(w.dtype)
    return w


# A/B switch: 0 sends cin = 32 (the first layer of KPFCNNDecoder) to apr_kpconv_weighted's generic kernel instead of
# apr_kpconv_weighted_c32 (DESIGN section 35 has the measurement behind the default)
KPCONV_C32 = os.environ.get("APR_KPCONV_C32", "1") != "0"


def kpconv_weighted(q_pts, s_pts, nbr, x, kernel_points, extent, mode=DEFAULT_MODE):
    """KPConv step 1 -> weighted features [Nq, ld] (ld = K*cin rounded up to 32, the padding exact zeros), already /
    neighbour count.  mode = (influence, closest) of apr_kpconv_weighted_mode.  Default mode, cin = 32, rows on 8-byte
    boundaries: apr_kpconv_weighted_c32 (KPCONV_C32).  K = kernel_points.shape[0] other than 15: apr_kpconv_weighted_nk
    (1 <= K <= 32; csrc/kpconv_nk.hip)."""
    nbr = _i32(nbr, "kpconv.nbr")
    x, ldx = ops._rows(x, "kpconv.x")
    nq, ns, cin = q_pts.shape[0], s_pts.shape[0], x.shape[1]
    kk = kernel_points.shape[0] * cin
    ld = (kk + 31) // 32 * 32
    wf = torch.zeros((nq, ld), dtype=torch.float32, device=x.device) if ld != kk else \
        torch.empty((nq, ld), dtype=torch.float32, device=x.device)
    rs = row_sums(x)
    qp, sp, kp = q_pts.contiguous(), s_pts.contiguous(), kernel_points.contiguous()
    args = (ptr(qp), nq, ptr(sp), ns, ptr(nbr), nbr.shape[1], ptr(x), ldx, cin, ptr(kp), kp.shape[0], float(extent), ptr(rs),
            ptr(wf), ld)
    if tuple(mode) == DEFAULT_MODE and KPCONV_C32 and cin == 32 and kernel_points.shape[0] == 15 \
            and 1 <= nbr.shape[1] <= 128 and ldx % 2 == 0 and x.data_ptr() % 8 == 0:
        # the MFMA correlation of the symmetric generator's first layer
        check(_lib.load().apr_kpconv_weighted_c32(*args, stream()))
    elif kernel_points.shape[0] != 15:
        check(_lib.load().apr_kpconv_weighted_nk(*args, int(mode[0]), int(mode[1]), stream()))
    else:
        check(_lib.load().apr_kpconv_weighted_mode(*args, int(mode[0]), int(mode[1]), stream()))
    return wf


def rows_aligned(x, c):
    """float32 GPU matrix of `c` columns whose rows start on 16-byte boundaries (what apr_kpconv_fused reads)"""
    return bool(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == c
                and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0)


def kpconv_fused(q_pts, s_pts, nbr, x, kernel_points, extent, w_info, out=None):
    """Rigid KPConv forward in one kernel (apr_kpconv_fused): correlation and contraction, the weighted features never
    reach memory.  `w_info`: `pack_linear` of W.reshape(15 * cin, cout) (its bf16-split image is read).  Forward only;
    shapes and layouts the kernel does not take raise (the callers fall back, not this wrapper)."""
    nbr = _i32(nbr, "kpconv_fused.nbr")
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise _lib.AprHipError("kpconv_fused.x: need a float32 GPU matrix with unit column stride")
    if not (q_pts.is_cuda and s_pts.is_cuda and kernel_points.is_cuda):
        raise _lib.AprHipError("kpconv_fused: the points and the kernel points must be GPU tensors")
    _, cin, cout, cin_p, cout_p, w_bf3 = w_info
    nq, ns = q_pts.shape[0], s_pts.shape[0]
    n_kp = kernel_points.shape[0]
    if w_bf3 is None or cin_p != cin or cout_p != cout or cin != n_kp * x.shape[1]:
        raise _lib.AprHipError("kpconv_fused: the weights need a bf16-split image of [15 * cin, cout]")
    if out is None:
        out = torch.empty((nq, cout), dtype=torch.float32, device=x.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (nq, cout) and out.stride(1) == 1):
        raise _lib.AprHipError("kpconv_fused.out: need a float32 GPU [nq, cout] matrix with unit column stride")
    rs = row_sums(x)
    check(_lib.load().apr_kpconv_fused(ptr(q_pts.contiguous()), nq, ptr(s_pts.contiguous()), ns, ptr(nbr), nbr.shape[1], ptr(x),
                                       x.stride(0), x.shape[1], ptr(kernel_points.contiguous()), n_kp, float(extent), ptr(rs),
                                       ptr(w_bf3), cout, ptr(out), out.stride(0), stream()))
    return out


_REV_CACHE = {}     # (data_ptr, shape, version, ns) -> (nbr tensor kept alive, rev_t, start): one build per neighbour table


def reverse_table(nbr, ns):
    """Flat positions of `nbr` [nq, H] sorted by the support row they point at + the start of every row's run
    (apr_reverse_table_build; stable, deterministic).  Cached per table: the layers of a pyramid level share theirs."""
    key = (nbr.data_ptr(), tuple(nbr.shape), nbr._version, int(ns))
    hit = _REV_CACHE.get(key)
    if hit is not None:
        return hit[1], hit[2]
    if len(_REV_CACHE) > 16:
        _REV_CACHE.clear()
    lib = _lib.load()
    nq, H = nbr.shape
    rev_t = torch.empty(nq * H, dtype=torch.int32, device=nbr.device)
    start = torch.empty(int(ns) + 1, dtype=torch.int32, device=nbr.device)
    sb = int(lib.apr_reverse_table_scratch_bytes(nq, H, int(ns)))
    scratch = torch.empty(sb, dtype=torch.uint8, device=nbr.device)
    check(lib.apr_reverse_table_build(ptr(nbr), nq, H, int(ns), ptr(rev_t), ptr(start), ptr(scratch), sb, stream()))
    _REV_CACHE[key] = (nbr, rev_t, start)
    return rev_t, start


DET_DX = os.environ.get("APR_KPCONV_DX", "det") != "atomic"     # A/B switch: "atomic" = round 2's float-atomic scatter
DX_CHUNK_BYTES = int(os.environ.get("APR_KPCONV_DX_CHUNK_MB", "64")) << 20     # contribution rows in flight per chunk


class KPConvFunction(torch.autograd.Function):
    """Rigid KPConv (blocks.py:229-374) with forward AND both gradients on the HIP kernels:
    forward   wf = step 1 (apr_kpconv_weighted), out = wf @ W (dense MFMA GEMM);
    d W       = wf^T @ dout                       (apr_spconv_wgrad, identity map; wf is recomputed, not stored);
    d x       = scatter of (dout @ W^T) through the influences (apr_kpconv_dfeat on the forward's neighbour table).
    The points, the kernel points and the neighbour table get no gradient (rigid kernel).
    mode = (influence, closest): the *_mode entry points; d x of a mode other than the default exists in the deterministic
    form only (apr_kpconv_dfeat_contrib_mode).  A kernel-point count other than 15 (1 <= K <= 32) runs the *_nk entry points
    (csrc/kpconv_nk.hip): the deterministic d x only, in every mode."""

    @staticmethod
    def forward(ctx, q_pts, s_pts, inds, x, weights, kernel_points, extent, mode=DEFAULT_MODE):
        inds = _i32(inds, "kpconv.nbr")
        x = x.contiguous()
        K, cin, cout = weights.shape
        ctx.mode = mode = (int(mode[0]), int(mode[1]))
        wf = kpconv_weighted(q_pts, s_pts, inds, x, kernel_points, extent, mode)
        w2 = weights.detach().reshape(K * cin, cout)
        if wf.shape[1] != K * cin:
            w2 = torch.cat([w2, torch.zeros((wf.shape[1] - K * cin, cout), dtype=w2.dtype, device=w2.device)], 0)
        out = linear(wf, pack_linear(w2, bf3=False))
        ctx.save_for_backward(q_pts, s_pts, inds, x, weights, kernel_points)
        ctx.extent = float(extent)
        return out

    @staticmethod
    def backward(ctx, dout):
        q_pts, s_pts, inds, x, weights, kernel_points = ctx.saved_tensors
        K, cin, cout = weights.shape
        dout = dout.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[4]:
            wf = kpconv_weighted(q_pts, s_pts, inds, x, kernel_points, ctx.extent, ctx.mode)
            dw = ops.spconv_wgrad(wf, dout, None, 1, wf.shape[1], cout)[0, :K * cin].reshape(K, cin, cout)
        if ctx.needs_input_grad[3]:
            dwf = linear(dout, pack_linear(weights.detach().reshape(K * cin, cout).t().contiguous(), bf3=False))   # [nq, K*cin]
            dwf, lddwf = ops._rows(dwf, "kpconv.dwf")
            rs = row_sums(x)
            lib = _lib.load()
            nq, H, ns = q_pts.shape[0], inds.shape[1], s_pts.shape[0]
            contrib_fn = lib.apr_kpconv_dfeat_contrib_mode if K == 15 else lib.apr_kpconv_dfeat_contrib_nk
            if DET_DX and cin % 4 == 0 and nq * H < (1 << 31):
                # deterministic: one contribution row per (query, neighbour), summed per support row in the fixed order of the
                # reverse table (no float atomics: the same bits every run).  The queries go through in chunks whose
                # contribution rows fit DX_CHUNK_BYTES (64 MB; unchunked the finest level of one pair needs 400 MB): a
                # support row's run is ascending in the flat position q * H + h, so chunk after chunk the gather continues
                # the same sequence of additions -- the bits do not depend on the chunk size (tested).
                rev_t, start = reverse_table(inds, ns)
                qc = max(1, min(nq, DX_CHUNK_BYTES // max(1, H * cin * 4)))
                contrib = torch.empty((min(nq, qc) * H, cin), dtype=torch.float32, device=x.device)
                dx = torch.empty_like(x)
                qp, sp, kp = q_pts.contiguous(), s_pts.contiguous(), kernel_points.contiguous()
                for q0 in range(0, nq, qc):
                    q1 = min(nq, q0 + qc)
                    check(contrib_fn(ptr(qp[q0:q1]), q1 - q0, ptr(sp), ns, ptr(inds[q0:q1]), H, ptr(dwf[q0:q1]), lddwf, cin,
                                     ptr(kp), kp.shape[0], ctx.extent, ptr(rs), ptr(contrib), ctx.mode[0], ctx.mode[1], stream()))
                    check(lib.apr_reverse_gather_range(ptr(contrib), cin, ptr(rev_t), ptr(start), ns, q0 * H, q1 * H,
                                                       int(q0 > 0), ptr(dx), dx.stride(0), stream()))
            else:
                if ctx.mode != DEFAULT_MODE or K != 15:
                    raise _lib.AprHipError("kpconv: the atomic d x (apr_kpconv_dfeat) is linear influence / sum aggregation and "
                                           "15 kernel points only")
                dx = torch.zeros_like(x)
                check(lib.apr_kpconv_dfeat(ptr(q_pts.contiguous()), nq, ptr(s_pts.contiguous()), ns, ptr(inds), H, ptr(dwf),
                                           lddwf, cin, ptr(kernel_points.contiguous()), kernel_points.shape[0], ctx.extent,
                                           ptr(rs), ptr(dx), dx.stride(0), stream()))
        return None, None, None, dx, dw, None, None, None


def deform_ok(x, cin, H, K=15):
    """Shapes and layouts the deformable kernels take (apr_kpconv_deform_*_mode at 15 kernel points, apr_kpconv_deform_*_nk at
    any other count from 1 to 32): cin a multiple of 64 up to 512, 1 <= H <= 128, float32 GPU rows on 16-byte boundaries.
    Everything else runs the torch formulation.  (d W goes through apr_spconv_wgrad over [nq, K cin]: it tiles any width,
    so K cin up to 32 * 512 = 16384 stays on the kernels.)"""
    return 1 <= K <= 32 and cin % 64 == 0 and 64 <= cin <= 512 and 1 <= H <= 128 and rows_aligned(x, cin)


def kpconv_deform_weighted(q_pts, s_pts, nbr, x, dkp, mod, extent, want_min_d2=True, mode=DEFAULT_MODE):
    """Deformable KPConv step 1 -> (wf [nq, K * cin], min_d2 [nq, K] or None), K = dkp.shape[1]: 15 kernel points run
    apr_kpconv_deform_weighted_mode, any other count from 1 to 32 apr_kpconv_deform_weighted_nk (csrc/kpconv_deform_nk.hip).
    dkp [nq, K, 3]: the query's own kernel points; mod [nq, K] or None; wf is already mod / (in-range count).
    mode = (influence, closest)."""
    nbr = _i32(nbr, "kpconv_deform.nbr")
    x, ldx = ops._rows(x, "kpconv_deform.x")
    nq, ns, cin = q_pts.shape[0], s_pts.shape[0], x.shape[1]
    K = dkp.shape[1] if dkp.dim() == 3 else 0
    if tuple(dkp.shape) != (nq, K, 3) or not 1 <= K <= 32 or (mod is not None and tuple(mod.shape) != (nq, K)):
        raise _lib.AprHipError("kpconv_deform: dkp must be [nq, K, 3] with 1 <= K <= 32 and mod [nq, K]")
    assert (K * cin) % 64 == 0      # cin % 64 == 0 (deform_ok): the packed weight rows need no zero padding
    dkp = dkp.detach().to(torch.float32).contiguous()
    mod = None if mod is None else mod.detach().to(torch.float32).contiguous()
    wf = torch.empty((nq, K * cin), dtype=torch.float32, device=x.device)
    md = torch.empty((nq, K), dtype=torch.float32, device=x.device) if want_min_d2 else None
    rs = row_sums(x)
    lib = _lib.load()
    fn = lib.apr_kpconv_deform_weighted_mode if K == 15 else lib.apr_kpconv_deform_weighted_nk
    check(fn(ptr(q_pts.contiguous()), nq, ptr(s_pts.contiguous()), ns, ptr(nbr), nbr.shape[1], ptr(x), ldx, cin, ptr(dkp),
             ptr(mod), K, float(extent), ptr(rs), ptr(wf), wf.stride(0), ptr(md), int(mode[0]), int(mode[1]), stream()))
    return wf, md


class KPConvDeformFunction(torch.autograd.Function):
    """Deformable / modulated KPConv (blocks.py:229-374) on the HIP kernels, given the query's kernel points dkp
    [nq, K, 3] and modulations mod [nq, K] (or None): returns (out, min_d2).  K = 15 runs the apr_kpconv_deform_*_mode
    entries, any other count from 1 to 32 the apr_kpconv_deform_*_nk ones (csrc/kpconv_deform_nk.hip).
    forward   wf = apr_kpconv_deform_weighted, out = wf @ W (dense MFMA GEMM); min_d2 is not differentiable (nothing in the
              reference differentiates it);
    d W       = wf^T @ dout (apr_spconv_wgrad; wf recomputed);
    d x       = apr_kpconv_deform_dfeat_contrib + apr_reverse_gather_range in DX_CHUNK_BYTES chunks (deterministic);
    d dkp, d mod = apr_kpconv_deform_dgeom.
    The in-range count is a constant of the graph.  The points and the neighbour table get no gradient.
    mode = (influence, closest): the *_mode entry points.  With the constant influence dkp gets None as its gradient, as in
    the reference's graph (the kernel's d_dkp is exactly 0)."""

    @staticmethod
    def forward(ctx, q_pts, s_pts, inds, x, weights, dkp, mod, extent, mode=DEFAULT_MODE):
        inds = _i32(inds, "kpconv_deform.nbr")
        x = x.contiguous()
        K, cin, cout = weights.shape
        ctx.mode = mode = (int(mode[0]), int(mode[1]))
        wf, md = kpconv_deform_weighted(q_pts, s_pts, inds, x, dkp, mod, extent, mode=mode)
        out = linear(wf, pack_linear(weights.detach().reshape(K * cin, cout), bf3=False))
        ctx.save_for_backward(q_pts, s_pts, inds, x, weights, dkp, mod)
        ctx.extent = float(extent)
        ctx.mark_non_differentiable(md)
        return out, md

    @staticmethod
    def backward(ctx, dout, _dmin):
        q_pts, s_pts, inds, x, weights, dkp, mod = ctx.saved_tensors
        K, cin, cout = weights.shape
        dout = dout.contiguous()
        dx = dw = ddkp = dmod = None
        if ctx.needs_input_grad[4]:
            wf, _ = kpconv_deform_weighted(q_pts, s_pts, inds, x, dkp, mod, ctx.extent, want_min_d2=False, mode=ctx.mode)
            dw = ops.spconv_wgrad(wf, dout, None, 1, wf.shape[1], cout)[0].reshape(K, cin, cout)
        need_geom = (ctx.needs_input_grad[5] and ctx.mode[0] != 0) or (mod is not None and ctx.needs_input_grad[6])
        if ctx.needs_input_grad[3] or need_geom:
            dwf = linear(dout, pack_linear(weights.detach().reshape(K * cin, cout).t().contiguous(), bf3=False))
            dwf, lddwf = ops._rows(dwf, "kpconv_deform.dwf")
            rs = row_sums(x)
            lib = _lib.load()
            nq, H, ns = q_pts.shape[0], inds.shape[1], s_pts.shape[0]
            qp, sp = q_pts.contiguous(), s_pts.contiguous()
            kd = dkp.detach().contiguous()
            md = None if mod is None else mod.detach().contiguous()
            contrib_fn = lib.apr_kpconv_deform_dfeat_contrib_mode if K == 15 else lib.apr_kpconv_deform_dfeat_contrib_nk
            dgeom_fn = lib.apr_kpconv_deform_dgeom_mode if K == 15 else lib.apr_kpconv_deform_dgeom_nk
            if ctx.needs_input_grad[3]:
                if nq * H >= (1 << 31):
                    raise _lib.AprHipError("kpconv_deform: neighbour table too large for the reverse table")
                rev_t, start = reverse_table(inds, ns)
                qc = max(1, min(nq, DX_CHUNK_BYTES // max(1, H * cin * 4)))
                contrib = torch.empty((min(nq, qc) * H, cin), dtype=torch.float32, device=x.device)
                dx = torch.empty_like(x)
                for q0 in range(0, nq, qc):
                    q1 = min(nq, q0 + qc)
                    check(contrib_fn(ptr(qp[q0:q1]), q1 - q0, ptr(sp), ns, ptr(inds[q0:q1]), H, ptr(dwf[q0:q1]), lddwf, cin,
                                     ptr(kd[q0:q1]), ptr(None if md is None else md[q0:q1]), K, ctx.extent, ptr(rs),
                                     ptr(contrib), ctx.mode[0], ctx.mode[1], stream()))
                    check(lib.apr_reverse_gather_range(ptr(contrib), cin, ptr(rev_t), ptr(start), ns, q0 * H, q1 * H,
                                                       int(q0 > 0), ptr(dx), dx.stride(0), stream()))
            if need_geom:
                ddkp = torch.empty((nq, K, 3), dtype=torch.float32, device=x.device)
                dmod = torch.empty((nq, K), dtype=torch.float32, device=x.device)
                check(dgeom_fn(ptr(qp), nq, ptr(sp), ns, ptr(inds), H, ptr(x), x.stride(0), cin, ptr(dwf), lddwf, ptr(kd),
                               ptr(md), K, ctx.extent, ptr(rs), ptr(ddkp), ptr(dmod), ctx.mode[0], ctx.mode[1], stream()))
                if mod is None:
                    dmod = None
                if ctx.mode[0] == 0:
                    ddkp = None
        return None, None, None, dx, dw, ddkp, dmod, None, None


def gather_pool(x, inds, mode, out=None):
    """mode 'max' -> max_pool(x, inds); 'closest' -> closest_pool(x, inds).  `out`: a [nq, c] column slice to write into."""
    inds = _i32(inds, "gather_pool.inds")
    x, ldx = ops._rows(x, "gather_pool.x")
    nq, c = inds.shape[0], x.shape[1]
    if out is None:
        out = torch.empty((nq, c), dtype=torch.float32, device=x.device)
    out, ldo = ops._rows(out, "gather_pool.out")
    if tuple(out.shape) != (nq, c):
        raise _lib.AprHipError("gather_pool: output shape mismatch")
    check(_lib.load().apr_gather_pool(ptr(x), ldx, x.shape[0], c, ptr(inds), inds.shape[1], nq,
                                      1 if mode == "closest" else 0, ptr(out), ldo, stream()))
    return out


class PoolFunction(torch.autograd.Function):
    """max_pool / closest_pool (blocks.py:71-102) with forward and backward on the HIP kernels: the forward records which
    neighbour gave each maximum (apr_gather_pool_argmax), the backward gathers dout over the reverse table of the index tensor
    (apr_gather_pool_backward: deterministic, the same bits every run).  Training path; inference keeps gather_pool."""

    @staticmethod
    def forward(ctx, x, inds, mode):
        inds = _i32(inds, "pool.inds")
        x = x.contiguous()
        ns, c = x.shape
        nq, H = inds.shape
        lib = _lib.load()
        amax = None
        if mode == "max":
            out = torch.empty((nq, c), dtype=torch.float32, device=x.device)
            amax = torch.empty((nq, c), dtype=torch.uint8, device=x.device)
            check(lib.apr_gather_pool_argmax(ptr(x), c, ns, c, ptr(inds), H, nq, ptr(out), c, ptr(amax), stream()))
        else:
            out = gather_pool(x, inds, "closest")
        ctx.save_for_backward(inds, amax if amax is not None else inds)
        ctx.cfg = (mode, int(ns), int(c))
        return out

    @staticmethod
    def backward(ctx, dout):
        inds, amax = ctx.saved_tensors
        mode, ns, c = ctx.cfg
        if not ctx.needs_input_grad[0]:
            return None, None, None
        dout = dout.contiguous()
        rev_t, start = reverse_table(inds, ns)
        dx = torch.empty((ns, c), dtype=torch.float32, device=dout.device)
        check(_lib.load().apr_gather_pool_backward(ptr(dout), c, c, ptr(rev_t), ptr(start), ns, inds.shape[1],
                                                   ptr(amax) if mode == "max" else None, 0 if mode == "max" else 1, ptr(dx), c,
                                                   stream()))
        return dx, None, None


HIP_TRAIN_POOL = os.environ.get("APR_HIP_TRAIN_POOL", "1") != "0"     # A/B switch: 0 = torch indexing for the pools in training


def pool_train(x, inds, mode):
    """The tracked (training) form of max_pool / closest_pool: HIP kernels when the table is narrow enough for the u8 arg-max."""
    if HIP_TRAIN_POOL and x.dim() == 2 and x.shape[0] > 0 and inds.shape[0] > 0 and inds.shape[1] <= 255:
        return PoolFunction.apply(x, inds, mode)
    g = gather_pad(x, inds if mode == "max" else inds[:, 0])
    return g.max(1)[0] if mode == "max" else g


def edge_features(f, knn):
    knn = _i32(knn, "edge_features.knn")
    f, ldf = ops._rows(f, "edge_features.f")
    n, c = f.shape
    out = torch.empty((n * knn.shape[1], 2 * c), dtype=torch.float32, device=f.device)
    check(_lib.load().apr_edge_features(ptr(f), ldf, n, c, ptr(knn), knn.shape[1], ptr(out), stream()))
    return out


class EdgeFeaturesFunction(torch.autograd.Function):
    """get_graph_feature as rows (gcn.py:9-35): e[(i, j)] = [f_i, f_knn(i, j) - f_i], with the input gradient on the HIP
    kernels: the centre's own terms by apr_edge_features_backward, the neighbours' terms gathered over the reverse table of
    the kNN graph in table order (apr_reverse_gather_range): deterministic, no float atomics."""

    @staticmethod
    def forward(ctx, f, knn):
        knn = _i32(knn, "edge_features.knn").contiguous()
        ctx.save_for_backward(knn)
        ctx.n, ctx.c = f.shape
        return edge_features(f.detach(), knn)

    @staticmethod
    def backward(ctx, de):
        knn, = ctx.saved_tensors
        n, c, k = ctx.n, ctx.c, knn.shape[1]
        de = de.contiguous()
        lib = _lib.load()
        dx = torch.empty((n, c), dtype=torch.float32, device=de.device)
        contrib = torch.empty((n * k, c), dtype=torch.float32, device=de.device)
        check(lib.apr_edge_features_backward(ptr(de), n, c, k, ptr(dx), c, ptr(contrib), stream()))
        rev_t, start = reverse_table(knn, n)
        check(lib.apr_reverse_gather_range(ptr(contrib), c, ptr(rev_t), ptr(start), n, 0, n * k, 1, ptr(dx), c, stream()))
        return dx, None


_GROUP_INDS = {}


def group_rows(n, k, device):
    """int32 [n, k] = the rows i*k + j of an [n*k, c] edge tensor (cached): max over a point's k edges is max_pool over it."""
    key = (n, k, device)
    t = _GROUP_INDS.get(key)
    if t is None:
        if len(_GROUP_INDS) > 8:
            _GROUP_INDS.clear()
        t = _GROUP_INDS[key] = torch.arange(n * k, dtype=torch.int32, device=device).view(n, k)
    return t


def group_max(y, n, k, scale, shift, slope):
    y, ldy = ops._rows(y, "group_max.y")
    c = y.shape[1]
    out = torch.empty((n, c), dtype=torch.float32, device=y.device)
    check(_lib.load().apr_group_max(ptr(y), ldy, n, k, c, ptr(scale), ptr(shift), float(slope), ptr(out), c, stream()))
    return out


def mha(q, k, v, heads):
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    n, c = q.shape
    out = torch.empty_like(q)
    check(_lib.load().apr_mha(ptr(q), ptr(k), ptr(v), n, k.shape[0], c // heads, heads, ptr(out), stream()))
    return out


class MHAFunction(torch.autograd.Function):
    """Multi-head softmax attention (gcn.py:94-116, channel c = d*heads + h) with forward and backward on the HIP kernels
    (apr_mha_train_forward / _backward): the forward keeps the probabilities, every sum has a fixed order."""

    @staticmethod
    def forward(ctx, q, k, v, heads):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        n, c = q.shape
        m, cv = k.shape[0], v.shape[1]          # v may be narrower than q / k (the cross saliency: one column)
        P = torch.empty((heads, n, m), dtype=torch.float32, device=q.device)
        out = torch.empty((n, cv), dtype=torch.float32, device=q.device)
        check(_lib.load().apr_mha_train_forward(ptr(q), ptr(k), ptr(v), n, m, c // heads, heads, cv // heads, ptr(P), ptr(out),
                                                stream()))
        ctx.save_for_backward(q, k, v, P)
        ctx.heads = heads
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, P = ctx.saved_tensors
        heads = ctx.heads
        n, c = q.shape
        m, cv = k.shape[0], v.shape[1]
        dout = dout.contiguous()
        dS = torch.empty_like(P)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        check(_lib.load().apr_mha_train_backward(ptr(q), ptr(k), ptr(v), ptr(P), ptr(dout), n, m, c // heads, heads, cv // heads,
                                                 ptr(dS), ptr(dq), ptr(dk), ptr(dv), stream()))
        return dq, dk, dv, None


def softmax_matvec_train(a, b, w, temperature):
    """softmax_j(<a_i, b_j> / temperature) @ w under autograd on the HIP attention kernels (one head, one value column):
    the scores are <q_i, b_j> / sqrt(c) with q = a * (sqrt(c) / temperature) -- that scaling is the only torch op, and it
    carries the gradient of the learned temperature."""
    c = a.shape[1]
    q = a * (math.sqrt(c) / temperature)
    return MHAFunction.apply(q, b, w.reshape(-1, 1), 1).reshape(-1)


HIP_TRAIN_MHA = os.environ.get("APR_HIP_TRAIN_MHA", "1") != "0"     # A/B switch: 0 = the attention of the training path on torch ops
MHA_MFMA = os.environ.get("APR_MHA", "mfma") != "scalar"      # A/B switch: the scalar kernel on interleaved channels


def mha_headmajor(q, k, v, heads):
    """`mha` with q / k / v head-major (channel h*dim + d); the result is in `mha`'s interleaved layout."""
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    n, c = q.shape
    out = torch.empty_like(q)
    check(_lib.load().apr_mha_headmajor(ptr(q), ptr(k), ptr(v), n, k.shape[0], c // heads, heads, ptr(out), stream()))
    return out


# the geometric cross attention's inference route: the MFMA kernel (dim 64); scalar = the training entry points (A/B switch)
MHA_CAT_MFMA = os.environ.get("APR_MHA_CAT", "mfma") != "scalar"


def _cat_coords(c, rows, name):
    if not c.is_cuda or c.dim() != 2 or c.shape[0] != rows or c.shape[1] != 3:
        raise _lib.AprHipError(f"{name}: need a [{rows}, 3] GPU tensor of coordinates")
    return c.detach().to(torch.float32).contiguous()


def mha_cat_headmajor(q, k, v, c0, c1, heads, padded=False):
    """The geometric cross attention ('cross_cat', gcn.py:131-156) with q / k / v head-major (channel h*dim + d), dim = 64:
    y [n, (dim+7)*heads], channel e*heads + h = feat | soft | aug1 | aug2.  The rows live in a buffer padded to the GEMM's
    granule of 32 columns with the pad zeroed; `padded` returns that whole buffer (what `linear_padded` reads)."""
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    n, c = q.shape
    m = k.shape[0]
    cy = (c // heads + 7) * heads
    ld = (cy + 31) // 32 * 32
    c0, c1 = _cat_coords(c0, n, "mha_cat.c0"), _cat_coords(c1, m, "mha_cat.c1")      # named: a converted copy lives past the launch
    y = torch.empty((n, ld), dtype=torch.float32, device=q.device)
    if ld > cy:
        y[:, cy:].zero_()
    check(_lib.load().apr_mha_cat_headmajor(ptr(q), ptr(k), ptr(v), ptr(c0), ptr(c1), n, m, c // heads, heads, ptr(y), ld, stream()))
    return y if padded else y[:, :cy]


def linear_padded(xp, wp_info, shift=None):
    """`linear` on rows the caller already padded with zeros to the packed width (no pad copy)."""
    wp, cin, cout, cin_p, cout_p, w_bf3 = wp_info
    if xp.shape[1] != cin_p or xp.stride(0) % 4 != 0 or xp.data_ptr() % 16 != 0 or xp.stride(1) != 1:
        return linear(xp[:, :cin], wp_info, shift=shift)
    if cout_p == cout and w_bf3 is not None and DENSE_BF3 and (shift is None or shift.data_ptr() % 16 == 0):
        return ops.dense_gemm_bf3(xp, w_bf3, cin_p, cout_p, shift=shift)
    if shift is not None and cout_p != cout:
        shift = torch.nn.functional.pad(shift.view(-1), (0, cout_p - cout))
    return ops.spconv(xp, None, 1, cin_p, cout_p, wp, shift=shift, n_out=xp.shape[0])[:, :cout]


class MHACatFunction(torch.autograd.Function):
    """The geometric cross attention on interleaved channels (c = d*heads + h) with forward and backward on the HIP kernels
    (apr_mha_cat_train_forward / _backward): the forward keeps the probabilities and y, every sum has a fixed order.  The
    coordinates take no gradient."""

    @staticmethod
    def forward(ctx, q, k, v, c0, c1, heads):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        n, c = q.shape
        m = k.shape[0]
        c0, c1 = _cat_coords(c0, n, "mha_cat.c0"), _cat_coords(c1, m, "mha_cat.c1")
        cy = (c // heads + 7) * heads
        P = torch.empty((heads, n, m), dtype=torch.float32, device=q.device)
        y = torch.empty((n, cy), dtype=torch.float32, device=q.device)
        check(_lib.load().apr_mha_cat_train_forward(ptr(q), ptr(k), ptr(v), ptr(c0), ptr(c1), n, m, c // heads, heads, ptr(P), ptr(y),
                                                    cy, stream()))
        ctx.save_for_backward(q, k, v, c0, c1, P, y)
        ctx.heads = heads
        return y

    @staticmethod
    def backward(ctx, dy):
        q, k, v, c0, c1, P, y = ctx.saved_tensors
        heads = ctx.heads
        n, c = q.shape
        m = k.shape[0]
        dy = dy.contiguous()
        dS = torch.empty_like(P)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        check(_lib.load().apr_mha_cat_train_backward(ptr(q), ptr(k), ptr(v), ptr(c0), ptr(c1), ptr(P), ptr(y), ptr(dy), y.shape[1], n, m,
                                                     c // heads, heads, ptr(dS), ptr(dq), ptr(dk), ptr(dv), stream()))
        return dq, dk, dv, None, None, None


def mha_cat_torch(q, k, v, c0, c1, heads):
    """The layer's statement in torch ops (gcn.py:142-156 on rows): the route when HIP_TRAIN_MHA is off or dim > 1024."""
    n, c = q.shape
    dim = c // heads
    qh, kh, vh = (t.view(-1, dim, heads) for t in (q, k, v))                      # channel c = d*heads + h
    prob = torch.softmax(torch.einsum('ndh,mdh->hnm', qh, kh) / dim ** .5, dim=-1)
    feat = torch.einsum('hnm,mdh->ndh', prob, vh)
    soft = torch.einsum('hnm,ma->nah', prob, c1.detach().to(q.dtype))
    aug1 = soft - c0.detach().to(q.dtype)[:, :, None]
    aug2 = torch.norm(aug1, dim=1, keepdim=True)
    return torch.cat([feat, soft, aug1, aug2], dim=1).reshape(n, -1)


def mha_cat_route(q, heads):
    """'train': `mha_cat` takes the HIP training entry points; 'torch': the torch-op statement."""
    hip = HIP_TRAIN_MHA and q.is_cuda and q.dtype == torch.float32 and q.shape[1] // heads <= 1024
    return 'train' if hip else 'torch'


def mha_cat(q, k, v, c0, c1, heads):
    """The geometric cross attention on interleaved channels: the HIP training entry points, or torch ops."""
    if mha_cat_route(q, heads) == 'train':
        return MHACatFunction.apply(q, k, v, c0, c1, heads)
    return mha_cat_torch(q, k, v, c0, c1, heads)


def softmax_matvec(a, b, w, temperature):
    a, w = a.contiguous(), w.contiguous().view(-1)
    out = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    n, m, c = a.shape[0], b.shape[0], a.shape[1]
    if c in (32, 64, 128, 256) and a.data_ptr() % 16 == 0:
        b = b.contiguous()
        if b.data_ptr() % 16 == 0:
            check(_lib.load().apr_softmax_matvec_mfma(ptr(a), ptr(b), ptr(w), n, m, c, float(temperature), ptr(out),
                                                      stream()))
            return out
    if 4 * (m + c) * 4 <= 60 * 1024:
        bt = b.t().contiguous()          # [c, m]: the kernel's lanes run along the keys
        check(_lib.load().apr_softmax_matvec_bt(ptr(a), ptr(bt), ptr(w), n, m, c, float(temperature), ptr(out), stream()))
    else:
        check(_lib.load().apr_softmax_matvec(ptr(a), ptr(b.contiguous()), ptr(w), n, m, c, float(temperature), ptr(out),
                                             stream()))
    return out


def score_head(x_col):
    """x_col: a [N] column view (stride allowed) -> clamp(sigmoid(x)) with NaN/Inf -> 0."""
    n = x_col.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=x_col.device)
    check(_lib.load().apr_score_head(ptr(x_col), x_col.stride(0), n, ptr(out), stream()))
    return out


class NormActFunction(torch.autograd.Function):
    """act(instance_norm(x) (+ residual)) -- KPFCNN's BatchNormBlock + LeakyReLU (+ shortcut), blocks.py:459-468, 489, 574,
    653-681 -- with forward AND backward on the HIP kernels: the forward is the fused inference launch pair
    (apr_instance_norm_act[_seg]); the backward turns dy into dz through the activation's own output (apr_act_backward), hands
    dz to the residual branch as it is, and runs apr_norm_backward per pair segment with the segment's statistics
    (apr_bn_stats, recomputed: nothing but x and the output is kept).  No torch op between them."""

    @staticmethod
    def forward(ctx, x, residual, eps, leaky, relu, segments):
        x = x.contiguous()
        res = residual.contiguous() if residual is not None else None
        with torch.no_grad():
            y = instance_norm_act(x.detach(), eps=eps, leaky=leaky, relu=relu,
                                  residual=None if res is None else res.detach(), segments=segments)
        ctx.save_for_backward(x, y)
        ctx.cfg = (float(eps), leaky, bool(relu), None if segments is None else list(segments), res is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        eps, leaky, relu, segments, has_res = ctx.cfg
        dy = dy.contiguous()
        n, c = x.shape
        mode = 2 if leaky is not None else int(relu)
        dz = dy
        if mode:
            dz = torch.empty_like(dy)
            check(_lib.load().apr_act_backward(ptr(dy), c, ptr(y), c, n, c, mode, float(leaky or 0.0), ptr(dz), c, stream()))
        dx = None
        if ctx.needs_input_grad[0]:
            segs = segments if (segments is not None and len(segments) > 2) else [0, n]
            dx = torch.empty_like(x)
            for a, b in zip(segs[:-1], segs[1:]):
                mean, var = ops.bn_stats(x[a:b])
                rstd = torch.rsqrt(var + eps)
                ops.norm_backward(x[a:b], dz[a:b], mean, rstd, None, want_affine_grads=False, out=dx[a:b])
        return dx, (dz if has_res and ctx.needs_input_grad[1] else None), None, None, None, None


HIP_TRAIN_NORMACT = os.environ.get("APR_HIP_TRAIN_NORMACT", "1") != "0"   # A/B switch: 0 = norm on HIP, activation / residual add in torch


def instance_norm_act(x, eps=1e-5, leaky=None, relu=False, residual=None, out=None, segments=None):
    """Per-channel normalisation over all rows, no affine (InstanceNorm1d on [1,C,N]) + activation.
    `segments`: row offsets [0, ..., n] of the scan pairs stacked in x (one statistic per pair and channel)."""
    if segments is not None and len(segments) <= 2:
        segments = None
    if tracking(x, residual):
        if HIP_TRAIN_NORM and HIP_TRAIN_NORMACT and x.dim() == 2 and x.shape[0] > 0:
            # training: the fused forward launches, and a backward of apr_act_backward + apr_norm_backward (no torch op)
            return NormActFunction.apply(x, residual, eps, leaky, relu, segments)
        # statistics, normalisation and its backward on the HIP kernels (ops.NormFunction, no affine); the
        # activation / residual add as elementwise torch ops
        nf = lambda t: ops.NormFunction.apply(t, None, None, eps)[0] if HIP_TRAIN_NORM else instance_norm_rows(t, eps)
        if segments is None:
            y = nf(x)
        else:
            y = torch.cat([nf(x[a:b]) for a, b in zip(segments[:-1], segments[1:])], 0)
        return _act(y if residual is None else y + residual, leaky, relu)
    if segments is not None:
        x, ldx = ops._rows(x, "instance_norm_act.x")
        n, c = x.shape
        if out is None:
            out = torch.empty((n, c), dtype=torch.float32, device=x.device)
        out, ldy = ops._rows(out, "instance_norm_act.out")
        ldr = 0
        if residual is not None:
            residual, ldr = ops._rows(residual, "instance_norm_act.residual")
        lib = _lib.load()
        nseg = len(segments) - 1
        sb = int(lib.apr_bn_stats_scratch_bytes(n + 256 * nseg, c))
        scratch = torch.empty(sb, dtype=torch.uint8, device=x.device)
        offs = (C.c_int64 * (nseg + 1))(*[int(v) for v in segments])
        mode = 2 if leaky is not None else int(bool(relu))
        check(lib.apr_instance_norm_act_seg(ptr(x), ldx, n, c, float(eps), ptr(residual), ldr, mode, float(leaky or 0.0),
                                            ptr(out), ldy, offs, nseg, ptr(scratch), sb, stream()))
        return out
    x, ldx = ops._rows(x, "instance_norm_act.x")
    n, c = x.shape
    if out is None:
        out = torch.empty((n, c), dtype=torch.float32, device=x.device)
    out, ldy = ops._rows(out, "instance_norm_act.out")
    ldr = 0
    if residual is not None:
        residual, ldr = ops._rows(residual, "instance_norm_act.residual")
    lib = _lib.load()
    sb = int(lib.apr_bn_stats_scratch_bytes(n, c))
    scratch = torch.empty(sb, dtype=torch.uint8, device=x.device)
    mode = 2 if leaky is not None else int(bool(relu))
    check(lib.apr_instance_norm_act(ptr(x), ldx, n, c, float(eps), ptr(residual), ldr, mode, float(leaky or 0.0),
                                    ptr(out), ldy, ptr(scratch), sb, stream()))
    return out
