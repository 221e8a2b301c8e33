"""Shared test helpers: seeded inputs + oracle/HIP model pairs driven by one state_dict."""
import numpy as np
import torch

from apr_amd import ops, synth
from oracle import me_oracle as OME
from oracle import resunet_oracle as OR


def voxelized_frame(seed, small=True, voxel_size=0.3, n_beams=None, n_azimuth=None):
    if n_beams is not None:
        xyz = synth.make_frame(seed, n_beams=n_beams, n_azimuth=n_azimuth)
    else:
        xyz = synth.make_small_frame(seed) if small else synth.make_frame(seed)
    c, sel = OME.sparse_quantize(xyz / np.float32(voxel_size), return_index=True)
    return xyz, c, sel


def batched_input(seeds, **kw):
    coords = [voxelized_frame(s, **kw)[1] for s in seeds]
    C = OME.batched_coordinates(coords)
    F = np.ones((len(C), 1), np.float32)
    return C, F


def model_pair(name, out_channels=32, conv1_kernel_size=5, seed=0, in_channels=1):
    """(oracle model, HIP model on cuda) sharing one randomly initialised state_dict."""
    from apr_amd.fcgf.model import load_model
    torch.manual_seed(seed)
    om = OR.MODELS[name](in_channels, out_channels, bn_momentum=0.05, normalize_feature=True,
                         conv1_kernel_size=conv1_kernel_size, D=3)
    OR.randomize_bn_stats(om, seed)
    hm = load_model(name)(in_channels, out_channels, bn_momentum=0.05, normalize_feature=True,
                          conv1_kernel_size=conv1_kernel_size, D=3)
    missing = hm.load_state_dict(om.state_dict(), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return om, hm.cuda()


def rel_l2(a, b):
    a = torch.as_tensor(a, dtype=torch.float64)
    b = torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# launch entry points of the conv routes (ops.spconv / dense_*): the name of each route
ROUTES = {"apr_spconv_ws3_fwd_bf3": "ws3", "apr_spconv_ws_fwd_bf3": "ws", "apr_spconv_fwd": "tile",
          "apr_spconv_os_fwd": "os", "apr_dense_gemm_bf3": "dense", "apr_dense_rows_bf3": "dense"}


class _LibProxy:
    """Stands in for the loaded library behind ops._lib_(): every call is logged by entry-point name."""

    def __init__(self, lib):
        self._lib = lib
        self.log = []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not callable(fn):
            return fn

        def call(*args):
            self.log.append(name)
            return fn(*args)
        return call


def _routes(names):
    return {ROUTES[n] for n in names if n in ROUTES}


def _recording_function(nodes, proxy):
    """ops.ConvBnActFunction that records each node's inputs, outputs, running statistics, gradients and routes."""
    base = ops.ConvBnActFunction

    def cl(t):
        return None if t is None else t.detach().clone()

    class Recording(base):
        @staticmethod
        def forward(ctx, x, kernel, gamma, beta, bias, residual, cfg):
            bn = cfg["bn"].bn if cfg["bn"] is not None else None
            rec = dict(x=cl(x), x_grad=x.requires_grad, kernel=cl(kernel), gamma=cl(gamma), beta=cl(beta), bias=cl(bias),
                       residual=cl(residual), cfg=cfg)
            if bn is not None:
                rec.update(rm=cl(bn.running_mean), rv=cl(bn.running_var), nbt=int(bn.num_batches_tracked))
            start = len(proxy.log)
            y = base.forward(ctx, x, kernel, gamma, beta, bias, residual, cfg)
            rec.update(y=cl(y), fwd=_routes(proxy.log[start:]))
            if bn is not None:
                rec.update(rm_after=cl(bn.running_mean), rv_after=cl(bn.running_var), nbt_after=int(bn.num_batches_tracked))
            ctx.rec = len(nodes)
            nodes.append(rec)
            return y

        @staticmethod
        def backward(ctx, dy):
            start = len(proxy.log)
            grads = base.backward(ctx, dy)
            nodes[ctx.rec].update(dy=cl(dy), grads=[cl(g) for g in grads[:6]], bwd=_routes(proxy.log[start:]))
            return grads

    return Recording


# coordinate level (tensor stride) of each stage of ResUNet2, by the module name of its fused training node
LEVEL = {"conv1": 1, "block1": 1, "conv2": 2, "block2": 2, "conv3": 4, "block3": 4, "conv4": 8, "block4": 8,
         "conv4_tr": 4, "block4_tr": 4, "conv3_tr": 2, "block3_tr": 2, "conv2_tr": 1, "block2_tr": 1, "conv1_tr": 1, "final": 1}


class EncoderRecorder:
    """Records the fused training nodes (ops.ConvBnActFunction) of a HIP ResUNet2 in train mode: every node's inputs,
    outputs, gradients and routes (`nodes`, `proxy.log`), the coordinate manager of each forward_train call, and from them
    the ReLU decisions as pins for the oracle (resunet_oracle.ResUNet2.forward)."""

    def __init__(self, monkeypatch, hm):
        self.proxy = _LibProxy(ops._lib_())
        monkeypatch.setattr(ops, "_lib_", lambda: self.proxy)
        self.nodes = []
        monkeypatch.setattr(ops, "ConvBnActFunction", _recording_function(self.nodes, self.proxy))
        self.calls = []
        self.names = {id(m): n for n, m in hm.named_modules()}
        real = hm.forward_train

        def forward_train(x, frame_rows=None):
            self.calls.append((x.coordinate_manager, len(self.nodes), frame_rows))
            return real(x, frame_rows=frame_rows)
        monkeypatch.setattr(hm, "forward_train", forward_train)

    def routes(self, nodes=None):
        nodes = self.nodes if nodes is None else nodes
        return (set().union(*(r["fwd"] for r in nodes)), set().union(*(r.get("bwd", set()) for r in nodes)))

    def pins(self, frame_coords, calls=None):
        """One {module name: (coords, mask)} per frame the reference encodes separately, in call order.  A node's mask is
        its own y > 0 with the rows of the HIP map at its level; a stacked call (forward_frames) is split by the node's
        row segments and the frames' batch indices shifted back."""
        out, f = [], 0
        for cm, first, rows in (self.calls if calls is None else calls):
            nodes = self.nodes[first:first + 23]
            assert len(nodes) == 23, len(nodes)
            nf = len(rows) if rows else 1
            shifts = [0]
            for g in range(1, nf):
                shifts.append(shifts[-1] + int(np.asarray(frame_coords[f + g - 1])[:, 0].max()) + 1)
            per = [dict() for _ in range(nf)]
            for rec in nodes:
                if not rec["cfg"]["relu"]:
                    continue
                name = self.names[id(rec["cfg"]["conv"])]
                ts = LEVEL[name.split(".")[0]]
                coords = cm.get_map(ts).coords[:cm.size(ts)].cpu().numpy()
                mask = (rec["y"] > 0).cpu()
                assert coords.shape[0] == mask.shape[0], (name, coords.shape, mask.shape)
                segs = rec["cfg"]["segs"] if nf > 1 else [0, coords.shape[0]]
                assert len(segs) == nf + 1, (name, segs)
                for g in range(nf):
                    c = coords[segs[g]:segs[g + 1]].copy()
                    c[:, 0] -= shifts[g]
                    per[g][name] = (c, mask[segs[g]:segs[g + 1]])
            out.extend(per)
            f += nf
        return out


class ReluSpy:
    """Watches the oracle's pinned ReLUs: where the float64 pre-activation's sign disagrees with the pinned mask, how many
    entries and how far from 0 relative to that site's RMS.  A pin applied a second time (the identity ReLU on a block's
    output) is not counted again."""

    def __init__(self, monkeypatch):
        from oracle import me_oracle as OME
        real = OME.relu
        self.sites, self._seen = [], set()

        def relu(x, pin=None):
            out = real(x, pin)
            if pin is not None and id(pin) not in self._seen:
                self._seen.add(id(pin))
                z, o = x.F.detach(), out.F.detach()
                flip = ((z > 0) & (o == 0)) | ((z < 0) & (o == z))
                rms = float(z.pow(2).mean().sqrt())
                worst = float(z[flip].abs().max()) / rms if bool(flip.any()) else 0.0
                self.sites.append((int(flip.sum()), worst, z.numel()))
            return out
        monkeypatch.setattr(OME, "relu", relu)

    def reset(self):
        self.sites.clear()
        self._seen.clear()

    def summary(self):
        """(flipped entries, worst |z| / rms over them, entries watched)"""
        return (sum(s[0] for s in self.sites), max((s[1] for s in self.sites), default=0.0), sum(s[2] for s in self.sites))


def oracle_copy(name, state, out_channels, dtype=torch.float64):
    """The oracle ResUNet2 `name` in `dtype` on the CPU with the given (HIP) state_dict, in train mode."""
    om = OR.MODELS[name](1, out_channels, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3)
    om.load_state_dict({k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu())
                        for k, v in state.items()})
    return om.to(dtype).train()


def stat_err(hip, ref):
    """Running statistics: max |hip - ref| / (|ref| + 1e-3 max |ref|)."""
    ref = torch.as_tensor(ref).double().cpu()
    return float(((torch.as_tensor(hip).double().cpu() - ref).abs() / (ref.abs() + 1e-3 * ref.abs().max())).max())
