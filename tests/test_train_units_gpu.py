"""Every fused training unit (ops.ConvBnActFunction: routed sparse conv -> training-mode BatchNorm -> (+ residual) -> ReLU)
of real training steps, node by node, against a float64 rebuild of the same unit from the node's own recorded inputs.

The whole-network comparisons in test_backward_gpu.py need a 1e-2 bar on the routed backward (a ReLU kink flips between two
summation orders, DESIGN.md "A ReLU on the kink"), so they cannot see a gradient that is 0.5 % off.  Here every node is rebuilt
on its own: the gather / index_add convolution over cfg["nbr"] (never the reverse maps, the flipped-transposed packs or the
weight-stationary lists), BatchNorm with the batch statistics of each row segment, the residual, the ReLU; autograd of the
rebuild gives the reference gradients.  The ReLU mask is the HIP node's own (y > 0): at an entry within fp32 noise of zero
both masks are valid subgradients; that the fp64 forward disagrees with it at only a handful of entries is asserted too.

Worst values per node, measured on an MI355X over the seven route cases and the four bias units below (relative L2; running
statistics as max |hip - ref| / (|ref| + 1e-3 max |ref|)): y 3.5e-7, din 2.8e-7, dW 6.2e-7, dres 0 (exact), dgamma 3.6e-7,
dbeta 3.5e-8, dbias of the final layer 2.8e-8, running_mean 3.8e-6, running_var 2.0e-7, mask disagreements 0, and
|dbias| / |dz| 5.1e-7 for a conv bias ahead of a BatchNorm (fp64 value 0).  Each bar is 2.6 - 11x its measured value
(dres, exact here, shares din's).  For scale: backward weights rounded to plain bf16 give din 1.7e-3 on every node."""
import numpy as np
import pytest
import torch

from apr_amd import MinkowskiEngine as ME
from apr_amd import ops, synth
from apr_amd.fcgf.model import resunet as RU
from oracle import me_oracle as OME
from tests.helpers import _LibProxy, _recording_function, model_pair, rel_l2

pytestmark = pytest.mark.gpu

BARS = {"y": 2e-6, "din": 3e-6, "dres": 3e-6, "dW": 5e-6, "dgamma": 3e-6, "dbeta": 4e-7, "dbias": 3e-7,
        "running_mean": 1e-5, "running_var": 2e-6,
        "dbias/|dz|": 5e-6}      # a conv bias ahead of a BatchNorm: |hip - fp64| / |dz| where the fp64 value is 0

def _ref_unit(rec):
    """float64 rebuild of one recorded node -> (y, mask disagreements, {name: (hip, ref)} of the gradients,
    [(name, hip, ref)] of the running statistics, |dL/dz| of the conv output)."""
    cfg = rec["cfg"]
    conv, norm = cfg["conv"], cfg["bn"]
    x = rec["x"].double().requires_grad_(rec["x_grad"])
    W = rec["kernel"].double().requires_grad_(True)
    W3 = W if W.dim() == 3 else W.unsqueeze(0)
    nbr = cfg["nbr"]
    if nbr is None:
        z = x @ W3[0]
    else:
        z = torch.zeros(nbr.shape[0], W3.shape[2], dtype=torch.float64, device=x.device)
        for k in range(nbr.shape[1]):
            j = torch.nonzero(nbr[:, k] >= 0).squeeze(1)
            if len(j):
                z = z.index_add(0, j, x[nbr[j, k].long()] @ W3[k])
    leaves = {"din": x, "dW": W}
    if rec["bias"] is not None:
        b = rec["bias"].double().requires_grad_(True)
        z = z + b.view(1, -1)
        leaves["dbias"] = b
    z.retain_grad()
    zc = z
    stats = []
    if norm is not None:
        bn = norm.bn
        g = rec["gamma"].double().requires_grad_(True)
        beta = rec["beta"].double().requires_grad_(True)
        leaves.update(dgamma=g, dbeta=beta)
        segs = cfg.get("segs") or [0, z.shape[0]]
        rm, rv, mom = rec["rm"].double(), rec["rv"].double(), bn.momentum
        parts = []
        for a, e in zip(segs[:-1], segs[1:]):
            zs = z[a:e]
            mean, var = zs.mean(0), zs.var(0, unbiased=False)
            parts.append((zs - mean) / torch.sqrt(var + bn.eps) * g + beta)
            with torch.no_grad():
                rm = (1 - mom) * rm + mom * mean
                rv = (1 - mom) * rv + mom * zs.var(0, unbiased=True)
        z = torch.cat(parts, 0)
        stats = [("running_mean", rec["rm_after"], rm), ("running_var", rec["rv_after"], rv)]
        assert rec["nbt_after"] - rec["nbt"] == len(segs) - 1
    if rec["residual"] is not None:
        r = rec["residual"].double().requires_grad_(True)
        z = z + r
        leaves["dres"] = r
    flips = 0
    if cfg["relu"]:
        mask = rec["y"] > 0                              # the HIP node's own mask (see the module docstring)
        flips = int((mask != (z > 0)).sum())
        y = z * mask
    else:
        y = z
    (y * rec["dy"].double()).sum().backward()
    hip = dict(zip(("din", "dW", "dgamma", "dbeta", "dbias", "dres"), rec["grads"]))
    pairs = {}
    for name, leaf in leaves.items():
        if leaf.requires_grad:
            pairs[name] = (hip[name], leaf.grad)
    return y.detach(), flips, pairs, stats, float(zc.grad.norm())


def _stat_err(hip, ref):
    ref = ref.double()
    return float(((hip.double() - ref).abs() / (ref.abs() + 1e-3 * ref.abs().max())).max())


def _check_nodes(nodes, tag):
    """Every node against its fp64 rebuild; prints the worst values per quantity, then asserts the bars."""
    worst, fails = {}, []

    def note(q, v, bar, i):
        worst[q] = max(worst.get(q, 0.0), v)
        if not v <= bar:
            fails.append(f"node {i} {q} {v:.2e} > {bar:.0e}")

    for i, rec in enumerate(nodes):
        assert "grads" in rec, f"node {i} got no backward"
        y, flips, pairs, stats, dz_norm = _ref_unit(rec)
        note("y", rel_l2(rec["y"], y), BARS["y"], i)
        n = rec["y"].numel()
        note("mask_flips", flips, max(2, 1e-5 * n), i)
        for q, (h, r) in pairs.items():
            assert h is not None, f"node {i}: no {q} from the HIP node"
            if q == "dbias" and rec["cfg"]["bn"] is not None:      # fp64 value 0: bounded against the conv output's gradient
                note("dbias/|dz|", float((h.reshape(r.shape).double() - r).norm()) / dz_norm, BARS["dbias/|dz|"], i)
            else:
                note(q, rel_l2(h.reshape(r.shape), r), BARS[q], i)
        for q, h, r in stats:
            note(q, _stat_err(h, r), BARS[q], i)
    print(f"[{tag}] {len(nodes)} nodes, worst: " + ", ".join(f"{q} {v:.2e}" for q, v in sorted(worst.items())))
    assert not fails, fails
    return worst


def _frame(seed, beams, azimuth, voxel):
    xyz, _, _ = synth.make_pair(seed, n_beams=beams, n_azimuth=azimuth)
    c, _ = OME.sparse_quantize(xyz / np.float32(voxel), return_index=True)
    return OME.batched_coordinates([c])


# (network, out channels, frames as (seed, beams, azimuth, voxel), environment, WS3_MAX_ROWS_128 or None,
#  routes that must run in backward, routes that must never run)
CASES = {
    "BN2C-default": ("ResUNetBN2C", 32, [(6, 32, 900, 0.3)], {}, None, {"ws3", "ws", "tile"}, set()),
    "FatBN-default": ("ResUNetFatBN", 128, [(4, 16, 800, 0.3)], {}, None, {"ws3", "ws", "tile", "dense"}, set()),
    # a frame whose stride-8 level has 62 rows (fewer than one 64-row tile)
    "BN2C-ws3off": ("ResUNetBN2C", 32, [(3, 16, 500, 2.0)], {"APR_WS3": "0"}, None, {"ws", "tile"}, {"ws3"}),
    "FatBN-ws3off": ("ResUNetFatBN", 128, [(11, 16, 600, 0.5)], {"APR_WS3": "0"}, None, {"ws", "tile", "dense"}, {"ws3"}),
    "BN2E-ws128": ("ResUNetBN2E", 32, [(12, 16, 600, 0.45)], {}, 16, {"ws", "ws3", "tile"}, set()),
    "BN2C-tile": ("ResUNetBN2C", 32, [(11, 16, 600, 0.5)], {"APR_WS_STAGES": "none"}, None, {"tile"}, {"ws3", "ws", "os"}),
    "FatBN-frames": ("ResUNetFatBN", 128, [(6, 32, 900, 0.3), (3, 32, 800, 0.3)], {}, None, {"ws3", "ws", "tile", "dense"},
                     set()),
}


@pytest.mark.parametrize("case", list(CASES))
def test_training_step_units_match_fp64(dev, case, monkeypatch):
    """One training forward + backward through ResUNet2.forward_train (forward_frames for two stacked frames): every one of
    the 23 nodes against its fp64 rebuild, and the routes each case stands for asserted to have run in backward."""
    name, out_ch, frames, env, ws3_max, need, never = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if ws3_max is not None:
        monkeypatch.setattr(RU, "WS3_MAX_ROWS_128", ws3_max)
    proxy = _LibProxy(ops._lib_())
    monkeypatch.setattr(ops, "_lib_", lambda: proxy)
    nodes = []
    monkeypatch.setattr(ops, "ConvBnActFunction", _recording_function(nodes, proxy))
    _, hm = model_pair(name, out_ch, seed=7)
    hm.train()
    xs = [ME.SparseTensor(torch.ones(len(C), 1, device=dev), coordinates=torch.from_numpy(C).to(dev))
          for C in (_frame(*f) for f in frames)]
    ys = hm.forward_frames(xs) if len(xs) > 1 else [hm(xs[0])]
    assert len(nodes) == 23, len(nodes)                       # the fused path ran (not the module-by-module one)
    g = torch.Generator().manual_seed(1)
    sum((y.F * torch.randn(tuple(y.F.shape), generator=g).to(dev)).sum() for y in ys).backward()

    # level sizes: none a multiple of 64 (so of 512 either); the ws3-off BN2C frame has a level below 64 rows
    sizes = sorted({rec["x"].shape[0] for rec in nodes} | {rec["y"].shape[0] for rec in nodes})
    assert all(n % 64 for n in sizes), sizes
    if case == "BN2C-ws3off":
        assert min(sizes) < 64, sizes
    if case == "FatBN-frames":
        assert all(rec["cfg"]["segs"] is not None and len(rec["cfg"]["segs"]) == 3 for rec in nodes if rec["cfg"]["bn"])

    _check_nodes(nodes, case)

    bwd = set().union(*(rec["bwd"] for rec in nodes))
    fwd = set().union(*(rec["fwd"] for rec in nodes))
    assert need <= bwd, (need, bwd)
    assert not (never & (bwd | fwd)), (never, bwd | fwd)
    if ws3_max is not None:
        # every same-level 128-channel map larger than the cap took the per-offset lists, forward and backward
        big = [rec for rec in nodes if rec["cfg"]["flip"] and rec["cfg"]["conv"].in_channels == 128
               and rec["cfg"]["plist"] is not None and rec["x"].shape[0] > ws3_max]
        assert big and all(rec["fwd"] == {"ws"} and rec["bwd"] == {"ws"} for rec in big), \
            [(rec["fwd"], rec["bwd"]) for rec in big]
    # a step builds a tile pack for exactly the launches that read one: forward and backward launches of the tile kernel
    # (the weight-stationary lists and the dense K = 1 kernels read the bf16-split images alone)
    tile_launches = proxy.log.count("apr_spconv_fwd")
    assert proxy.log.count("apr_spconv_pack_weights") == tile_launches, \
        (proxy.log.count("apr_spconv_pack_weights"), tile_launches)


def _unit_case(dev, cin, cout, K, relu, residual, route, seed):
    """A bare ConvBnActFunction node with conv bias=True ahead of its BatchNorm (no network has one), same-level map."""
    rng = np.random.default_rng(seed)
    C = _frame(seed, 16, 500, 0.4)
    x = ME.SparseTensor(torch.ones(len(C), 1, device=dev), coordinates=torch.from_numpy(C).to(dev))
    cm = x.coordinate_manager
    n = cm.size(1)
    conv = ME.MinkowskiConvolution(cin, cout, kernel_size=3 if K == 27 else 1, stride=1, bias=True, dimension=3).to(dev)
    norm = ME.MinkowskiBatchNorm(cout, momentum=0.1).to(dev)
    with torch.no_grad():
        conv.bias.copy_(torch.from_numpy(rng.uniform(1.0, 3.0, (1, cout)).astype(np.float32)))    # far from 0: visible
        norm.bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, cout).astype(np.float32)))
        norm.bn.bias.copy_(torch.from_numpy(rng.uniform(-0.5, 0.5, cout).astype(np.float32)))
    m = (1, 1, 3, False)
    nbr = cm.kernel_map(*m) if K == 27 else None
    pl = None
    if route in ("ws3", "ws"):
        pl = cm.pair_list(*m, triples=route == "ws3")
    cfg = dict(conv=conv, bn=norm, nbr=nbr, plist=pl, nbr_bwd=nbr, plist_bwd=pl, flip=nbr is not None, relu=relu, n_out=n,
               segs=None)
    feats = torch.from_numpy(rng.standard_normal((n, cin)).astype(np.float32)).to(dev).requires_grad_(True)
    res = torch.from_numpy(rng.standard_normal((n, cout)).astype(np.float32)).to(dev).requires_grad_(True) if residual else None
    return conv, norm, feats, res, cfg


@pytest.mark.parametrize("route,cin,cout,K,relu,residual", [("tile", 32, 32, 27, True, False),
                                                            ("ws3", 64, 64, 27, True, True),
                                                            ("ws", 128, 64, 27, False, False),
                                                            ("dense", 64, 128, 1, True, False)])
def test_conv_bias_ahead_of_batchnorm(dev, route, cin, cout, K, relu, residual, monkeypatch):
    """ConvBnActFunction with a conv bias ahead of the BatchNorm: the bias enters the batch statistics (running_mean) and
    gets a gradient (col_sums(dz), analytically 0) -- and the unit's other outputs match fp64 as in the networks."""
    proxy = _LibProxy(ops._lib_())
    monkeypatch.setattr(ops, "_lib_", lambda: proxy)
    nodes = []
    fn = _recording_function(nodes, proxy)
    conv, norm, feats, res, cfg = _unit_case(dev, cin, cout, K, relu, residual, route, seed=cin + cout + K)
    y = fn.apply(feats, conv.kernel, norm.bn.weight, norm.bn.bias, conv.bias, res, cfg)
    g = torch.Generator().manual_seed(2)
    (y * torch.randn(tuple(y.shape), generator=g).to(dev)).sum().backward()
    assert conv.bias.grad is not None
    rec = nodes[0]
    assert rec["fwd"] == {route} and rec["bwd"] == {route}, (route, rec["fwd"], rec["bwd"])
    # the fp64 rebuild adds the bias before the batch statistics: running_mean (momentum * bias ~ 0.2 off without it) and
    # bias.grad are checked there with the node's other outputs
    worst = _check_nodes(nodes, f"bias-{route}")
    assert "dbias/|dz|" in worst and "running_mean" in worst
