"""Host-side halves of the symmetric recipe (FCGF_APR/scripts/train_apr_nuscenes.sh; no GPU): the predicate of the tile family's
big-kernel conv, the routing it must not touch, the constructors of the training / validation steps, and the oracle's sparse
generator on the oracle encoder's output tensor."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from apr_amd import _lib, ops
from apr_amd.fcgf.lib.complement_trainer import GenerativePairTrainStep
from apr_amd.fcgf.lib.validation import GenerativePairValidStep, SymmetricPairValidStep
from oracle import me_oracle as OME
from oracle import resunet_oracle as OR
from tests.helpers import voxelized_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bigk_predicate(lib):
    yes = [(125, 128, 32), (125, 32, 128), (125, 64, 64), (33, 32, 32), (64, 32, 32)]
    no = [(27, 64, 64), (32, 32, 32), (126, 32, 32), (125, 1, 32), (125, 48, 32), (125, 32, 12)]
    assert [lib.apr_spconv_bigk_supported(*s) for s in yes] == [1] * len(yes)
    assert [lib.apr_spconv_bigk_supported(*s) for s in no] == [0] * len(no)
    assert all(ops.bigk_supported(*s) for s in yes) and not any(ops.bigk_supported(*s) for s in no)


def test_route_of_a_5x5x5_layer_is_still_the_tile_family(lib):
    """The new kernel is a finer choice INSIDE apr_spconv_fwd: no route id of its own, whatever the caller hands over."""
    for cin, cout in ((128, 32), (32, 128)):
        for extra in ({}, {"w_bf3": 0x4000}, {"plist": 0x5000, "counters": 0x6000, "w_bf3": 0x4000},
                      {"os_pairs": 0x7000, "os_rows": 48}):
            d = _lib.SpconvDesc()
            d.inp, d.ldi, d.nbr, d.n_out = 0x1000, cin, 0x2000, 1000
            d.K, d.cin, d.cout, d.out, d.ldo = 125, cin, cout, 0x3000, cout
            for k, v in extra.items():
                setattr(d, k, v)
            assert lib.apr_spconv_route(C.byref(d)) == _lib.ROUTE_TILE, (cin, cout, extra)
    header = open(os.path.join(ROOT, "include", "apr_hip.h")).read()
    assert re.findall(r"^  APR_ROUTE_([A-Z0-9_]+)", header, flags=re.M) == ["TILE", "WS", "WS_BF3", "WS3", "OS", "DENSE_ROWS",
                                                                           "DENSE_GEMM"]


def test_steps_construct():
    st = GenerativePairTrainStep(None, None, None, symmetric=True)
    assert st.symmetric is True
    assert GenerativePairTrainStep(None, None, None).symmetric is False
    v = SymmetricPairValidStep(None, None, regularization_type='RepelL1', strict_reference=False)
    assert isinstance(v, GenerativePairValidStep) and v.symmetric is True and v.strict_reference is False
    with pytest.raises(NotImplementedError, match="out of scope"):
        GenerativePairValidStep(None, None, symmetric=True)


def test_simplenet_families_stay_unmirrored():
    from apr_amd.fcgf.model import load_model
    for name in ("SimpleNet", "SimpleNetBN2C"):      # unknown names: None and a log line, as the reference's registry
        assert load_model(name) is None
    assert load_model("ResUNetFatBN") is not None


def test_oracle_generator_on_the_oracle_encoders_tensor():
    """lib/complement_trainer.py:52-60, :414: ResUNetFatBN(128, ratio * 3, conv1_kernel_size=5) takes the encoder's output
    SparseTensor (same coordinates, 128 channels) and, with normalize_feature, returns unit 12-vectors; a loss on them
    reaches the encoder's parameters through the generator's conv1."""
    torch.manual_seed(0)
    _, c, _ = voxelized_frame(3, n_beams=8, n_azimuth=200)
    coords = OME.batched_coordinates([c])
    enc = OR.ResUNetFatBN(1, 128, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).double().train()
    gen = OR.ResUNetFatBN(128, 12, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).double().train()
    assert tuple(gen.conv1.kernel.shape) == (125, 128, 32)
    x = OME.SparseTensor(torch.ones(len(coords), 1, dtype=torch.float64), coordinates=coords)
    y = enc(x)
    g = gen(y)
    assert tuple(g.F.shape) == (len(coords), 12) and np.array_equal(np.asarray(g.C), np.asarray(y.C))
    assert torch.allclose(g.F.norm(dim=1), torch.ones(len(coords), dtype=torch.float64), atol=1e-12)
    (g.F * torch.linspace(-1, 1, 12, dtype=torch.float64)).sum().backward()
    assert float(enc.conv1.kernel.grad.abs().max()) > 0 and float(gen.conv1.kernel.grad.abs().max()) > 0
