"""CPU: the NPR MLP mirror has the reference's module / parameter layout (FCGF_APR/model/mlp.py)."""
import hashlib
import json
import os

import torch

from apr_amd.fcgf.lib import apg

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_generative_mlp_state_dict_equals_reference():
    """Same keys in the same order, shapes, dtypes and bits of every tensor as the reference's modules built after the same
    seed (tests/golden/fcgf_mlp_ref.json, written by make_reference_modules_golden.py from the reference's mlp.py)."""
    with open(os.path.join(GOLD, "fcgf_mlp_ref.json")) as f:
        ref = json.load(f)
    for name in ("GenerativeMLP", "GenerativeMLP_98", "GenerativeMLP_54"):
        torch.manual_seed(0)
        sb = getattr(apg, name)(in_channel=32, out_points=4).state_dict()
        assert [k for k, *_ in ref[name]] == list(sb.keys()), name
        for k, shape, dtype, sha in ref[name]:
            v = sb[k]
            assert list(v.shape) == shape and str(v.dtype) == dtype, (name, k)
            assert hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest() == sha, (name, k)


def test_layout_without_reference():
    m = apg.GenerativeMLP_98(in_channel=128, out_points=4)
    sd = m.state_dict()
    assert sd["mlp.0.weight"].shape == (512, 128) and sd["mlp.3.weight"].shape == (256, 512)
    assert sd["mlp.6.weight"].shape == (12, 256) and "mlp.2.running_var" in sd
