"""The 'cross_cat' layer of the overlap-attention module (apr_amd/predator/models/gcn.py) as a torch module, without a GPU:
it constructs, carries the reference's parameter names and shapes (tests/golden/predator_cross_cat_ref.npz, written by the
reference's own gcn.py), loads the reference's state_dict strictly, shares proj[0] with distribute, draws the reference's
weights from the same seed, and refuses what the reference cannot run."""
import os

import numpy as np
import pytest
import torch

from apr_amd.predator.models import gcn

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predator_cross_cat_ref.npz")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def _fixture_state(g):
    return {k[len("a_sd/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("a_sd/")}


def test_constructs_with_the_three_layer_kinds():
    m = gcn.GCN(4, 64, 10, ['self', 'cross_cat', 'self'])
    assert isinstance(m.layers[0], gcn.SelfAttention) and isinstance(m.layers[2], gcn.SelfAttention)
    cat = m.layers[1]
    assert isinstance(cat, gcn.AttentionalPropagationCat) and isinstance(cat.attn, gcn.MultiHeadedAttentionCat)
    assert cat.attn.merge.weight.shape == (64 + 28, 64 + 28, 1) and cat.mlp[0].weight.shape == (128, 128 + 28, 1)
    assert cat.mlp[3].weight.shape == (64, 128, 1) and not cat.mlp[3].bias.any()
    assert m._desc() is None, "a module with a cross_cat layer must never reach the one-call plan"


def test_keys_and_shapes_are_the_references_and_its_state_loads_strictly(g):
    sd = _fixture_state(g)
    m = gcn.GCN(4, 64, 10, ['cross_cat'])
    mine = m.state_dict()
    assert list(mine.keys()) == list(sd.keys())
    assert all(tuple(mine[k].shape) == tuple(sd[k].shape) for k in sd)
    assert "layers.0.attn.distribute.weight" in mine and "layers.0.attn.proj.0.weight" in mine
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    # named_parameters: the fixture holds one gradient per parameter, the shared tensor once
    names = [n for n, _ in m.named_parameters()]
    assert len(names) == len(set(names)) == 12 and set(names) == {k[len("a_g/"):] for k in g if k.startswith("a_g/")}


def test_proj0_is_distribute():
    attn = gcn.GCN(4, 64, 10, ['cross_cat']).layers[0].attn
    assert attn.proj[0] is attn.distribute
    assert attn.proj[1] is not attn.distribute and attn.proj[2] is not attn.proj[1]
    params = list(attn.parameters())
    assert sum(p is attn.distribute.weight for p in params) == 1 and len(params) == 8
    assert torch.equal(attn.proj[1].weight, attn.distribute.weight), "the copies start from distribute's values"


def test_same_seed_gives_the_references_weights(g):
    torch.manual_seed(int(g["b_seed"]))
    sd = gcn.GCN(4, 256, 10, ['self', 'cross_cat', 'self']).state_dict()
    assert list(sd.keys()) == [str(k) for k in g["b_keys"]]
    sums = np.array([float(v.double().sum()) for v in sd.values()])
    sumsq = np.array([float((v.double() ** 2).sum()) for v in sd.values()])
    assert np.allclose(sums, g["b_sum"], rtol=1e-12, atol=1e-12) and np.allclose(sumsq, g["b_sumsq"], rtol=1e-12, atol=0)


def test_forward_with_two_heads_raises_value_error():
    m = gcn.GCN(2, 64, 10, ['cross_cat'])           # constructs, as the reference does
    x0, x1, c0, c1 = torch.zeros(5, 64), torch.zeros(4, 64), torch.zeros(5, 3), torch.zeros(4, 3)
    with pytest.raises(ValueError):
        m.layers[0](x0, x1, c0, c1)
    with pytest.raises(ValueError):
        m._forward_layers(c0, c1, x0, x1)


def test_unknown_layer_name_still_raises():
    with pytest.raises(NotImplementedError):
        gcn.GCN(4, 64, 10, ['self', 'cross_dog'])
