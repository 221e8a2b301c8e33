"""collate_pair_fn / collate_debug_pair_fn (apr_amd/fcgf/lib/complement_data_loader.py) key by key and dtype by dtype
against what the reference's own collate text (FCGF_APR/lib/data_loaders.py:26-78, lib/complement_data_loader.py:1282-1333)
returned on the same CPU items (tests/golden/fcgf_losses_ref.npz, written by make_fcgf_losses_ref_golden.py); the
bookkeeping is also spelt out by hand.  No GPU."""
import numpy as np
import pytest
import torch

from apr_amd.fcgf.lib import complement_data_loader as CDL
from tests import fcgf_losses_oracle as O

_items = O.collate_items


@pytest.mark.parametrize("name", ["collate_pair_fn", "collate_debug_pair_fn"])
def test_bookkeeping(name):
    b = getattr(CDL, name)(_items())
    assert set(b) == {'pcd0', 'pcd1', 'sinput0_C', 'sinput0_F', 'sinput1_C', 'sinput1_F', 'correspondences', 'T_gt', 'len_batch'}
    assert b['correspondences'].dtype == torch.int32
    assert b['correspondences'].tolist() == [[0, 1], [6, 8], [2 + 18, 3 + 22], [16 + 18, 18 + 22]]     # the skipped item moved the head
    assert b['len_batch'] == [[7, 9], [17, 19]]
    assert b['T_gt'].dtype == torch.float32 and tuple(b['T_gt'].shape) == (8, 4)
    items = _items()
    for tag, col, lens in (("0", 0, (7, 11, 17)), ("1", 1, (9, 13, 19))):
        C, F = b[f'sinput{tag}_C'], b[f'sinput{tag}_F']
        assert C.dtype == torch.int32 and tuple(C.shape) == (sum(lens), 4) and F.dtype == torch.float32
        assert C[:, 0].tolist() == [k for k, n in enumerate(lens) for _ in range(n)]
        assert torch.equal(C[:, 1:], torch.cat([it[2 + col] for it in items]))
        if name == "collate_pair_fn":       # the kept items only, concatenated
            assert b[f'pcd{tag}'].dtype == torch.float32 and torch.equal(b[f'pcd{tag}'], torch.cat([items[0][col], items[2][col]]))
        else:
            assert isinstance(b[f'pcd{tag}'], tuple) and [len(x) for x in b[f'pcd{tag}']] == list(lens)


@pytest.mark.parametrize("name", ["collate_pair_fn", "collate_debug_pair_fn"])
def test_equals_the_reference_text(name):
    Z = O.load_fixture()
    got = O.flatten_collated(getattr(CDL, name)(_items()), name)
    want = {k: Z[k] for k in Z.files if k.startswith(name + "_")}
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
