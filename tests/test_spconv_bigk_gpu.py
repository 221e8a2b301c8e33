"""The tile family's kernel for 32 < K <= 125 with real channel counts (spconv_bigk.hip: the symmetric recipe's 5^3 generator
conv1, 128 -> 32, and its input gradient, 32 -> 128) through ops.spconv against a float64 gather-and-sum, row by row, at the
bars tests/test_spconv_gpu.py holds the tile family to: rel_l2 < 2e-6 over the output, every row within 5e-6 of its own
magnitude sum_k |x_row| |W_k|, and the same bits on a second run."""
import numpy as np
import pytest
import torch

from apr_amd import ops

pytestmark = pytest.mark.gpu

EDGE_OFFSETS = (0, 31, 32, 63, 64, 95, 96, 124)      # mask-word and ballot-round edges


def oracle_conv(x, nbr, W, scale=None, shift=None, residual=None, relu=False):
    out = torch.zeros(nbr.shape[0], W.shape[2], dtype=torch.float64)
    xd, Wd = x.double(), W.double()
    for o in range(nbr.shape[1]):
        j = np.nonzero(nbr[:, o] >= 0)[0]
        if len(j):
            out.index_add_(0, torch.from_numpy(j), xd[torch.from_numpy(nbr[j, o].astype(np.int64))] @ Wd[o])
    if scale is not None:
        out = out * scale.double()
    if shift is not None:
        out = out + shift.double()
    if residual is not None:
        out = out + residual.double()
    return torch.relu(out) if relu else out


def random_map(rng, n_in, n_out, K, density):
    nbr = rng.integers(0, n_in, size=(n_out, K)).astype(np.int32)
    nbr[rng.random((n_out, K)) > density] = -1
    return nbr


def operands(rng, n_in, K, cin, cout):
    x = torch.from_numpy(rng.standard_normal((n_in, cin)).astype(np.float32))
    W = torch.from_numpy((rng.standard_normal((K, cin, cout)) / np.sqrt(cin * 8)).astype(np.float32))
    return x, W


def check_bare(dev, x, nbr, W):
    """The bare contraction through ops.spconv at the three bars; -> the device result."""
    K, cin, cout = W.shape
    wp = ops.pack_weights(W.to(dev))
    nbr_d = torch.from_numpy(nbr).to(dev)
    got = ops.spconv(x.to(dev), nbr_d, K, cin, cout, wp)
    again = ops.spconv(x.to(dev), nbr_d, K, cin, cout, wp)
    assert torch.equal(got, again)
    ref = oracle_conv(x, nbr, W)
    mag = oracle_conv(x.abs(), nbr, W.abs()).norm(dim=1)
    err = (got.cpu().double() - ref).norm(dim=1)
    assert bool((err[mag == 0] == 0).all())      # rows without a neighbour are exact zeros
    assert float((err / mag.clamp_min(1e-300)).max()) < 5e-6
    if float(ref.norm()) > 0:
        assert float(err.norm() / ref.norm()) < 2e-6
    return got


def test_predicate_covers_the_shapes_tested_here():
    assert all(ops.bigk_supported(K, cin, cout) for K, cin, cout in
               [(125, 32, 32), (125, 128, 32), (125, 32, 128), (125, 64, 64), (33, 32, 32), (64, 64, 32)])
    assert not ops.bigk_supported(125, 48, 32)


@pytest.mark.parametrize("n_out", [1, 31, 33, 65, 200])
@pytest.mark.parametrize("cin,cout", [(32, 32), (128, 32), (32, 128), (64, 64)])
def test_random_tables(dev, n_out, cin, cout):
    """Ragged last tile, one and several tiles, one and several column tiles and cin chunks; thin (LiDAR-like) occupancy."""
    rng = np.random.default_rng(n_out * 1000 + cin + cout)
    n_in = max(n_out, 40)
    x, W = operands(rng, n_in, 125, cin, cout)
    check_bare(dev, x, random_map(rng, n_in, n_out, 125, 0.06), W)


@pytest.fixture(scope="module")
def abutting_map(dev):
    """The (1, 1, 5) kernel map of two batch items over the SAME voxel block: rows of one item have every spatial neighbour
    of the other item right next to them in coordinate space, apart from the batch index."""
    from apr_amd.MinkowskiEngine.core import CoordinateManager
    rng = np.random.default_rng(5)
    items = []
    for b in range(2):
        cells = np.argwhere(rng.random((7, 7, 5)) < 0.45).astype(np.int32)
        items.append(np.concatenate([np.full((len(cells), 1), b, np.int32), cells], axis=1))
    C = np.concatenate(items)
    cm = CoordinateManager(torch.from_numpy(C).to(dev))
    nbr = cm.kernel_map(1, 1, 5).cpu().numpy()
    coords = cm.get_map(1).coords.cpu().numpy()
    return coords, nbr


def test_real_5x5x5_map_of_two_abutting_batch_items(dev, abutting_map):
    coords, nbr = abutting_map
    n = len(coords)
    assert nbr.shape == (n, 125) and n > 128
    j, o = np.nonzero(nbr >= 0)
    assert np.array_equal(coords[j, 0], coords[nbr[j, o], 0])      # the table itself never crosses the batch index
    assert (nbr >= 0).sum(axis=1).max() > 40
    rng = np.random.default_rng(11)
    x, W = operands(rng, n, 125, 128, 32)
    got = check_bare(dev, x, nbr, W).cpu()
    # nothing leaks across the batch index: zeroing the other item's input rows leaves an item's output rows as they were
    for b in (0, 1):
        xb = x.clone()
        xb[coords[:, 0] != b] = 0
        only = ops.spconv(xb.to(dev), torch.from_numpy(nbr).to(dev), 125, 128, 32, ops.pack_weights(W.to(dev))).cpu()
        assert torch.equal(only[coords[:, 0] == b], got[coords[:, 0] == b])


def test_input_gradient_form(dev, abutting_map):
    """The input gradient of the 128 -> 32 layer is the same operator with 32 -> 128 channels over the same (symmetric)
    table and the flip-transposed weights: it equals the float64 transpose of the forward, dX[i] = sum over the pairs
    (j, o) with nbr[j, o] = i of dY[j] @ W[o]^T."""
    coords, nbr = abutting_map
    n = len(coords)
    rng = np.random.default_rng(13)
    _, W = operands(rng, n, 125, 128, 32)
    dy = torch.from_numpy(rng.standard_normal((n, 32)).astype(np.float32))
    wt = ops.weights_flip_transpose(W.to(dev), True)
    assert tuple(wt.shape) == (125, 32, 128)
    nbr_d = torch.from_numpy(nbr).to(dev)
    got = ops.spconv(dy.to(dev), nbr_d, 125, 32, 128, ops.pack_weights(wt))
    assert torch.equal(got, ops.spconv(dy.to(dev), nbr_d, 125, 32, 128, ops.pack_weights(wt)))
    ref = torch.zeros(n, 128, dtype=torch.float64)
    mag = torch.zeros(n, 128, dtype=torch.float64)
    for o in range(125):
        j = np.nonzero(nbr[:, o] >= 0)[0]
        if len(j):
            i = torch.from_numpy(nbr[j, o].astype(np.int64))
            ref.index_add_(0, i, dy[j].double() @ W[o].double().T)
            mag.index_add_(0, i, dy[j].double().abs() @ W[o].double().abs().T)
    err = (got.cpu().double() - ref).norm(dim=1)
    assert float((err / mag.norm(dim=1).clamp_min(1e-300)).max()) < 5e-6
    assert float(err.norm() / ref.norm()) < 2e-6


def hand_table(n_in, with_full_row):
    """Rows: no neighbour at all; (optionally) all 125 present, the centre of a filled 5 x 5 x 5 block; one row per edge
    offset with that offset alone; then the same single-offset rows again 70 rows further on, in the second tile."""
    rows = [np.full(125, -1, np.int32)]
    if with_full_row:
        rows.append(np.arange(125, dtype=np.int32))
    for rep in range(2):
        for i, o in enumerate(EDGE_OFFSETS):
            r = np.full(125, -1, np.int32)
            r[o] = (7 * i + 3 + rep) % n_in
            rows.append(r)
        if rep == 0:
            rows += [np.full(125, -1, np.int32)] * (70 - len(rows))
    return np.stack(rows)


@pytest.mark.parametrize("cin,cout", [(128, 32), (32, 128)])
def test_hand_made_rows(dev, cin, cout):
    rng = np.random.default_rng(cin)
    x, W = operands(rng, 130, 125, cin, cout)
    nbr = hand_table(130, True)
    assert (nbr[0] < 0).all() and (nbr[1] >= 0).all() and (nbr[2:10] >= 0).sum() == 8
    got = check_bare(dev, x, nbr, W).cpu().double()
    # a row with one neighbour is one matrix-vector product
    for i, o in enumerate(EDGE_OFFSETS):
        ref = x[nbr[2 + i, o]].double() @ W[o].double()
        assert float((got[2 + i] - ref).norm() / ref.norm()) < 2e-6


def test_an_offset_no_row_uses(dev):
    rng = np.random.default_rng(3)
    x, W = operands(rng, 150, 125, 64, 64)
    nbr = np.concatenate([hand_table(150, False), random_map(rng, 150, 77, 125, 0.1)])
    nbr[:, 50] = -1
    nbr[:, 64] = np.where(np.arange(len(nbr)) % 5 == 0, nbr[:, 64], -1)
    W[50] = float("nan")      # an unused offset's weights are never multiplied in
    check_bare(dev, x, nbr, W)


@pytest.mark.parametrize("K", [33, 64])
def test_smaller_kernels(dev, K):
    rng = np.random.default_rng(K)
    x, W = operands(rng, 300, K, 32, 32)
    check_bare(dev, x, random_map(rng, 300, 131, K, 0.2), W)
    x, W = operands(rng, 300, K, 64, 64)
    check_bare(dev, x, random_map(rng, 300, 64, K, 1.0), W)      # every pair list full: 64 pairs, four groups of 16


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("cin,cout", [(128, 32), (32, 128)])
def test_slices_and_epilogue(dev, cin, cout, epilogue):
    """Input, residual and output as column slices of wider buffers; scale / shift / residual / ReLU all on or all off."""
    rng = np.random.default_rng(cin + int(epilogue))
    n_in, n_out = 180, 133
    xw = torch.from_numpy(rng.standard_normal((n_in, cin + 32)).astype(np.float32))
    _, W = operands(rng, n_in, 125, cin, cout)
    nbr = random_map(rng, n_in, n_out, 125, 0.08)
    scale = torch.from_numpy(rng.uniform(0.5, 1.5, cout).astype(np.float32)) if epilogue else None
    shift = torch.from_numpy(rng.standard_normal(cout).astype(np.float32)) if epilogue else None
    resw = torch.from_numpy(rng.standard_normal((n_out, cout + 64)).astype(np.float32)) if epilogue else None
    outw = torch.zeros(n_out, cout + 96, device=dev)

    def run(out):
        return ops.spconv(xw.to(dev)[:, 32:], torch.from_numpy(nbr).to(dev), 125, cin, cout, ops.pack_weights(W.to(dev)),
                          scale=None if scale is None else scale.to(dev), shift=None if shift is None else shift.to(dev),
                          residual=None if resw is None else resw.to(dev)[:, :cout], relu=epilogue, out=out)
    got = run(outw[:, 32:32 + cout])
    ref = oracle_conv(xw[:, 32:], nbr, W, scale, shift, None if resw is None else resw[:, :cout], relu=epilogue)
    assert float((got.cpu().double() - ref).norm() / ref.norm()) < 2e-6
    assert float(outw[:, :32].abs().max()) == 0.0 and float(outw[:, 32 + cout:].abs().max()) == 0.0
    assert torch.equal(run(None), got)


def test_shape_outside_the_predicate_takes_the_generic_kernel(dev):
    rng = np.random.default_rng(48)
    x, W = operands(rng, 90, 125, 48, 32)
    check_bare(dev, x, random_map(rng, 90, 70, 125, 0.1), W)
