"""GPU: the indexed split-precision trunk (crl_trunk_forward_indexed, the second evaluation of the hybrid mode's close
calls) against the batch split-precision kernels AT DEPTH, bit for bit.

The batch kernels are held to the float64 reference by tests/test_gpu_trunk_arith.py; the indexed launch claims their
bits on the listed boards and claims to leave every other row alone, so no tolerance enters here.  The towers are walked
with n_blocks = k for k = 1 .. 3: from k = 2 on the 256-filter launches run the mid-tower second convolution
(k_layer_conv<8, 2, 2, 1> one board per workgroup, k_layer_conv<8, 2, 3, 2> two boards per workgroup: the skip re-read
from the activation image and rewritten in place, the A / B image ping-pong under the list) and the fused 64 / 128-filter
kernel (k_trunk_x16<F, NB, 1, 0, PAIR, 0, 1, 1>) hands one block over to the next; the first k that differs names the layer.

List lengths sit on both sides of the 256-board boundary between the two 256-filter windows (IDX 2: at most 256 listed
boards, one per workgroup; IDX 3: more, two per workgroup, an odd list padded with its last entry).

Negative controls: one Whi element of a MID-tower convolution scaled by 1.01 in the image only the indexed call sees
changes every listed row (so the indexed launch does run that convolution on those boards) and no other; and the f16 rows
the indexed launch overwrites differ from the split kernel's on every listed board (so "became the split kernel's bits"
says something).
"""
import numpy as np
import pytest
import torch

from oracle import tower_oracle, trunk_reference as tr
from tests.test_gpu_trunk_arith import (BLOCKS, DEV, _bits_from_planes, _image_offset, _kernel_name, _lib, _model,
                                        _random_planes, _run, _SmallBatch, _weights)

pytestmark = pytest.mark.gpu

SENTINEL = (-5, 2 ** 31 - 3, 77)         # words [1 .. 3] of the list header: not the trunk's to touch
# (filters, n_boards, small-batch switch) -> boards per workgroup of the fused indexed kernel (256 filters: both windows)
CELLS = {(64, 8, 1): 2, (64, 516, 1): 4, (128, 516, 1): 2, (256, 516, 1): None}
_CACHE = {}


def _lengths(n):
    return (1, 3, n, 0) if n == 8 else (1, 3, 255, 256, 257, n, 0)


def _window(filters, length):
    if filters != 256 or length == 0:
        return "-"
    return "IDX 2 (one board per workgroup)" if length <= 256 else "IDX 3 (two boards per workgroup)"


def _pick(n, length, seed):
    """``length`` distinct boards of n in shuffled order; board 0 is left out of every list that leaves one out (the
    unused tail of the list holds zeros: a launch that read past the list's end would rewrite row 0)."""
    rng = np.random.default_rng(seed)
    if length == n:
        return [int(b) for b in rng.permutation(n)]
    return [int(b) + 1 for b in rng.permutation(n - 1)[:length]]


def _hybrid_model(w):
    key = id(w)
    if key not in _CACHE:
        _CACHE[key] = (w, _model(w, "hybrid"))              # both weight images packed
    return _CACHE[key][1]


def _inputs(n, seed):
    planes16 = _random_planes(n, seed=seed)
    bits = _bits_from_planes(planes16)
    assert torch.unique(bits, dim=0).shape[0] == n           # no two boards are equal
    return bits


def _indexed(model, bits, n_blocks, base, pick, image=None):
    """crl_trunk_forward_indexed over ``pick`` onto a clone of ``base``: (head activations, the list afterwards)."""
    L = _lib()
    n = bits.shape[0]
    assert len(set(pick)) == len(pick) and all(0 <= b < n for b in pick)
    lst = torch.zeros(L.LIST_HEADER + n, dtype=torch.int32, device=DEV)
    lst[0] = len(pick)
    lst[1:L.LIST_HEADER] = torch.tensor(SENTINEL, dtype=torch.int32)
    if pick:
        lst[L.LIST_HEADER:L.LIST_HEADER + len(pick)] = torch.tensor(pick, dtype=torch.int32)
    want = lst.clone()
    hp = base.clone()
    ws = model._trunk_workspace(n)
    L.trunk_forward_indexed(model.filters, bits, image if image is not None else model._wtiles3, model._wbias, n, n_blocks,
                            model._head_w, model._head_b, hp, lst, ws, ws.numel() if ws is not None else 0)
    torch.cuda.synchronize()
    assert torch.equal(lst, want), "the indexed trunk wrote into its list"
    return hp


def _mask(n, pick):
    m = torch.zeros(n, dtype=torch.bool, device=DEV)
    if pick:
        m[pick] = True
    return m


def _check_lists(model, bits, k, lengths, label):
    """Indexed against batch at n_blocks = k for every list length; returns the rows of the report."""
    n = bits.shape[0]
    _, h48 = _run(model, "f16x3", bits, k)
    _, h16 = _run(model, "f16", bits, k)
    rows_differ = (h16 != h48).any(dim=1)
    report = []
    for length in lengths:
        pick = _pick(n, length, seed=100 * k + length)
        mask = _mask(n, pick)
        # (else "became the split kernel's bits" would be vacuous)
        assert bool(rows_differ[mask].all()), (label, k, length, "f16 and f16x3 agree on a listed board")
        hp = _indexed(model, bits, k, h16, pick)
        bad_listed = int((hp[mask] != h48[mask]).any(dim=1).sum())
        bad_other = int((hp[~mask] != h16[~mask]).any(dim=1).sum())
        report.append((k, length, _window(model.filters, length), bad_listed, bad_other))
        assert bad_listed == 0, (label, "n_blocks", k, "listed", length, _window(model.filters, length),
                                 "%d listed rows are not the batch kernel's" % bad_listed)
        assert bad_other == 0, (label, "n_blocks", k, "listed", length, _window(model.filters, length),
                                "%d unlisted rows changed" % bad_other)
    return report


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("cell", sorted(CELLS), ids=lambda c: "%d-%d-small%d" % c)
def test_depth_chain_listed_rows_are_the_batch_kernels_bits(cell, k):
    filters, n, small = cell
    model = _hybrid_model(_weights(filters))
    bits = _inputs(n, seed=3)
    with _SmallBatch(small):
        if CELLS[cell] is not None:                          # the fused indexed kernel takes the batch kernel's geometry
            name = _kernel_name(filters, n, _lib().TRUNK_BITPLANES | _lib().TRUNK_SPLIT)
            assert name.startswith("k_trunk_x16<%d, %d," % (filters, CELLS[cell])), name
        report = _check_lists(model, bits, k, _lengths(n), "cell %s" % (cell,))
    for row in report:
        print("indexed %d filters, %d boards: n_blocks %d, %d listed, %s: %d / %d rows off" % ((filters, n) + row))


@pytest.mark.parametrize("filters,n,lengths", [(256, 8, (3, 8)), (128, 8, (3, 8)), (256, 260, (260,))],
                         ids=["256-8", "128-8", "256-260"])
def test_twenty_blocks_run_every_convolution_slot_through_the_indexed_launches(filters, n, lengths):
    """20 blocks = 41 convolutions (crl_tower::MAX_CONVS); 260 boards, all listed: a list beyond 256 (two boards per
    workgroup at 256 filters)."""
    key = ("w20", filters)
    if key not in _CACHE:
        _CACHE[key] = tower_oracle.init_weights(20, filters, seed=13, randomize_bn=True)
    model = _hybrid_model(_CACHE[key])
    bits = _inputs(n, seed=20)
    for row in _check_lists(model, bits, 20, lengths, "20 blocks %d filters, %d boards" % (filters, n)):
        print("indexed %d filters, %d boards: n_blocks %d, %d listed, %s: %d / %d rows off" % ((filters, n) + row))


@pytest.mark.parametrize("filters,length", [(256, 3), (256, 257), (128, 3), (128, 257)])
def test_negative_control_a_mid_tower_weight_changes_every_listed_row_and_no_other(filters, length):
    """Whi of block 1's second convolution (256 filters: the KIND 2 launch), one element x 1.01, in the image the indexed
    call alone is given: an indexed launch that skipped the mid-tower convolution, or ran it on other boards than the
    listed ones, would pass the bit comparisons above and fails here."""
    n = 516
    w = _weights(filters)
    P = tr.prepare(w, DEV)
    model = _hybrid_model(w)
    bits = _inputs(n, seed=3)
    x1, _ = _run(model, "f16x3", bits, 1)
    _, h48 = _run(model, "f16x3", bits, BLOCKS)
    _, h16 = _run(model, "f16", bits, BLOCKS)
    # the input channel of that convolution (conv1's output of block 1, from the kernel's own X_1) that is active on
    # EVERY board, to the output channel it weighs most, centre tap
    _, y = tr.block(P, 1, x1, "f16x3", "hilo" if filters == 256 else "fp32", mid=True)
    per_board = y.reshape(n, 64, filters).max(dim=1).values.min(dim=0).values
    i = int(per_board.argmax())
    assert per_board[i] > 0
    c = P.conv2[1]
    o = int(c.whi[4, i].abs().argmax())
    size = 9 * filters * filters * 2
    image = model._wtiles3.clone()
    seg = image[image.numel() - 3 * size:image.numel() - 2 * size]        # ... stem, b0c1, b0c2, b1c1, [b1c2], b2c1, b2c2
    j = _image_offset(filters, "f16x3", 4, i, o)
    assert seg[j].double() == c.whi[4, i, o] and seg[j] != 0             # (the documented image layout finds that weight)
    seg[j] = (seg[j].float() * 1.01).half()
    assert not torch.equal(image, model._wtiles3)
    pick = _pick(n, length, seed=7)
    mask = _mask(n, pick)
    sane = _indexed(model, bits, BLOCKS, h16, pick)
    assert torch.equal(sane[mask], h48[mask]) and torch.equal(sane[~mask], h16[~mask])
    hp = _indexed(model, bits, BLOCKS, h16, pick, image=image)
    same = int((hp[mask] == h48[mask]).all(dim=1).sum())
    print("control %d filters, %d listed (%s): %d of %d listed rows unchanged by the altered weight"
          % (filters, length, _window(filters, length), same, length))
    assert same == 0, (filters, length, same)
    assert torch.equal(hp[~mask], h16[~mask])
