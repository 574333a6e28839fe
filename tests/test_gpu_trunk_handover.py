"""GPU: the layer hand-over of k_trunk_x16 (csrc/tower_x16.hpp) computes what it computed before its epilogue
went from three shapes (stem / conv1 / conv2) to two (the stem as a conv2 on a -0 skip stream with a -inf floor).

What can go wrong in a hand-over: the stem gaining a ReLU or losing a zero's sign, conv1 touching the skip stream,
conv2 adding a stale one, the skip stream not surviving a second and a third block, a wave slot (board pair, rank
half, channel group) handing over another slot's registers.  So: 8 boards (two workgroups of the NB = 4 kernel),
n_blocks = 0 (stem only), 1 (each kind once), 2 and 3 (the skip stream carried on), both plane formats, seeded
planes and weights, and

  (a) trunk and heads of the NB = 4 kernel equal the NB = 2 kernel's bit for bit;
  (b) both lie within the bounds of tests/test_gpu_trunk_arith.py (CHAIN_BOUND["f16"], HEADS_BOUND) of the
      operand-exact float64 reference, layer-local;
  (c) sha256 of trunk and heads equal tests/golden/trunk_handover_digests.json, which this file's generator
      (python -m tests.test_gpu_trunk_handover OUT.json) recorded on an MI355X from the commit BEFORE the two-shape
      epilogue.  The digests also cover one 64-filter and one 256-filter kernel and the split-precision (f16x3)
      kernels of 64 and 128 filters at 4 boards: a zero whose sign changed, or one denormal flushed, changes them.
"""
import hashlib
import json
import os
import sys

import pytest
import torch

from oracle import tower_oracle, trunk_reference as tr
from tests import test_gpu_trunk_arith as ta

pytestmark = pytest.mark.gpu

DEV = ta.DEV
BLOCKS = 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trunk_handover_digests.json")
# label -> (filters, mode, boards, small-batch switch, the kernel (F, NB, PAIR, GROUP, SPLIT))
CASES = {
    "128 f16 nb4": (128, "f16", 8, 0, (128, 4, 1, 0, 0)),
    "128 f16 nb2": (128, "f16", 8, 1, (128, 2, 1, 0, 0)),
    "64 f16": (64, "f16", 4, 1, (64, 2, 0, 0, 0)),
    "256 f16": (256, "f16", 4, 1, (256, 1, 1, 0, 0)),
    "64 f16x3": (64, "f16x3", 4, 1, (64, 2, 0, 0, 1)),
    "128 f16x3": (128, "f16x3", 4, 1, (128, 2, 1, 0, 1)),
}
_CACHE = {}


def _weights(filters):
    key = ("w", filters)
    if key not in _CACHE:
        _CACHE[key] = tower_oracle.init_weights(BLOCKS, filters, seed=17, randomize_bn=True)
    return _CACHE[key]


def _outputs(label):
    """[(trunk, heads) for n_blocks = 0 .. BLOCKS] of one case, computed once; both plane formats give the same bits."""
    if label not in _CACHE:
        filters, mode, n, small, kern = CASES[label]
        L = ta._lib()
        model = ta._model(_weights(filters), mode)
        planes16 = ta._random_planes(8, seed=90)[:n].contiguous()      # (the 4-board cases: the first four of the 8)
        bits = ta._bits_from_planes(planes16)
        flags = L.TRUNK_SPLIT if mode == "f16x3" else 0
        rows = []
        with L.trunk_set_small_batch(small):
            assert ta._kernel_name(filters, n, flags | L.TRUNK_BITPLANES) == ta._x16_name(*kern, bits=1)
            assert ta._kernel_name(filters, n, flags) == ta._x16_name(*kern, bits=0)
            for k in range(BLOCKS + 1):
                x, h = ta._run(model, mode, bits, k)
                x16, h16 = ta._run(model, mode, planes16, k)
                assert torch.equal(x, x16) and torch.equal(h, h16), (label, k, "the two plane formats differ")
                rows.append((x, h))
        _CACHE[label] = (planes16, rows)
    return _CACHE[label]


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def digests():
    """{label: [{"out": sha256, "head_out": sha256} for n_blocks = 0 .. BLOCKS]}"""
    return {label: [{"out": _sha(x), "head_out": _sha(h)} for x, h in _outputs(label)[1]] for label in sorted(CASES)}


@pytest.mark.parametrize("n_blocks", range(BLOCKS + 1))
def test_nb4_equals_nb2_bit_for_bit(n_blocks):
    x4, h4 = _outputs("128 f16 nb4")[1][n_blocks]
    x2, h2 = _outputs("128 f16 nb2")[1][n_blocks]
    assert torch.equal(x4, x2), "trunk"
    assert torch.equal(h4, h2), "heads"
    assert bool((x4 < 0).any()) == (n_blocks == 0),"the stem is linear, a block's output is not negative"


@pytest.mark.parametrize("label", ["128 f16 nb4", "128 f16 nb2"])
def test_layer_local_chain_and_heads_within_the_float64_reference(label):
    planes16, rows = _outputs(label)
    P = tr.prepare(_weights(128), DEV)
    for k, (x, h) in enumerate(rows):
        ref = tr.stem(P, planes16, "f16") if k == 0 else tr.block(P, k - 1, rows[k - 1][0], "f16", "fp32")
        s = ta._stats(x, ref)
        he = ta._heads_error(P, x, h)
        print("%s n_blocks=%d: chain (max, p99.9) = %s, heads = %g" % (label, k, s, he))
        assert ta._within(s, "f16"), (label, k, s, ta.CHAIN_BOUND["f16"])
        assert he <= ta.HEADS_BOUND, (label, k, he)


@pytest.mark.parametrize("label", sorted(CASES))
def test_digests_equal_the_recorded_ones(label):
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = [{"out": _sha(x), "head_out": _sha(h)} for x, h in _outputs(label)[1]]
    for k, (g, e) in enumerate(zip(got, golden[label])):
        assert g == e, (label, "n_blocks=%d" % k)
    assert len(golden[label]) == BLOCKS + 1


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(digests(), f, indent=1, sort_keys=True)
        f.write("\n")
