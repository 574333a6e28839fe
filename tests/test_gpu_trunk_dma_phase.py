"""GPU: the rank-tile trunk kernel k_trunk_x16<128, 4, *, 0, 1, 0, 0, 0> with the request schedule of
CRL_TRUNK_DMA_PHASE (csrc/tower_x16.hpp): the waves of the upper rank half ask for a tap's weight tiles a sub-step
after the sync that frees their ring slots, their SIMD partners directly behind it.

What could go wrong is a tile that is read before it has landed or overwritten while it is read, which shows as
wrong or unstable values in some workgroups; the arithmetic is untouched, so the bar is bits.  516 boards is the
smallest batch the dispatch gives to the NB = 4 kernel: 129 workgroups, a partial round.  128 filters, n_blocks 0 (the stem alone: the last tap's schedule only), 1 and 3, both plane
formats, seeded random planes and weights.  `out` and `head_out` must equal, bit for bit,

  * those of the NB = 2 kernel on the same boards (batches of at most 512 boards go to it; it has no rank halves and
    this schedule does not exist in it),
  * a second launch of the NB = 4 kernel itself.
"""
import pytest
import torch

from tests import test_gpu_trunk_arith as ta

pytestmark = pytest.mark.gpu

FILTERS = 128
BOARDS = 516
NB4 = (128, 4, 1, 0, 0)
NB2 = (128, 2, 1, 0, 0)
_CACHE = {}


def _setup():
    if not _CACHE:
        planes16 = ta._random_planes(BOARDS, seed=1111)
        _CACHE["planes"] = {0: planes16, 1: ta._bits_from_planes(planes16)}
        _CACHE["model"] = ta._model(ta._weights(FILTERS), "f16")
    return _CACHE["model"], _CACHE["planes"]


@pytest.mark.parametrize("bits", [0, 1], ids=["fp16_planes", "bitboards"])
@pytest.mark.parametrize("n_blocks", [0, 1, 3])
def test_nb4_equals_nb2_and_itself_bit_for_bit(n_blocks, bits):
    L = ta._lib()
    model, both = _setup()
    planes = both[bits]
    flags = L.TRUNK_BITPLANES if bits else 0
    assert ta._kernel_name(FILTERS, BOARDS, flags) == ta._x16_name(*NB4, bits=bits)
    x4, h4 = ta._run(model, "f16", planes, n_blocks)
    x4b, h4b = ta._run(model, "f16", planes, n_blocks)
    cuts = (0, 256, BOARDS)                    # every launch takes a multiple of four boards
    for a, b in zip(cuts, cuts[1:]):
        assert ta._kernel_name(FILTERS, b - a, flags) == ta._x16_name(*NB2, bits=bits)
    xs, hs = zip(*(ta._run(model, "f16", planes[a:b].contiguous(), n_blocks) for a, b in zip(cuts, cuts[1:])))
    x2, h2 = torch.cat(xs), torch.cat(hs)
    assert x2.shape == x4.shape and h2.shape == h4.shape
    assert torch.equal(x4, x4b) and torch.equal(h4, h4b), "two launches of the NB = 4 kernel differ"
    bad = (x4 != x2).flatten(1).any(dim=1) | (h4 != h2).any(dim=1)
    assert not bad.any(), ("boards on which NB = 4 differs from NB = 2", bad.nonzero().flatten().tolist()[:16])
    assert not torch.equal(x4[0], x4[1])
