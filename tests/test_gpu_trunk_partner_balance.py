"""GPU: the partner balance of the rank-tile trunk kernel, k_trunk_x16<128, 4, *, 1, 1, 0, 0, 0> (csrc/tower_x16.hpp,
ALT = 1; reached through CRL_TRUNK_BALANCE of crl_trunk_forward_x).

Only WHO requests the weight tiles changes against ALT = 0 -- the lower rank half of every SIMD pair for both waves --
so every output must keep its bits.  What can go wrong is the ring: a piece requested for the partner wave that lands
in the wrong kilobyte of a slot, is requested twice or not at all, or is read before the barrier has published it.
516 boards are 129 workgroups (the last one sits in a partly idle round of the chip); n_blocks 0, 1 and 3 give towers
of 1, 3 and 7 convolutions (a launch's last two syncs request nothing); both plane formats.  Asked for, byte for byte,
trunk and heads:

  * the production ALT = 0 kernel (the same call without the flag),
  * the NB = 2 kernel (the batch in launches of at most 512 boards, which the small-batch rule gives to it),
  * a second launch of itself.

The ALT = 0 kernel is held to the float64 reference by tests/test_gpu_trunk_arith.py and tests/test_gpu_trunk_rank_tiles.py.
"""
import pytest
import torch

from oracle import tower_oracle
from tests import test_gpu_trunk_arith as ta

pytestmark = pytest.mark.gpu

DEV = ta.DEV
FILTERS = 128
BOARDS = 516
BLOCKS = 3
_CACHE = {}


def _name(nb, bits, alt):
    return "k_trunk_x16<%d, %d, %d, %d, 1, 0, 0, 0>" % (FILTERS, nb, bits, alt)


def _setup():
    if not _CACHE:
        w = tower_oracle.init_weights(BLOCKS, FILTERS, seed=23, randomize_bn=True)
        _CACHE["model"] = ta._model(w, "f16")
        planes16 = ta._random_planes(BOARDS, seed=91)
        _CACHE["planes"] = {0: planes16, 1: ta._bits_from_planes(planes16)}
    return _CACHE["model"], _CACHE["planes"]


def _run(model, planes, n_blocks, balance):
    L = ta._lib()
    n = planes.shape[0]
    flags = (L.TRUNK_BITPLANES if planes.dtype == torch.int64 else 0) | (L.TRUNK_BALANCE if balance else 0)
    out = torch.full((n, 8, 8, FILTERS), float("nan"), dtype=torch.float32, device=DEV)
    heads = torch.full((n, 192), float("nan"), dtype=torch.float32, device=DEV)
    L.trunk_forward_x(FILTERS, flags, planes, model._wtiles, model._wbias, out, n, n_blocks, model._head_w, model._head_b,
                      heads, None, 0)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(heads).all()
    return out, heads


def test_the_flag_names_the_balanced_kernel_for_the_rank_tile_cell_only():
    L = ta._lib()
    for bits in (0, 1):
        plane_flag = L.TRUNK_BITPLANES if bits else 0
        assert L.trunk_kernel_name(FILTERS, BOARDS, plane_flag | L.TRUNK_BALANCE) == _name(4, bits, 1)
        assert L.trunk_kernel_name(FILTERS, BOARDS, plane_flag) == _name(4, bits, 0)
        assert L.trunk_kernel_name(FILTERS, 512, plane_flag | L.TRUNK_BALANCE) == _name(2, bits, 0)      # NB = 2: no rank tiles
        for filters, n, flags in ((64, BOARDS, plane_flag), (256, BOARDS, plane_flag), (FILTERS, BOARDS, plane_flag | L.TRUNK_SPLIT)):
            assert L.trunk_kernel_name(filters, n, flags | L.TRUNK_BALANCE) == L.trunk_kernel_name(filters, n, flags)
    model, _ = _setup()
    assert model.filters == FILTERS and model.precision == "f16"


@pytest.mark.parametrize("bits", [0, 1], ids=["fp16_planes", "bitboards"])
@pytest.mark.parametrize("n_blocks", [0, 1, 3])
def test_balanced_kernel_keeps_the_bits_of_production_of_nb2_and_of_itself(n_blocks, bits):
    L = ta._lib()
    model, planes = _setup()
    p = planes[bits]
    plane_flag = L.TRUNK_BITPLANES if bits else 0
    assert L.trunk_kernel_name(FILTERS, BOARDS, plane_flag | L.TRUNK_BALANCE) == _name(4, bits, 1)
    x, h = _run(model, p, n_blocks, True)
    x_again, h_again = _run(model, p, n_blocks, True)
    x0, h0 = _run(model, p, n_blocks, False)
    cuts = (0, 512, BOARDS)                    # every launch takes a multiple of four boards
    for a, b in zip(cuts, cuts[1:]):
        assert L.trunk_kernel_name(FILTERS, b - a, plane_flag) == _name(2, bits, 0)
    parts = [_run(model, p[a:b].contiguous(), n_blocks, False) for a, b in zip(cuts, cuts[1:])]
    x2, h2 = torch.cat([q[0] for q in parts]), torch.cat([q[1] for q in parts])
    assert x2.shape == x.shape and h2.shape == h.shape
    assert torch.equal(x, x_again) and torch.equal(h, h_again), "two launches of the balanced kernel differ"
    assert torch.equal(x, x0) and torch.equal(h, h0), "the balanced kernel differs from the production ALT = 0 kernel"
    assert torch.equal(x, x2) and torch.equal(h, h2), "the balanced kernel differs from the NB = 2 kernel"
    # (none of this passes on a constant: the boards differ, and so do the two ends of the batch)
    assert not torch.equal(x[0], x[1]) and not torch.equal(x[0], x[BOARDS - 1])


def test_the_model_runs_the_balanced_kernel_and_keeps_its_outputs():
    """ChessModel's f16 forward passes the flag; what it returns is what the production kernel returns."""
    model, planes = _setup()
    trunk, heads = model._run_fused(planes[1], want_trunk=True)
    torch.cuda.synchronize()
    x0, h0 = _run(model, planes[1], model.blocks, False)
    assert torch.equal(trunk, x0) and torch.equal(heads, h0)
