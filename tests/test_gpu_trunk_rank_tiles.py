"""GPU: the rank tiles of the 128-filter, four-boards-per-workgroup f16 trunk kernel (csrc/tower_x16.hpp).

There a wave owns 2 boards x 4 ranks x 64 channels: an MFMA block is one rank of a PAIR of boards, the upper rank
half enumerates its ranks in reverse, and a block whose rank + dy leaves the board is skipped as a whole.  What can
go wrong is addressing: a lane reading its partner board's rows, a skipped block that is on the board, an off-board
row that is read, a wrong rank order in the upper half.  Every case runs the NB = 4 kernel (small-batch switch off)
at 8 and 12 boards -- 2 and 3 workgroups: every pair slot, both rank halves, both channel groups -- in both plane
formats, and asks for

  * the bits of the untouched NB = 2 kernel (the same call with the switch on), trunk and heads, at every depth;
  * the layer-local chain of tests/test_gpu_trunk_arith.py against oracle/trunk_reference.py within
    CHAIN_BOUND["f16"], and the heads within HEADS_BOUND.
"""
import numpy as np
import pytest
import torch

from oracle import tower_oracle, trunk_reference as tr
from tests import test_gpu_trunk_arith as ta

pytestmark = pytest.mark.gpu

DEV = ta.DEV
BLOCKS = 3
FILTERS = 128
SIZES = (8, 12)
NB4 = (128, 4, 1, 0, 0)
NB2 = (128, 2, 1, 0, 0)
_CACHE = {}


def _weights():
    if "w" not in _CACHE:
        _CACHE["w"] = tower_oracle.init_weights(BLOCKS, FILTERS, seed=11, randomize_bn=True)
    return _CACHE["w"]


def _both_kernels(model, planes, k):
    """(trunk, heads) of the NB = 4 kernel and of the NB = 2 kernel for one plane tensor at n_blocks = k."""
    L = ta._lib()
    n = planes.shape[0]
    flags = L.TRUNK_BITPLANES if planes.dtype == torch.int64 else 0
    bits = 1 if planes.dtype == torch.int64 else 0
    with L.trunk_set_small_batch(0):
        assert ta._kernel_name(FILTERS, n, flags) == ta._x16_name(*NB4, bits=bits)
        x4, h4 = ta._run(model, "f16", planes, k)
    assert ta._kernel_name(FILTERS, n, flags) == ta._x16_name(*NB2, bits=bits)           # (the default, restored)
    x2, h2 = ta._run(model, "f16", planes, k)
    return x4, h4, x2, h2


def _check(w, planes16, label):
    """Every depth 0 .. BLOCKS, both plane formats: NB = 4 == NB = 2 bit for bit, and the layer-local chain and the
    heads against the float64 reference.  -> the NB = 4 kernel's X_BLOCKS."""
    P = tr.prepare(w, DEV)
    model = ta._model(w, "f16")
    bits = ta._bits_from_planes(planes16)
    prev = None
    for k in range(BLOCKS + 1):
        x4, h4, x2, h2 = _both_kernels(model, bits, k)
        x4p, h4p, x2p, h2p = _both_kernels(model, planes16, k)
        assert torch.equal(x4, x2) and torch.equal(h4, h2), (label, k, "bitboards: NB 4 differs from NB 2")
        assert torch.equal(x4p, x2p) and torch.equal(h4p, h2p), (label, k, "fp16 planes: NB 4 differs from NB 2")
        assert torch.equal(x4, x4p) and torch.equal(h4, h4p), (label, k, "the two plane formats differ")
        ref = tr.stem(P, planes16, "f16") if k == 0 else tr.block(P, k - 1, prev, "f16", "fp32")
        s = ta._stats(x4, ref)
        print("%s n_blocks=%d: chain (max, p99.9) = %s" % (label, k, s))
        assert ta._within(s, "f16"), (label, k, s, ta.CHAIN_BOUND["f16"])
        prev, heads = x4, h4
    he = ta._heads_error(P, prev, heads)
    print("%s: heads = %g" % (label, he))
    assert he <= ta.HEADS_BOUND, (label, he)
    return prev


@pytest.mark.parametrize("first_full", [0, 1])
def test_pair_isolation(first_full):
    """Boards alternate between all 127 planes set and empty, in one order and in the other: a lane of one board
    that reads a row of its pair partner sees 127 ones where the reference has none."""
    for n in SIZES:
        planes = torch.zeros((n, 8, 8, 128), dtype=torch.float16, device=DEV)
        planes[(1 - first_full)::2, :, :, :127] = 1
        x = _check(_weights(), planes, "pair isolation first_full=%d n=%d" % (first_full, n))
        assert not torch.equal(x[0], x[1])


def _edge_planes(n, seed):
    """Bits only on ranks 1, 2, 7, 8 and on files a, h (density 0.5 there)."""
    rng = np.random.default_rng(seed)
    on = np.zeros((8, 8), bool)
    on[[0, 1, 6, 7], :] = True
    on[:, [0, 7]] = True
    p = (rng.random((n, 8, 8, 127)) < 0.5) & on[None, :, :, None]
    planes = torch.zeros((n, 8, 8, 128), dtype=torch.float16, device=DEV)
    planes[..., :127] = torch.from_numpy(p.astype(np.float16)).to(DEV)
    return planes


@pytest.mark.parametrize("tap", range(9))
def test_one_tap_weights(tap):
    """Every 3x3 convolution's weights are zero except one tap (the randomised-BN biases stay), on planes whose bits
    sit on the border ranks and files: an on-board block that is skipped loses its only products, an off-board row
    that is read adds products the reference does not have, and a wrong rank order in the upper half moves them."""
    w = dict(_weights())
    for name in list(w):
        if name.endswith(".kernel") and np.asarray(w[name]).ndim == 4 and np.asarray(w[name]).shape[0] == 3:
            k = np.zeros_like(w[name])
            k[tap // 3, tap % 3] = np.asarray(w[name])[tap // 3, tap % 3]
            w[name] = k
    for n in SIZES:
        _check(w, _edge_planes(n, 60 + n), "one tap %d n=%d" % (tap, n))


def test_every_wave_slot_carries_signal():
    """Random planes (density 0.15): besides the checks of every case, the outputs differ between the boards of a
    pair and between the ranks -- none of this file passes on a constant."""
    for n in SIZES:
        x = _check(_weights(), ta._random_planes(n, seed=70 + n), "random n=%d" % n)
        for b in range(0, n, 2):
            assert not torch.equal(x[b], x[b + 1]), ("boards of a pair", b)
        for b in range(n):
            for y in range(7):
                assert not torch.equal(x[b, y], x[b, y + 1]), ("ranks", b, y)
