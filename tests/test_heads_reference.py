"""CPU: oracle/heads_reference.py checking itself, and the host-side packing of the dense heads
(chessrl_amd.packing: pack_split / pack_dense) against the layout chessrl_amd/csrc/heads.hpp documents.

The GPU comparisons (tests/test_gpu_heads_arith.py) rest on what is established here: that "split" is the fp32 layers'
arithmetic to ~2^-22 of a logit's condition, that each of its three products matters (a dropped one is >= 100x worse),
that hi + lo pairs are exact fp32 numbers (the bit-exact probes), and that the sliced softmax formula is the softmax.
"""
import numpy as np
import pytest
import torch

from oracle import heads_reference as hr
from tests import heads_util as hu

N = 1000                                     # boards of the self-check (test_gpu_search.py's largest heads batch)
# |split - exact| <= this x (|x|.|W| + |b|): each operand pair hi + lo holds its fp32 value to 2^-22 relative (11 + 11
# significand bits, normal range), and the dropped lo.lo product is below 2^-22 of |x||W|: three terms of 2^-22.
SPLIT_BOUND = 3 * 2.0 ** -22                 # = 7.2e-7; found 3.7e-7 (flat: 1.4e-6 absolute), 5.6e-8 (peaked) of the condition
# an fp32 dot product of n terms + bias, any summation order: gamma_n = n u / (1 - n u), u = 2^-24 (Higham 3.5)
FP32_BOUND = {128: 129 * 2.0 ** -24, 64: 65 * 2.0 ** -24}


def _sets():
    flat = hu.flat_weights()
    act = hu.activations(N, "base", seed=1000)
    return {"flat": (flat, act), "peaked": (hu.scaled_policy(flat, act, hu.PEAKED_SPREAD), act),
            "huge": (hu.scaled_policy(flat, act, hu.HUGE_SPREAD), act)}


@pytest.fixture(scope="module")
def sets():
    return _sets()


def _tower(w):
    from chessrl_amd.model import Tower
    net = Tower(2, 64)
    net.load_keras_dict(w)
    return net.float().eval()


@pytest.mark.parametrize("kind", ["flat", "peaked"])
def test_split_is_the_fp32_layers_arithmetic_and_every_product_matters(sets, kind):
    w, act = sets[kind]
    P = hr.prepare(w)
    exact, cond = hr.logits(P, act, "exact"), hr.logit_condition(P, act)
    sp = hr.logits(P, act, "split")
    err = (sp - exact).abs()
    p_exact, p_split = hr.softmax(exact), hr.softmax(sp)
    rel_p = ((p_split - p_exact).abs() / p_exact).max().item()
    net = _tower(w)
    with torch.no_grad():
        l32 = net.policy_fc(torch.from_numpy(act[:, :128])).double()
        v32 = torch.tanh(net.value_fc2(torch.relu(net.value_fc1(torch.from_numpy(act[:, 128:]))))[:, 0]).double()
    e32 = ((l32 - exact).abs() / cond).max().item()
    print("%s: split vs exact max |dlogit| %.3g (%.3g of the condition), max rel dp %.3g; torch fp32 vs exact %.3g of "
          "the condition" % (kind, err.max().item(), (err / cond).max().item(), rel_p, e32))
    assert (err / cond).max().item() <= SPLIT_BOUND
    assert e32 <= FP32_BOUND[128]
    for drop in ("lo_whi", "hi_wlo"):
        d = (hr.logits(P, act, "split", drop) - exact).abs().max().item()
        print("%s: drop %s max |dlogit| %.3g" % (kind, drop, d))
        assert d >= 100 * err.max().item(), (drop, d)
    # the value head, the same way
    z, zc = hr.value_preact(P, act, "exact"), hr.value_condition(P, act)
    zs = hr.value_preact(P, act, "split")
    zerr = (zs - z).abs()
    assert (zerr / zc).max().item() <= SPLIT_BOUND
    assert (v32 - hr.value(P, act, "exact")).abs().max().item() <= (FP32_BOUND[64] + 257 * 2.0 ** -24) * zc.max().item() + 2e-7
    for drop in ("lo_whi", "hi_wlo"):
        d = (hr.value_preact(P, act, "split", drop) - z).abs().max().item()
        print("%s: value drop %s max |dz| %.3g (split %.3g)" % (kind, drop, d, zerr.max().item()))
        assert d >= 100 * zerr.max().item(), (drop, d)
    assert torch.equal(hr.value(P, act, "split"), torch.tanh(zs))


def test_modes_and_drops_are_checked():
    P = hr.prepare(hu.flat_weights())
    act = hu.activations(2)
    with pytest.raises(ValueError):
        hr.logits(P, act, "f16")
    with pytest.raises(ValueError):
        hr.logits(P, act, "exact", "lo_whi")
    with pytest.raises(ValueError):
        hr.value(P, act, "split", "lo_lo")


@pytest.mark.parametrize("tiles,ksteps", [(128, 4), (16, 2)])
def test_unpack_split_inverts_pack_split_for_every_element(tiles, ksteps):
    from chessrl_amd import packing
    rng = np.random.default_rng(tiles)
    x = torch.from_numpy((rng.normal(0, 1, (tiles * 16, ksteps * 32)) * 10.0 ** rng.integers(-6, 3, (tiles * 16, 1)))
                         .astype(np.float32))
    image = packing.pack_split(x, tiles, ksteps)
    assert image.dtype == torch.float16 and image.numel() == 2 * x.numel()
    hi, lo = hr.unpack_split(image, tiles, ksteps)
    ehi = x.half()
    elo = (x - ehi.float()).half()
    assert torch.equal(hi.view(torch.int16), ehi.view(torch.int16))
    assert torch.equal(lo.view(torch.int16), elo.view(torch.int16))
    # the reference's own split (float64 route) is the same pair, and fragment_offset finds single elements
    rhi, rlo = hr.split(x)
    assert torch.equal(rhi, ehi.double()) and torch.equal(rlo, elo.double())
    for unit, inp in ((0, 0), (17, 41), (tiles * 16 - 1, ksteps * 32 - 1), (5 * 16 + 3, 32 + 8 + 7)):
        assert image[hr.fragment_offset(unit, inp, ksteps, 0)] == ehi[unit, inp]
        assert image[hr.fragment_offset(unit, inp, ksteps, 1)] == elo[unit, inp]


def test_pack_dense_places_everything_where_the_kernels_read_it(sets):
    from chessrl_amd import packing
    w, _ = sets["flat"]
    P = hr.prepare(w)
    pol_wp, pol_bias, val_w1p, val_b1, val_w2 = packing.pack_dense(w)
    hi, lo = hr.unpack_split(pol_wp, 128, 4)                            # [2048 labels][128 inputs]
    assert torch.equal(hi[:1968].double(), P.policy.whi.t()) and torch.equal(lo[:1968].double(), P.policy.wlo.t())
    assert not hi[1968:].any() and not lo[1968:].any()                  # the pad labels: zero weights ...
    assert pol_bias.dtype == torch.float32 and pol_bias.shape == (2048,)
    assert torch.equal(pol_bias, P.bias_pad)
    assert torch.equal(pol_bias[:1968], torch.from_numpy(w["policy.dense.bias"]))
    assert (pol_bias[1968:] == np.float32(-1e30)).all()                 # ... and a bias no logit reaches
    hi, lo = hr.unpack_split(val_w1p, 16, 2)                            # [256 hidden][64 inputs]
    assert torch.equal(hi.double(), P.value1.whi.t()) and torch.equal(lo.double(), P.value1.wlo.t())
    assert torch.equal(val_b1, torch.from_numpy(w["value.dense1.bias"]))
    assert val_w2.dtype == torch.float32 and val_w2.shape == (257,)
    assert torch.equal(val_w2[:256].double(), P.w2) and val_w2[256].item() == P.b2


def _fp32_exact(x):
    return torch.equal(x.to(torch.float32).to(torch.float64), x)


def test_hi_plus_lo_is_an_exact_fp32_number(sets):
    """The bit-exact GPU probes rest on it: fp32(Whi) + fp32(Wlo) (and hhi + hlo) round nowhere."""
    w, _ = sets["flat"]
    for scale in (1.0, 37.3):
        ws = dict(w)
        for name in ("policy.dense.kernel", "value.dense1.kernel"):
            ws[name] = (np.asarray(w[name], np.float64) * scale).astype(np.float32)
        P = hr.prepare(ws)
        for d in (P.policy, P.value1):
            assert _fp32_exact(d.whi + d.wlo)
            # and the pair is the fp32 weight to 2^-22 (normal range)
            assert ((d.whi + d.wlo - d.w).abs() <= 2.0 ** -22 * d.w.abs() + 2.0 ** -25).all()
    for kind in ("base", "tiny", "big"):
        hi, lo = hr.split(torch.from_numpy(hu.activations(64, kind)))
        assert _fp32_exact(hi + lo)
    hi, lo = hr.split(torch.from_numpy(hu.activations(64, "tiny")))
    assert ((lo != 0) & (lo.abs() < 2.0 ** -14)).any()                  # "tiny" does reach fp16 subnormals


@pytest.mark.parametrize("kind", ["flat", "peaked", "huge"])
def test_slice_formula_is_the_softmax(sets, kind):
    w, act = sets[kind]
    P = hr.prepare(w)
    lg = hr.logits(P, act[:64], "split")
    spread = (lg.max(1).values - lg.min(1).values).min().item()
    assert spread >= {"flat": 0.0, "peaked": 40.0, "huge": 200.0}[kind]
    p = hr.softmax(lg)
    st = hr.slice_stats(lg)
    assert st.shape == (64, 8, 2)
    assert (st[:, :7, 1] >= 1).all() and (st[:, :, 1] <= 256).all() and (st[:, 7, 1] <= 176).all()
    assert torch.equal(st[:, :, 0].max(1).values, lg.max(1).values)     # the pad never holds a maximum
    q = hr.prob_from_stats(lg, st)
    live = p > 1e-300
    assert (((q - p).abs() / p.clamp(min=1e-300))[live]).max().item() <= 1e-12
    assert (q[~live] <= 1e-299).all()
    assert (p.sum(1) - 1).abs().max().item() <= 1e-13 and (q.sum(1) - 1).abs().max().item() <= 1e-12


def test_weight_sets_hold_their_preconditions(sets):
    w, act = sets["flat"]
    rows = hu.activations(hu.ROWS, "base")
    assert hu.logit_spread(hu.scaled_policy(w, rows, hu.PEAKED_SPREAD), rows).min() >= 40
    assert hu.logit_spread(hu.scaled_policy(w, rows, hu.HUGE_SPREAD), rows).min() >= 200
    big = hu.activations(1000, "base", seed=9)
    z = hu.value_z(hu.spread_value(w, big), big)
    print("peaked spread %s, value z %.3g .. %.3g, min |z| %.3g" % (
        np.sort(hu.logit_spread(hu.scaled_policy(w, rows, hu.PEAKED_SPREAD), rows))[[0, -1]], z.min(), z.max(), np.abs(z).min()))
    assert np.abs(z).max() >= 12 and np.abs(z).min() <= 0.05
    assert np.tanh(z).astype(np.float32).max() == 1.0 and np.tanh(z).astype(np.float32).min() == -1.0
