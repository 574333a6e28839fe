"""CPU: oracle/trunk_reference.py, the float64 operand-exact reference the fused trunk kernels are held to
(tests/test_gpu_trunk_arith.py).  Before it may judge a kernel it must itself be right: its "exact" mode is
the fp32 tower oracle's arithmetic, single elements recomputed by scalar loops agree with it, and its
rounding modes really round (f16x3 lands next to exact, f16 does not)."""
import numpy as np
import pytest
import torch

from oracle import tower_oracle, trunk_reference as tr

BLOCKS, FILTERS, BOARDS = 2, 64, 4
# output squares of the scalar checks: corners, edges, interior (row, col)
SQUARES = [(0, 0), (7, 7), (0, 7), (7, 0), (0, 3), (4, 7), (3, 4)]


@pytest.fixture(scope="module")
def net():
    w = tower_oracle.init_weights(BLOCKS, FILTERS, seed=5, randomize_bn=True)
    rng = np.random.default_rng(5)
    for name in list(w):                        # non-zero biases: a bias row must matter
        if name.endswith(".bias") and "dense" not in name:
            w[name] = rng.normal(0, 0.1, w[name].shape).astype(np.float32)
    planes = (rng.random((BOARDS, 8, 8, 127)) < 0.2).astype(np.float32)
    return w, planes, tr.prepare(w)


def _oracle_trunk(w, planes):
    """The trunk of oracle/tower_oracle.forward (fp32 torch), NHWC."""
    x = torch.as_tensor(planes).float().permute(0, 3, 1, 2)
    x = tower_oracle._conv(x, w, "stem", 1)
    for i in range(int(w["meta.blocks"])):
        y = torch.relu(tower_oracle._bn(tower_oracle._conv(x, w, "block%d.conv1" % i, 1), w, "block%d.bn1" % i))
        y = tower_oracle._bn(tower_oracle._conv(y, w, "block%d.conv2" % i, 1), w, "block%d.bn2" % i)
        x = torch.relu(x + y)
    return x


def test_exact_mode_is_the_fp32_tower_oracle(net):
    w, planes, P = net
    x = tr.trunk(P, planes, "exact")
    ref = _oracle_trunk(w, planes)
    scale = ref.abs().max().item()
    assert (x - ref.permute(0, 2, 3, 1).double()).abs().max().item() <= 2e-6 * scale
    # heads in the kernel's row layout against the oracle's head convolutions
    h = tr.heads(P, x)
    p = torch.relu(tower_oracle._bn(tower_oracle._conv(ref, w, "policy.conv", 0), w, "policy.bn"))
    v = torch.relu(tower_oracle._bn(tower_oracle._conv(ref, w, "value.conv", 0), w, "value.bn"))
    p = p.permute(0, 2, 3, 1).reshape(BOARDS, 128)
    v = v.permute(0, 2, 3, 1).reshape(BOARDS, 64)
    hs = max(p.abs().max().item(), v.abs().max().item())
    assert (h[:, :128] - p.double()).abs().max().item() <= 2e-6 * hs
    assert (h[:, 128:] - v.double()).abs().max().item() <= 2e-6 * hs
    # ... and through the dense layers to the oracle's policy and value
    hp = h[:, :128].float()
    pol = torch.softmax(hp @ torch.from_numpy(w["policy.dense.kernel"]) + torch.from_numpy(w["policy.dense.bias"]), -1)
    vv = torch.relu(h[:, 128:].float() @ torch.from_numpy(w["value.dense1.kernel"]) + torch.from_numpy(w["value.dense1.bias"]))
    val = torch.tanh(vv @ torch.from_numpy(w["value.dense2.kernel"]) + torch.from_numpy(w["value.dense2.bias"]))[:, 0]
    epol, eval_ = tower_oracle.forward(w, planes)
    assert (pol - epol).abs().max().item() <= 1e-6 and (val - eval_).abs().max().item() <= 1e-6


def _fold_scalar(w, conv, bn, o):
    """(kernel [ky][kx][i] of output channel o, bias) folded with plain Python floats."""
    k = np.asarray(w[conv + ".kernel"], np.float64)[..., o]
    b = float(w[conv + ".bias"][o])
    if bn is None:
        return k, b
    s = float(w[bn + ".gamma"][o]) / np.sqrt(float(w[bn + ".var"][o]) + tower_oracle.BN_EPS)
    return k * s, (b - float(w[bn + ".mean"][o])) * s + float(w[bn + ".beta"][o])


def _conv_scalar(src, k, b, row, col, split_w=None):
    """One output of a 'same' 3x3 convolution by a scalar loop over taps and input channels; src [8][8][C]
    (numpy float64).  ``split_w``: callable(k value) -> the value the kernel multiplies by."""
    acc = b
    for ky in range(3):
        for kx in range(3):
            r, c = row + ky - 1, col + kx - 1
            if not (0 <= r < 8 and 0 <= c < 8):
                continue                                    # zero border
            for i in range(src.shape[-1]):
                wv = float(k[ky, kx, i])
                acc += float(src[r, c, i]) * (split_w(wv) if split_w else wv)
    return acc


def test_scalar_loops_agree_with_the_reference_on_single_elements(net):
    w, planes, P = net
    bd, blk = 1, 1
    x0 = tr.stem(P, planes)
    x1, y1 = tr.block(P, blk, x0, mid=True)                      # (block 1 on the stem: any block input will do)
    checked = 0
    for o in (0, 17, FILTERS - 1):
        ks, bs = _fold_scalar(w, "stem", None, o)
        k1, b1 = _fold_scalar(w, "block%d.conv1" % blk, "block%d.bn1" % blk, o)
        k2, b2 = _fold_scalar(w, "block%d.conv2" % blk, "block%d.bn2" % blk, o)
        for row, col in SQUARES:
            s = _conv_scalar(planes[bd].astype(np.float64), ks, bs, row, col)
            assert abs(s - x0[bd, row, col, o].item()) <= 1e-12 * max(1.0, abs(s))
            c1 = max(0.0, _conv_scalar(x0[bd].numpy(), k1, b1, row, col))
            assert abs(c1 - y1[bd, row, col, o].item()) <= 1e-12 * max(1.0, abs(c1))
            c2 = max(0.0, _conv_scalar(y1[bd].numpy(), k2, b2, row, col) + x0[bd, row, col, o].item())
            assert abs(c2 - x1[bd, row, col, o].item()) <= 1e-12 * max(1.0, abs(c2))
            checked += 3
    # heads (the kernel's fp32 head weights: the host's fold, pinned bit for bit below): policy channel k of
    # position p at row p*2 + k, the value at 128 + p
    hw, hb = P.head_w.numpy(), P.head_b.numpy()
    for k, (kk, bb) in enumerate([_fold_scalar(w, "policy.conv", "policy.bn", k) for k in (0, 1)]
                                 + [_fold_scalar(w, "value.conv", "value.bn", 0)]):
        assert np.abs(hw[:, k] - kk[0, 0]).max() <= 1e-6 * np.abs(kk).max() and abs(hb[k] - bb) <= 1e-6 * max(1, abs(bb))
    h = tr.heads(P, x1)
    for row, col in SQUARES:
        pos = row * 8 + col
        xv = x1[bd, row, col].numpy()
        for k in range(3):
            e = max(0.0, sum(float(hw[i, k]) * float(xv[i]) for i in range(FILTERS)) + float(hb[k]))
            assert abs(e - h[bd, pos * 2 + k if k < 2 else 128 + pos].item()) <= 1e-12 * max(1.0, abs(e))
        checked += 3
    assert checked == 3 * len(SQUARES) * 4


def test_scalar_loop_of_the_split_product_agrees_with_the_f16x3_reference(net):
    """hi*Whi + lo*Whi + hi*Wlo with numpy's fp16 for hi, lo, Whi, Wlo, element by element."""
    w, planes, P = net
    bd, blk = 2, 0
    x0 = tr.stem(P, planes, "f16x3")
    _, y = tr.block(P, blk, x0, "f16x3", mid=True)
    hi = x0[bd].numpy().astype(np.float16).astype(np.float64)
    lo = (x0[bd].numpy() - hi).astype(np.float16).astype(np.float64)
    k32, b32 = tr._fold32(w, "block%d.conv1" % blk, "block%d.bn1" % blk)      # the host's fp32 fold (pinned below)
    k32, b32 = k32.numpy().reshape(3, 3, FILTERS, FILTERS), b32.numpy()
    whi = lambda v: float(np.float16(np.float32(v)))
    wlo = lambda v: float(np.float16(np.float32(v) - np.float32(np.float16(np.float32(v)))))
    for o in (3, 40):
        k, b = k32[..., o], float(b32[o])
        for row, col in SQUARES:
            acc = (_conv_scalar(hi, k, b, row, col, whi) + _conv_scalar(lo, k, 0.0, row, col, whi)
                   + _conv_scalar(hi, k, 0.0, row, col, wlo))
            e = max(0.0, acc)
            assert abs(e - y[bd, row, col, o].item()) <= 1e-12 * max(1.0, abs(e))


def test_rounded_modes_start_from_the_hosts_fp32_fold_bit_for_bit(net):
    """The emulated modes' weights are the host's stored fp32 values (chessrl_amd.packing.fold: what pack_trunk
    rounds to Whi / Wlo and what the kernels add as biases); the float64 fold is within fp32 rounding of them."""
    from chessrl_amd.model import _fold
    w, _, P = net
    convs = [("stem", None, P.stem)] + [("block%d.conv%d" % (i, j), "block%d.bn%d" % (i, j), c)
                                        for i in range(BLOCKS) for j, c in ((1, P.conv1[i]), (2, P.conv2[i]))]
    for conv, bn, c in convs:
        k, b = _fold(w, conv, bn)                                          # OIHW fp32
        k = k.permute(2, 3, 1, 0).reshape(9, k.shape[1], k.shape[0])       # [tap][in][out]
        hi = k.half()
        assert torch.equal(c.whi, hi.double()) and torch.equal(c.wlo, (k - hi.float()).half().double())
        assert torch.equal(c.b32, b.double())
        assert (c.w - k.double()).abs().max().item() <= 2.0 ** -23 * k.abs().max().item()
    kp, bp = _fold(w, "policy.conv", "policy.bn")
    kv, bv = _fold(w, "value.conv", "value.bn")
    assert torch.equal(P.head_w, torch.cat([kp.reshape(2, FILTERS), kv.reshape(1, FILTERS)]).t().double())
    assert torch.equal(P.head_b, torch.cat([bp, bv]).double())


def test_split_emulation_is_next_to_exact_and_f16_is_not(net):
    w, planes, P = net
    exact = tr.trunk(P, planes, "exact")
    scale = exact.abs().max().item()
    bound = 2.0 ** -20 * scale
    for skip in tr.SKIPS:
        d = (tr.trunk(P, planes, "f16x3", skip) - exact).abs().max().item()
        assert 0 < d <= bound, (skip, d / scale)
    d16 = (tr.trunk(P, planes, "f16") - exact).abs().max().item()
    assert d16 > 16 * bound, d16 / scale                       # the fp16 rounding is really applied
    # dropping one of the three split products moves the result far outside the split bound
    for drop in ("lo_whi", "hi_wlo"):
        assert (tr.trunk(P, planes, "f16x3", drop=drop) - exact).abs().max().item() > 16 * bound


def test_hilo_skip_differs_from_the_fp32_skip_by_at_most_2_to_the_minus_22(net):
    w, planes, P = net
    x = tr.trunk(P, planes, "exact", n_blocks=1).flatten()
    x = x[x != 0]
    hi, lo = tr.split(x)
    err = ((hi + lo) - x).abs()
    # lo = fp16(x - hi) is off by at most 2^-11 |lo| <= 2^-22 |x| while lo is an fp16 normal, by at most half the
    # smallest fp16 subnormal (2^-25) below: 2^-22 relative wherever |x| >= 2^-3
    big = x.abs() >= 2.0 ** -3
    assert big.sum() > 100 and (~big).sum() > 100
    assert (err[big] / x[big].abs()).max().item() <= 2.0 ** -22
    assert (err <= torch.clamp(2.0 ** -22 * x.abs(), min=2.0 ** -25)).all()
    assert (err[big] / x[big].abs()).max().item() > 2.0 ** -26     # ... and the two skips are not the same
    # the whole trunk with either skip: the same up to that rounding, but not equal
    a, b = tr.trunk(P, planes, "f16x3", "fp32"), tr.trunk(P, planes, "f16x3", "hilo")
    assert 0 < (a - b).abs().max().item() <= 2.0 ** -20 * a.abs().max().item()


def test_magnitude_scaling_scales_every_activation(net):
    w, planes, P = net
    x = tr.trunk(P, planes, "exact", every=True)
    for s in (1e-3, 1e4):
        Ps = tr.prepare(tr.scale_magnitude(w, s))
        xs = tr.trunk(Ps, planes, "exact", every=True)
        for a, b in zip(x, xs):
            assert (b - s * a).abs().max().item() <= 1e-6 * s * a.abs().max().item()
        h, hs = tr.heads(P, x[-1]), tr.heads(Ps, xs[-1])
        assert (hs - s * h).abs().max().item() <= 1e-6 * s * h.abs().max().item()


def test_modes_and_knobs_are_checked():
    w = tower_oracle.init_weights(1, 64, seed=0)
    P = tr.prepare(w)
    planes = np.zeros((4, 8, 8, 127), np.float32)
    with pytest.raises(ValueError):
        tr.stem(P, planes, "f32")
    with pytest.raises(ValueError):
        tr.block(P, 0, tr.stem(P, planes), "f16", drop="lo_whi")
    with pytest.raises(ValueError):
        tr.block(P, 0, tr.stem(P, planes), "f16x3", skip="f16")
