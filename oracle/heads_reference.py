"""oracle/heads_reference.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

float64 restatement of the ARITHMETIC the dense-head kernels claim to perform (chessrl_amd/csrc/heads.hpp,
chessrl_amd/csrc/slices.hpp), operand for operand, from the 192 head activations per board that the trunk leaves
([0,128) policy, [128,192) value):

    policy = softmax(act[:128] . Wp[128][1968] + bp)                      Dense(1968, softmax)
    value  = tanh(relu(act[128:] . W1[64][256] + b1) . w2[256] + b2)      Dense(256, relu) -> Dense(1, tanh)

The kernels run both products on fp16 MFMAs over split operands (heads.hpp:10-13): an fp32 number x is carried as
hi = fp16(x), lo = fp16(x - hi) (fp16 subnormals kept), and  W.h = Whi.hhi + Wlo.hhi + Whi.hlo  is accumulated in
fp32 on top of the bias.  This module applies the same roundings in float64, so that what is left between a kernel
and ``mode="split"`` is the kernel's fp32 summation order.  It works from the Keras-layout weight dict
(oracle/tower_oracle.init_weights) and does NOT go through chessrl_amd.packing.pack_dense / pack_split:
a packing bug is not shared by kernel and reference.  ``unpack_split`` inverts the documented fragment layout
independently (heads.hpp:15-18), for the tests of the packing itself.

Modes: ``exact`` (float64 weights and activations, no rounding anywhere) and ``split`` (above).  ``drop`` drops one
of the three products ("lo_whi": Whi.hlo, "hi_wlo": Wlo.hhi): the negative controls of the tests.

The sliced form of the policy head (heads.hpp: k_heads_sliced + k_policy_normalise, slices.hpp) cuts the 2048 padded
labels (bias -1e30 beyond 1967) into 8 slices of 256 and leaves per board and slice (m = max logit, s = sum exp(l - m));
a probability is exp(l - M) / S with M = max_k m_k, S = sum_k s_k exp(m_k - M): ``slice_stats`` / ``prob_from_stats``.

Everything is plain torch float64 on ``device``.  Only tests/ may import this module.
"""
import numpy as np
import torch

N_LABELS = 1968
N_LABELS_PAD = 2048
N_SLICES = 8
SLICE = N_LABELS_PAD // N_SLICES
PAD_BIAS = -1e30
POL_IN, VAL_IN, VAL_HIDDEN = 128, 64, 256
MODES = ("exact", "split")
DROPS = (None, "lo_whi", "hi_wlo")


def _f16(x):
    return x.to(torch.float16).to(torch.float64)


def split(x):
    """(hi, lo) = (fp16(x), fp16(x - hi)) of the fp32 values x, as float64.  x - hi is exact in fp32 (and in
    float64), so the single rounding float64 -> fp16 is the kernel's fp32 -> fp16 one; subnormals are kept."""
    x = torch.as_tensor(x).to(torch.float32).to(torch.float64)
    hi = _f16(x)
    return hi, _f16(x - hi)


class _Dense(object):
    """One dense kernel [in][out]: float64 (exact), the fp32 values and their fp16 pair, the fp32 bias."""

    def __init__(self, w, name, device):
        k32 = torch.as_tensor(np.asarray(w[name + ".kernel"], np.float32))
        b32 = torch.as_tensor(np.asarray(w[name + ".bias"], np.float32))
        self.w = torch.as_tensor(np.asarray(w[name + ".kernel"], np.float64)).to(device)
        self.b = torch.as_tensor(np.asarray(w[name + ".bias"], np.float64)).to(device)
        hi, lo = split(k32)
        self.whi, self.wlo = hi.to(device), lo.to(device)
        self.b32 = b32.to(torch.float64).to(device)


class HeadWeights(object):
    def __init__(self, w, device="cpu"):
        self.device = torch.device(device)
        self.policy = _Dense(w, "policy.dense", device)               # [128][1968]
        self.value1 = _Dense(w, "value.dense1", device)               # [64][256]
        w2 = np.asarray(w["value.dense2.kernel"], np.float32).reshape(-1)
        b2 = np.asarray(w["value.dense2.bias"], np.float32).reshape(-1)
        assert self.policy.w.shape == (POL_IN, N_LABELS) and self.value1.w.shape == (VAL_IN, VAL_HIDDEN)
        assert w2.shape == (VAL_HIDDEN,) and b2.shape == (1,)
        self.w2 = torch.as_tensor(w2.astype(np.float64)).to(device)   # fp32 values (the kernel reads fp32)
        self.b2 = float(b2[0])
        pad = torch.full((N_LABELS_PAD,), PAD_BIAS, dtype=torch.float32)
        pad[:N_LABELS] = torch.as_tensor(np.asarray(w["policy.dense.bias"], np.float32))
        self.bias_pad = pad.to(device)                                # fp32 [2048], as the kernel reads it


def prepare(w, device="cpu"):
    return HeadWeights(w, device)


def _check(mode, drop):
    if mode not in MODES or drop not in DROPS or (drop is not None and mode != "split"):
        raise ValueError("mode %r, drop %r" % (mode, drop))


def _affine(d, x, mode, drop):
    """bias + x . W of dense layer d in ``mode``: the accumulator before the activation."""
    if mode == "exact":
        return x @ d.w + d.b
    hi, lo = split(x)
    hi, lo = hi.to(d.whi.device), lo.to(d.whi.device)
    acc = (hi if drop == "lo_whi" else hi + lo) @ d.whi               # hi + lo: exact in float64
    if drop != "hi_wlo":
        acc = acc + hi @ d.wlo
    return acc + d.b32


def _act(P, act, lo, hi):
    return torch.as_tensor(act)[:, lo:hi].to(device=P.device, dtype=torch.float64)


def logits(P, act, mode="exact", drop=None):
    """[n][1968] policy logits of the head activations act [n][192] (fp32 values)."""
    _check(mode, drop)
    return _affine(P.policy, _act(P, act, 0, POL_IN), mode, drop)


def logit_condition(P, act):
    """[n][1968] |x| . |W| + |b|: the scale of a logit's fp32 rounding error."""
    return _act(P, act, 0, POL_IN).abs() @ P.policy.w.abs() + P.policy.b.abs()


def softmax(lg):
    """float64 softmax over the 1968 labels."""
    lg = torch.as_tensor(lg).to(torch.float64)
    e = torch.exp(lg - lg.max(dim=-1, keepdim=True).values)
    return e / e.sum(dim=-1, keepdim=True)


def pad_logits(lg):
    """[n][2048]: the logits with the kernel's pad (-1e30: bias of the pad labels, whose weights are zero)."""
    lg = torch.as_tensor(lg).to(torch.float64)
    out = torch.full(lg.shape[:-1] + (N_LABELS_PAD,), PAD_BIAS, dtype=torch.float64, device=lg.device)
    out[..., :N_LABELS] = lg
    return out


def slice_stats(lg):
    """[n][8][2] = (m_k, s_k): max logit of slice k and sum exp(l - m_k) over the slice, of the 8 slices of 256
    padded labels."""
    p = pad_logits(lg).reshape(-1, N_SLICES, SLICE)
    m = p.max(dim=-1).values
    s = torch.exp(p - m.unsqueeze(-1)).sum(dim=-1)
    return torch.stack([m, s], dim=-1)


def norm_from_stats(stats):
    """(M [n], S [n]) of stats [n][8][2]: M = max_k m_k, S = sum_k s_k exp(m_k - M)."""
    stats = torch.as_tensor(stats).to(torch.float64)
    m, s = stats[..., 0], stats[..., 1]
    M = m.max(dim=-1).values
    return M, (s * torch.exp(m - M.unsqueeze(-1))).sum(dim=-1)


def prob_from_stats(logit, stats):
    """slices.hpp in float64: exp(l - M) / S for logit [n][...] and stats [n][8][2]."""
    logit = torch.as_tensor(logit).to(torch.float64)
    M, S = norm_from_stats(stats)
    shape = (-1,) + (1,) * (logit.dim() - 1)
    return torch.exp(logit - M.reshape(shape)) / S.reshape(shape)


def value_preact(P, act, mode="exact", drop=None):
    """[n] z = relu(x . W1 + b1) . w2 + b2, the argument of the tanh."""
    _check(mode, drop)
    h = torch.relu(_affine(P.value1, _act(P, act, POL_IN, POL_IN + VAL_IN), mode, drop))
    return h @ P.w2 + P.b2


def value(P, act, mode="exact", drop=None):
    return torch.tanh(value_preact(P, act, mode, drop))


def value_condition(P, act):
    """[n] (|x| . |W1| + |b1|) . |w2| + |b2|: the scale of the fp32 rounding error of the tanh's argument."""
    h = _act(P, act, POL_IN, POL_IN + VAL_IN).abs() @ P.value1.w.abs() + P.value1.b.abs()
    return h @ P.w2.abs() + abs(P.b2)


def fragment_offset(unit, inp, ksteps, lo=0):
    """Offset (in halves) of x[unit][inp] in the packed image [tile][k-step][hi|lo][q][r][8]: lane 16 q + r of
    fragment (tile, k-step) holds x[16 tile + r][32 s + 8 q + e]."""
    t, r = divmod(unit, 16)
    s, rest = divmod(inp, 32)
    q, e = divmod(rest, 8)
    return ((((t * ksteps + s) * 2 + lo) * 4 + q) * 16 + r) * 8 + e


def unpack_split(image, tiles, ksteps):
    """Inverse of the fragment layout: the flat fp16 image -> (hi, lo), each fp16 [16 tiles][32 ksteps]."""
    image = torch.as_tensor(image)
    assert image.dtype == torch.float16 and image.numel() == tiles * ksteps * 2 * 64 * 8
    frag = image.reshape(tiles, ksteps, 2, 4, 16, 8)                  # [t][s][hl][q][r][e]
    x = frag.permute(2, 0, 4, 1, 3, 5).reshape(2, tiles * 16, ksteps * 32)   # [hl][t][r][s][q][e]
    return x[0].contiguous(), x[1].contiguous()
