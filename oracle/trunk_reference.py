"""oracle/trunk_reference.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

float64 restatement of the ARITHMETIC the fused trunk kernels claim to perform (stem Conv3x3 + N residual
blocks with BatchNorm folded, then the three 1x1 head convolutions with their BN + ReLU), operand for
operand: where a kernel rounds an operand to fp16, or splits it into an fp16 pair, this reference applies
the same rounding in float64.  What is left between a kernel and this reference is then the kernel's fp32
summation order (~1e-6 relative), so a comparison can see one wrong weight, bias row or tap.

Everything is plain torch float64 on ``device`` (the GPU tests run it on the card).  A 3x3 convolution is
nine shifted ``[B*64, Cin] x [Cin, F]`` matmuls over an explicitly zero-bordered input -- no cuDNN / MIOpen.
BatchNorm is folded HERE, in float64, from the Keras-layout weight dict (oracle/tower_oracle.init_weights),
not by chessrl_amd.packing.fold / pack_trunk: a folding or packing bug is not shared by kernel and reference.
"exact" runs on that float64 fold.  The rounded modes start from the weights as the host stores them: folded in
fp32 (W32 = k * s, s = gamma / sqrt(var + eps), b32 = (b - mean) * s + beta: torch fp32 on the CPU, the operation
order of the host), then Whi = fp16(W32), Wlo = fp16(W32 - Whi); biases and head weights are those fp32 values.
(An fp32 rounding of the float64 fold differs from the host's fp32 fold in the last bit of about a third of the
weights, and that flips Whi of ~1 weight in 20 000 by one fp16 step: measured 2e-5 of max |X| in "f16", larger
than the kernels' summation-order error this reference is there to isolate.)

Modes (rounding points as csrc/tower_x16.hpp:686-772 and csrc/tower_layer.hpp:544-588 state them; the
accumulators start from the bias, tower_x16.hpp:327 / tower_layer.hpp:274):

* ``exact``: float64 folded weights and biases, no rounding anywhere.
* ``f16`` (one fp16 MFMA per product, k_trunk_x16 with SPLIT = 0): operands fp16(x), weights Whi.
  The stem's output is the fp32 skip stream, fp16(stem) the next operand (tower_x16.hpp:759-772);
  conv1 produces fp16(relu(acc)) (:726-739); conv2 produces relu(acc + skip), the new fp32 skip, whose
  fp16 rounding is the next operand (:740-758).
* ``f16x3`` (CRL_TRUNK_SPLIT): activations are carried as hi = fp16(x), lo = fp16(x - hi) (tower_x16.hpp:
  686-700, tower_layer.hpp:578-588) and every product is hi*Whi + lo*Whi + hi*Wlo (the stem's 0/1 planes
  have lo = 0).  The skip stream added by conv2 is, by ``skip``:
    - ``"fp32"``: the fp32 value (k_trunk_x16 keeps it in registers, tower_x16.hpp:701-725);
    - ``"hilo"``: hi + lo of the block input as it stands in the activation image (the layer-wise 256-filter
      kernels re-read it, tower_layer.hpp:544-553): within 2^-22 of the fp32 value, not equal to it.

Heads (tower_x16.hpp:806-849, tower_layer.hpp:560-607): ReLU of the three folded 1x1 convolutions over the
fp32 trunk output, in the kernel's row layout: policy at ``pos*2 + k``, value at ``128 + pos``.

Entry points: ``prepare`` (fold + round once), ``stem``, ``block`` (one residual block from a given block
input X_k: a kernel's own output can be fed back in), ``trunk`` (from the planes), ``heads``.  ``drop`` drops
one of the three split products ("lo_whi" or "hi_wlo"): the negative controls of the GPU tests.

Only tests/ may import this module.
"""
import numpy as np
import torch

BN_EPS = 1e-3
IN_PLANES = 127
MODES = ("exact", "f16", "f16x3")
SKIPS = ("fp32", "hilo")
DROPS = (None, "lo_whi", "hi_wlo")


def _fold64(w, conv, bn=None):
    """(kernel [9 taps = ky*3+kx][Cin][Cout], bias [Cout]) of `conv` with the following BatchNorm folded, float64."""
    k = np.asarray(w[conv + ".kernel"], np.float64)                    # HWIO
    b = np.asarray(w[conv + ".bias"], np.float64)
    if bn is not None:
        g, beta = np.asarray(w[bn + ".gamma"], np.float64), np.asarray(w[bn + ".beta"], np.float64)
        mean, var = np.asarray(w[bn + ".mean"], np.float64), np.asarray(w[bn + ".var"], np.float64)
        s = g / np.sqrt(var + BN_EPS)
        k = k * s
        b = (b - mean) * s + beta
    kh, kw, cin, cout = k.shape
    return k.reshape(kh * kw, cin, cout), b


def _fold32(w, conv, bn=None):
    """The same fold in fp32 as the host stores it (torch CPU fp32 arithmetic, the host's operation order)."""
    k = torch.as_tensor(np.asarray(w[conv + ".kernel"], np.float32))     # HWIO
    b = torch.as_tensor(np.asarray(w[conv + ".bias"], np.float32))
    if bn is not None:
        g = lambda n: torch.as_tensor(np.asarray(w[bn + "." + n], np.float32))
        s = g("gamma") / torch.sqrt(g("var") + BN_EPS)
        k = k * s
        b = (b - g("mean")) * s + g("beta")
    kh, kw, cin, cout = k.shape
    return k.reshape(kh * kw, cin, cout), b


class _Conv(object):
    """One folded convolution: float64 (exact), and the host's fp32 fold -- its bias, the fp16 pair Whi / Wlo."""

    def __init__(self, w, conv, bn, device):
        k, b = _fold64(w, conv, bn)
        self.w = torch.as_tensor(k, dtype=torch.float64, device=device)
        self.b = torch.as_tensor(b, dtype=torch.float64, device=device)
        w32, b32 = _fold32(w, conv, bn)
        hi = w32.to(torch.float16)
        self.whi = hi.to(device=device, dtype=torch.float64)
        self.wlo = (w32 - hi.float()).to(torch.float16).to(device=device, dtype=torch.float64)   # w32 - hi: exact in fp32
        self.b32 = b32.to(device=device, dtype=torch.float64)


class TrunkWeights(object):
    """The folded, rounded weights of a Keras-layout dict, on ``device``."""

    def __init__(self, w, device="cpu"):
        self.blocks, self.filters = int(w["meta.blocks"]), int(w["meta.filters"])
        self.device = torch.device(device)
        self.stem = _Conv(w, "stem", None, device)
        self.conv1, self.conv2 = [], []
        for i in range(self.blocks):
            self.conv1.append(_Conv(w, "block%d.conv1" % i, "block%d.bn1" % i, device))
            self.conv2.append(_Conv(w, "block%d.conv2" % i, "block%d.bn2" % i, device))
        kp, bp = _fold32(w, "policy.conv", "policy.bn")                    # [1][F][2]
        kv, bv = _fold32(w, "value.conv", "value.bn")                      # [1][F][1]
        self.head_w = torch.cat([kp[0], kv[0]], dim=1).to(device=device, dtype=torch.float64)   # [F][3], the kernel's fp32
        self.head_b = torch.cat([bp, bv]).to(device=device, dtype=torch.float64)


def prepare(w, device="cpu"):
    return TrunkWeights(w, device)


def _f16(x):
    return x.to(torch.float16).to(torch.float64)


def split(x):
    """(hi, lo) = (fp16(x), fp16(x - hi)) as float64."""
    hi = _f16(x)
    return hi, _f16(x - hi)


def _conv3(x, k):
    """'same' 3x3 convolution, x [B,8,8,Cin], k [9][Cin][F] -> [B,8,8,F]: nine shifted matmuls, zero borders."""
    b, cin = x.shape[0], x.shape[-1]
    xp = torch.zeros((b, 10, 10, cin), dtype=torch.float64, device=x.device)
    xp[:, 1:9, 1:9] = x
    acc = None
    for t in range(9):
        ky, kx = divmod(t, 3)
        part = xp[:, ky:ky + 8, kx:kx + 8, :].reshape(b * 64, cin) @ k[t]
        acc = part if acc is None else acc + part
    return acc.reshape(b, 8, 8, k.shape[-1])


def _apply(c, x, mode, drop=None):
    """bias + the products of convolution `c` on block input x in `mode` (the accumulator before the epilogue)."""
    if mode == "exact":
        return _conv3(x, c.w) + c.b
    if mode == "f16":
        return _conv3(_f16(x), c.whi) + c.b32
    hi, lo = split(x)
    if drop == "lo_whi":
        acc = _conv3(hi, c.whi)
    else:
        acc = _conv3(hi + lo, c.whi)                  # hi*Whi + lo*Whi (exact in float64 up to 2^-53)
    if drop != "hi_wlo":
        acc = acc + _conv3(hi, c.wlo)
    return acc + c.b32


def _check(mode, skip, drop):
    if mode not in MODES or skip not in SKIPS or drop not in DROPS or (drop is not None and mode != "f16x3"):
        raise ValueError("mode %r, skip %r, drop %r" % (mode, skip, drop))


def _planes(P, planes):
    x = torch.as_tensor(planes)[..., :IN_PLANES]
    return x.to(device=P.device, dtype=torch.float64)


def stem(P, planes, mode="exact", drop=None):
    """Stem output from planes [B,8,8,>=127] (0/1): linear, the start of the skip stream."""
    _check(mode, "fp32", drop)
    return _apply(P.stem, _planes(P, planes), mode, drop)


def block(P, i, x, mode="exact", skip="fp32", drop=None, mid=False):
    """Residual block ``i`` on the fp32 block input ``x`` [B,8,8,F] (any float dtype): X_{i+1} as float64;
    with ``mid`` also conv1's output as the next convolution consumes it (fp16-rounded in "f16")."""
    _check(mode, skip, drop)
    x = torch.as_tensor(x).to(device=P.device, dtype=torch.float64)
    y = torch.relu(_apply(P.conv1[i], x, mode, drop))
    if mode == "f16":
        y = _f16(y)
    s = x
    if mode == "f16x3" and skip == "hilo":
        hi, lo = split(x)
        s = hi + lo
    out = torch.relu(_apply(P.conv2[i], y, mode, drop) + s)
    return (out, y) if mid else out


def trunk(P, planes, mode="exact", skip="fp32", drop=None, n_blocks=None, every=False):
    """X_{n_blocks} (default: all blocks) from the planes; with ``every`` the list [X_0 = stem, X_1, ...]."""
    xs = [stem(P, planes, mode, drop)]
    for i in range(P.blocks if n_blocks is None else n_blocks):
        xs.append(block(P, i, xs[-1], mode, skip, drop))
    return xs if every else xs[-1]


def heads(P, x):
    """[B,192] ReLU of the three folded 1x1 head convolutions over the trunk output x [B,8,8,F]:
    [0,128) policy at position*2 + k, [128,192) value at 128 + position."""
    x = torch.as_tensor(x).to(device=P.device, dtype=torch.float64)
    b = x.shape[0]
    h = torch.relu(x.reshape(b, 64, -1) @ P.head_w + P.head_b)           # [B][64][3]
    return torch.cat([h[..., :2].reshape(b, 128), h[..., 2]], dim=1)


def heads_condition(P, x):
    """[B,192] sum of |terms| of each head output (|x| . |W| + |b|): the scale of its fp32 rounding error."""
    x = torch.as_tensor(x).to(device=P.device, dtype=torch.float64).abs()
    b = x.shape[0]
    h = x.reshape(b, 64, -1) @ P.head_w.abs() + P.head_b.abs()
    return torch.cat([h[..., :2].reshape(b, 128), h[..., 2]], dim=1)


def scale_magnitude(w, s):
    """A copy of the Keras-layout dict whose every activation is ``s`` times the original's: the trunk is
    positively homogeneous, so scaling the stem kernel and every bias term (conv biases, BN mean and beta)
    by s scales the stem output, every block and every head convolution by s."""
    out = dict(w)
    out["stem.kernel"] = (np.asarray(w["stem.kernel"], np.float64) * s).astype(np.float32)
    for name in w:
        if name.endswith((".bias", ".mean", ".beta")) and "dense" not in name:
            out[name] = (np.asarray(w[name], np.float64) * s).astype(np.float32)
    return out
