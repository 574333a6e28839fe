"""Weight images of the HIP tower: Keras-layout weight dict in, CPU tensors out (pure functions, no device).

These images are the contract with csrc/tower_x16.hpp, csrc/tower_layer.hpp and csrc/heads.hpp
(include/chessrl_hip.h documents them); ``ChessModel`` only moves them to the device.  The float64 references the
kernels are tested against fold and lay out the weights with code of their own, so a bug here is not shared.
"""
import numpy as np
import torch

BN_EPS = 1e-3            # keras.layers.BatchNormalization default
N_POLICY = 1968
PAD_PLANES = 128

# what pack_weights returns, in order: ChessModel keeps each under this attribute name
NAMES = ("_wtiles", "_wtiles3", "_wbias", "_head_w", "_head_b", "_pol_wp", "_pol_bias", "_val_w1p", "_val_b1", "_val_w2")


def _f32(w, name):
    return torch.from_numpy(np.asarray(w[name], np.float32))


def fold(w, conv, bn=None):
    """(OIHW fp32 kernel, bias) of `conv` with the following BatchNorm folded in."""
    k = _f32(w, conv + ".kernel").permute(3, 2, 0, 1).contiguous()
    b = _f32(w, conv + ".bias").clone()
    if bn is not None:
        s = _f32(w, bn + ".gamma") / torch.sqrt(_f32(w, bn + ".var") + BN_EPS)
        k = k * s.view(-1, 1, 1, 1)
        b = (b - _f32(w, bn + ".mean")) * s + _f32(w, bn + ".beta")
    return k, b


def plane_order(F_):
    """(row -> output channel, row -> chunk swizzle) of a weight plane as the trunk kernel keeps
    it in LDS (csrc/tower_x16.hpp: Geo16::row_channel, wswz)."""
    rows = np.arange(F_)
    ct, i = (rows >> 4) & 1, rows & 15
    chan = (rows & ~31) + 8 * (i >> 2) + 4 * ct + (i & 3)
    return chan, (-(rows >> 2)) & 3


def pack_trunk(w, blocks, filters, want_f16=True, want_x3=True):
    """BN-folded fp16 kernels as the planes the fused trunk consumes, in consumption order
    [conv][tap=ky*3+kx][in-ch/32][F rows][4 chunks][8 in]: row r holds output channel
    plane_order(F)[0][r], its four 16-byte chunks (8 input channels each) sit at position
    chunk ^ swizzle(r) -- byte for byte the image the kernel wants in LDS, so its weight DMA
    copies contiguous blocks.  Returns (f16 image, split image, biases f32 [conv][F]); an image
    that was not asked for is an 8-element placeholder."""
    F_ = filters
    chan, swz = plane_order(F_)
    chan_t = torch.from_numpy(chan)
    src_chunk = torch.from_numpy(np.arange(4)[None, :] ^ swz[:, None])        # [row][phys] -> chunk
    names = [("stem", None)]
    for i in range(blocks):
        names += [("block%d.conv1" % i, "block%d.bn1" % i), ("block%d.conv2" % i, "block%d.bn2" % i)]
    tiles, tiles3, biases = [], [], []

    def planes_of(k16):
        """fp16 OIHW kernel -> [tap][in-ch/32][row][chunk][8] in the LDS image's order."""
        cin = k16.shape[1]                                 # 128 for the stem, F otherwise
        t = k16.permute(2, 3, 0, 1).reshape(9, F_, cin // 32, 4, 8)                  # [tap][o][g][chunk][8]
        t = t[:, chan_t]                                                              # rows in plane order
        t = t.permute(0, 2, 1, 3, 4)                                                  # [tap][g][row][chunk][8]
        idx = src_chunk.view(1, 1, F_, 4, 1).expand(9, cin // 32, F_, 4, 8)
        return torch.gather(t, 3, idx)                                                # chunk ^ swizzle(row)

    for conv, bn in names:
        k, b = fold(w, conv, bn)                           # OIHW fp32
        if conv == "stem" and k.shape[1] < PAD_PLANES:    # 127 planes -> 128 channels
            kp = torch.zeros(k.shape[0], PAD_PLANES, 3, 3)
            kp[:, :k.shape[1]] = k
            k = kp
        hi = k.to(torch.float16)
        t_hi = planes_of(hi)
        if want_f16:
            tiles.append(t_hi.contiguous().reshape(-1))
        if want_x3:
            # CRL_TRUNK_SPLIT: per tap the planes of Whi, then of Wlo = fp16(W - Whi); the kernel
            # uses every Whi plane for hi.Whi and lo.Whi in one pass, the Wlo planes for hi.Wlo
            t_lo = planes_of((k - hi.float()).to(torch.float16))
            if F_ == 256:
                # the layer-wise kernels of csrc/tower_layer.hpp keep a 32-channel K-chunk of the activations in
                # LDS for all nine taps: planes K-CHUNK-major, [g][tap][part][row]...
                tiles3.append(torch.stack([t_hi, t_lo], dim=2).permute(1, 0, 2, 3, 4, 5).contiguous().reshape(-1))
            else:
                tiles3.append(torch.stack([t_hi, t_lo], dim=1).contiguous().reshape(-1))   # [tap][part][g][row]...
        biases.append(b)
    empty = torch.zeros(8, dtype=torch.float16)
    return (torch.cat(tiles) if want_f16 else empty, torch.cat(tiles3) if want_x3 else empty,
            torch.stack(biases).float())


def pack_split(x, tiles, ksteps):
    """fp32 [tiles*16 units][ksteps*32 inputs] -> fp16 (hi, lo) MFMA fragments in the order
    csrc/heads.hpp reads them: [tile][k-step][hi|lo][lane = 16 q + r][8], the lane holding
    x[16 tile + r][32 s + 8 q + e]."""
    hi = x.half()
    lo = (x - hi.float()).half()
    frag = torch.stack([hi, lo])                                         # [2][units][inputs]
    frag = frag.reshape(2, tiles, 16, ksteps, 4, 8)                      # [hl][t][r][s][q][e]
    return frag.permute(1, 3, 0, 4, 2, 5).contiguous().reshape(-1)       # [t][s][hl][q][r][e]


def pack_dense(w):
    """Dense layers of the two heads (model.py:44-48, 56-61) for crl_heads_forward."""
    wp = torch.zeros((2048, 128))
    wp[:N_POLICY] = _f32(w, "policy.dense.kernel").t()
    pb = torch.full((2048,), -1e30)
    pb[:N_POLICY] = _f32(w, "policy.dense.bias")
    w1 = _f32(w, "value.dense1.kernel").t().contiguous()                 # [256][64]
    return (pack_split(wp, 128, 4), pb.float(), pack_split(w1, 16, 2), _f32(w, "value.dense1.bias").clone(),
            torch.cat([_f32(w, "value.dense2.kernel").reshape(-1), _f32(w, "value.dense2.bias").reshape(-1)]))    # w2, b2


def pack_weights(w, blocks, filters, want_f16=True, want_x3=True):
    """Everything the HIP tower reads, as the ten CPU tensors of ``NAMES``: the trunk images and biases,
    the 1x1 head convolutions ([3][F] kernels: 2 policy + 1 value, [3] biases) and the dense layers."""
    kp, bp = fold(w, "policy.conv", "policy.bn")           # [2][F][1][1]
    kv, bv = fold(w, "value.conv", "value.bn")             # [1][F][1][1]
    return (pack_trunk(w, blocks, filters, want_f16, want_x3)
            + (torch.cat([kp.reshape(2, filters), kv.reshape(1, filters)]).float(), torch.cat([bp, bv]).float())
            + pack_dense(w))
