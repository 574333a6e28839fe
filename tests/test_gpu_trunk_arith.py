"""GPU: every fused-trunk kernel against the float64 reference of the arithmetic it claims
(oracle/trunk_reference.py), through the C-ABI (crl_trunk_forward_x) on the model's packed images.

The reference rounds operands exactly where a kernel does (fp16 operands in "f16", hi / lo pairs in "f16x3"),
so what is left is the kernel's fp32 summation order.  The sharp check is LAYER-LOCAL: the kernel runs with
n_blocks = k for k = 0 (the stem; the fused kernels) .. B on the same image, and its X_k is compared with the
reference block applied to the kernel's OWN X_{k-1} -- each block starts from the kernel's exact operand.

Statistics are relative to the layer's max |X| (of the reference): the maximum, and for "f16" also the 99.9th
percentile -- conv1's output is rounded to fp16 inside a block, and a kernel accumulator that differs from the
float64 one in its last fp32 bits legitimately rounds some of those to the neighbouring fp16 value.  Measured, that
is not rare at the block output: ~1 conv1 element in 5000 flips, but each conv2 output sums 576 .. 2304 of them,
so a good share of the outputs carry one flip (2^-11 of one product): "f16" sits at 2e-5 of max |X| at the 99.9th
percentile, "f16x3" (every block input and conv1 output carried to 2^-22) at 1e-6 in the maximum.

Every comparison runs on ALL boards of the batch: every slot of a workgroup (board index mod NB) and the first
and last workgroup are among them.
"""

import numpy as np
import pytest
import torch

from oracle import tower_oracle, trunk_reference as tr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BLOCKS = 3
# Bounds, relative to the layer's max |X|.  Measured on MI355X (max over every cell / input of this file) beside them.
CHAIN_BOUND = {
    # mode: (max, 99.9th percentile)         measured (max, 99.9th percentile)
    "f16": (1.5e-4, 6e-5),                  # 5.5e-5, 2.5e-5
    "f16x3": (3e-6, 3e-6),                  # 1.4e-6, 6.1e-7
}
FULL_BOUND = {        # full depth, kernel against the same-mode emulation from the planes
    "f16": 2e-3,      # 8.6e-4 (20 blocks; 3 blocks: 4.4e-4)
    "f16x3": 5e-6,    # 2.1e-6
}
EXACT_BOUND = {       # full depth, kernel against "exact" (the fp32 net's arithmetic in float64)
    "f16": 4e-3,      # test_gpu_search.py's bound for the fp16 trunk; 1.4e-3 (sharp weights, real positions)
    "f16x3": 2e-5,    # test_gpu_search.py's bound for the split trunk; 4.0e-6
}
HEADS_BOUND = 5e-7    # |kernel - reference| / (|X| . |W| + |b|) of a head output, from the kernel's own X_B; 1.4e-7

# Every k_trunk_x16 instantiation of trunk_forward (csrc/api.hip: CRL_X16(F, NB, PAIR, GROUP, SPLIT)) and the
# layer-wise 256-filter split kernels (NB 2, 4), each in both plane formats.
X16 = [(256, 1, 1, 0, 0), (256, 2, 1, 0, 0), (64, 2, 0, 0, 0), (64, 4, 0, 1, 0), (128, 2, 1, 0, 0), (128, 4, 1, 0, 0),
       (128, 2, 1, 0, 1), (64, 2, 0, 0, 1), (64, 4, 0, 0, 1)]
LAYER_NB = (2, 4)


def _x16_name(f, nb, pair, group, split, bits):
    return "k_trunk_x16<%d, %d, %d, 0, %d, %d, %d, 0>" % (f, nb, bits, pair, group, split)


def _layer_name(nb, bits):
    return "k_layer_conv<8, 1|2|3, 0, %d> (+ k_layer_conv<4, 0, 0, %d>, k_layer_expand<%d, 0, %d>)" % (nb, nb, bits, nb)


# (filters, mode, n_boards, small-batch switch) -> the kernel (as (F, NB, PAIR, GROUP, SPLIT), or ("layer", NB))
CELLS = {
    (64, "f16", 4, 1): (64, 2, 0, 0, 0),
    (64, "f16", 512, 1): (64, 2, 0, 0, 0),
    (64, "f16", 516, 1): (64, 4, 0, 1, 0),
    (64, "f16", 8, 0): (64, 4, 0, 1, 0),
    (128, "f16", 4, 1): (128, 2, 1, 0, 0),
    (128, "f16", 516, 1): (128, 4, 1, 0, 0),
    (128, "f16", 8, 0): (128, 4, 1, 0, 0),
    (256, "f16", 4, 1): (256, 1, 1, 0, 0),
    (256, "f16", 256, 1): (256, 1, 1, 0, 0),
    (256, "f16", 260, 1): (256, 2, 1, 0, 0),
    (256, "f16", 8, 0): (256, 2, 1, 0, 0),
    (64, "f16x3", 4, 1): (64, 2, 0, 0, 1),
    (64, "f16x3", 512, 1): (64, 2, 0, 0, 1),
    (64, "f16x3", 516, 1): (64, 4, 0, 0, 1),
    (64, "f16x3", 8, 0): (64, 4, 0, 0, 1),
    (128, "f16x3", 260, 1): (128, 2, 1, 0, 1),
    (128, "f16x3", 516, 1): (128, 2, 1, 0, 1),
    (256, "f16x3", 4, 1): ("layer", 2),
    (256, "f16x3", 512, 1): ("layer", 2),
    (256, "f16x3", 516, 1): ("layer", 4),
}
MEASURED = {}
_CACHE = {}


def _lib():
    from chessrl_amd import _lib
    return _lib


def _expected_name(kern, bits):
    return _layer_name(kern[1], bits) if kern[0] == "layer" else _x16_name(*kern, bits=bits)


def _kernel_name(filters, n, flags):
    return _lib().trunk_kernel_name(filters, n, flags)


def _SmallBatch(on):
    return _lib().trunk_set_small_batch(on)


def _bits_from_planes(planes):
    """fp16/0-1 planes [B,8,8,128] -> int64 [B,128] plane bitboards (bit sq, spatial index sq ^ 56)."""
    b = planes.shape[0]
    flat = planes.reshape(b, 64, 128).to(torch.int64)
    sq = torch.arange(64, device=planes.device) ^ 56
    w = torch.ones(64, dtype=torch.int64, device=planes.device) << sq
    return (flat * w.view(1, 64, 1)).sum(dim=1)


def _random_planes(n, seed=3):
    rng = np.random.default_rng(seed)
    planes = torch.zeros((n, 8, 8, 128), dtype=torch.float16, device=DEV)
    planes[..., :127] = torch.from_numpy((rng.random((n, 8, 8, 127)) < 0.15).astype(np.float16)).to(DEV)
    return planes


def _weights(filters, kind="random_bn", blocks=BLOCKS):
    key = ("w", filters, kind, blocks)
    if key not in _CACHE:
        if kind == "random_bn":
            w = tower_oracle.init_weights(blocks, filters, seed=11, randomize_bn=True)
        elif kind == "sharp":
            w = tower_oracle.calibrated_weights(blocks, filters, _real_positions()[1][:512], seed=7)
        else:
            raise ValueError(kind)
        _CACHE[key] = w
    return _CACHE[key]


def _model(w, mode):
    from chessrl_amd.model import ChessModel
    m = ChessModel(weights=w, precision=mode)
    assert m.fused and m.precision == mode
    return m


def _real_positions():
    if "real" not in _CACHE:
        from chessrl_amd.model import ChessModel
        from tests.util import encode_prefixes, selfplay_position_prefixes
        prefixes, info = selfplay_position_prefixes(516)
        assert len(prefixes) == 516
        bits, planes = encode_prefixes(ChessModel(blocks=2, filters=64, precision="f16"), prefixes)
        p16 = torch.zeros((516, 8, 8, 128), dtype=torch.float16, device=DEV)
        p16[..., :127] = torch.from_numpy(planes).to(DEV).half()
        assert torch.equal(_bits_from_planes(p16), bits)
        _CACHE["real"] = (bits, planes, p16)
    return _CACHE["real"]


def _run(model, mode, planes, n_blocks, image=None, bias=None):
    """One crl_trunk_forward_x launch: (fp32 trunk [n,8,8,F], head activations [n,192])."""
    L = _lib()
    n, f = planes.shape[0], model.filters
    split = mode == "f16x3"
    image = image if image is not None else (model._wtiles3 if split else model._wtiles)
    bias = bias if bias is not None else model._wbias
    flags = (L.TRUNK_BITPLANES if planes.dtype == torch.int64 else 0) | (L.TRUNK_SPLIT if split else 0)
    out = torch.full((n, 8, 8, f), float("nan"), dtype=torch.float32, device=DEV)
    heads = torch.full((n, 192), float("nan"), dtype=torch.float32, device=DEV)
    ws = model._trunk_workspace(n) if split else None
    L.trunk_forward_x(f, flags, planes, image, bias, out, n, n_blocks, model._head_w, model._head_b, heads, ws,
                      ws.numel() if ws is not None else 0)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(heads).all()
    return out, heads


def _skip(filters, mode):
    return "hilo" if (filters == 256 and mode == "f16x3") else "fp32"


def _stats(kern, ref):
    """(max, 99.9th percentile) of |kern - ref| / max |ref|."""
    d = (kern.double() - ref).abs().flatten()
    m = max(ref.abs().max().item(), 1e-300)
    k = max(1, int(np.ceil(0.999 * d.numel())))
    return d.max().item() / m, d.kthvalue(k).values.item() / m


def _within(stat, mode, bound=None):
    mx, p = stat
    bmax, bp = bound or CHAIN_BOUND[mode]
    return mx <= bmax and (mode != "f16" or p <= bp)


def _record(key, value):
    MEASURED[key] = value
    print("%s: %s" % (key, value))


def _chain(model, P, mode, planes16, bits, n_blocks):
    """Layer-local chain: [(k, (max, p99.9)) per k], the kernel's X_{B-1}, X_B and heads of the n_blocks = B run.
    Both plane formats run; they must give the same bits."""
    f = model.filters
    skip = _skip(f, mode)
    layer = f == 256 and mode == "f16x3"
    rows, prev, last = [], None, None
    for k in range(1 if layer else 0, n_blocks + 1):
        xk, hk = _run(model, mode, bits, k)
        xk16, hk16 = _run(model, mode, planes16, k)
        assert torch.equal(xk, xk16) and torch.equal(hk, hk16), "the two plane formats differ at n_blocks=%d" % k
        if k == 0:
            ref = tr.stem(P, planes16, mode)
        elif prev is None:                            # layer-wise: no stem-only launch; stem + block 0 from the planes
            ref = tr.block(P, 0, tr.stem(P, planes16, mode), mode, skip)
        else:
            ref = tr.block(P, k - 1, prev, mode, skip)
        rows.append((k, _stats(xk, ref)))
        last, prev = prev, xk
        heads = hk
    return rows, last, prev, heads


def _heads_error(P, x, heads):
    ref = tr.heads(P, x)
    cond = tr.heads_condition(P, x)
    return ((heads.double() - ref).abs() / cond.clamp(min=1e-30)).max().item()


def _check_cell(model, P, mode, planes16, bits, label, n_blocks=BLOCKS, chain_bound=None, full_bound=None):
    rows, _, xb, heads = _chain(model, P, mode, planes16, bits, n_blocks)
    worst = (max(s[0] for _, s in rows), max(s[1] for _, s in rows))
    he = _heads_error(P, xb, heads)
    skip = _skip(model.filters, mode)
    full = tr.trunk(P, planes16, mode, skip, n_blocks=n_blocks)
    exact = tr.trunk(P, planes16, "exact", n_blocks=n_blocks)
    fe = _stats(xb, full)[0]
    ee = _stats(xb, exact)[0]
    _record(label, {"chain_max": worst[0], "chain_p999": worst[1], "heads": he, "full_vs_mode": fe,
                    "full_vs_exact": ee, "per_block": [(k, s[0]) for k, s in rows]})
    for k, s in rows:
        assert _within(s, mode, chain_bound), (label, k, s, chain_bound or CHAIN_BOUND[mode])
    assert he <= HEADS_BOUND, (label, he)
    assert fe <= (full_bound or FULL_BOUND[mode]), (label, fe)
    return ee


@pytest.mark.parametrize("bits", [0, 1])
def test_dispatch_table_reaches_every_instantiation(bits):
    L = _lib()
    seen = set()
    for (f, mode, n, small), kern in sorted(CELLS.items(), key=str):
        flags = (L.TRUNK_BITPLANES if bits else 0) | (L.TRUNK_SPLIT if mode == "f16x3" else 0)
        with _SmallBatch(small):
            name = _kernel_name(f, n, flags)
        assert name == _expected_name(kern, bits), ((f, mode, n, small), name)
        seen.add(name)
    every = {_x16_name(*k, bits=bits) for k in X16} | {_layer_name(nb, bits) for nb in LAYER_NB}
    assert seen == every, sorted(every - seen)


@pytest.mark.parametrize("cell", sorted(CELLS, key=str), ids=lambda c: "%d-%s-%d-small%d" % c)
def test_layer_local_chain_heads_and_full_depth_per_dispatch_cell(cell):
    f, mode, n, small = cell
    w = _weights(f)
    P = tr.prepare(w, DEV)
    model = _model(w, mode)
    planes16 = _random_planes(n)
    with _SmallBatch(small):
        assert _kernel_name(f, n, _lib().TRUNK_BITPLANES | (_lib().TRUNK_SPLIT if mode == "f16x3" else 0)) == \
            _expected_name(CELLS[cell], 1)
        ee = _check_cell(model, P, mode, planes16, _bits_from_planes(planes16), "cell %s" % (cell,))
    assert ee <= EXACT_BOUND[mode], (cell, ee)


@pytest.mark.parametrize("mode", ["f16", "f16x3"])
@pytest.mark.parametrize("filters", [64, 128, 256])
def test_twenty_block_chain_runs_every_convolution_slot(filters, mode):
    """20 blocks = 41 convolutions (crl_tower::MAX_CONVS): the chain over every block of the deepest tower."""
    w = tower_oracle.init_weights(20, filters, seed=13, randomize_bn=True)
    P = tr.prepare(w, DEV)
    model = _model(w, mode)
    planes16 = _random_planes(8, seed=20)
    ee = _check_cell(model, P, mode, planes16, _bits_from_planes(planes16), "20 blocks %d %s" % (filters, mode),
                     n_blocks=20)
    _record("20 blocks %d %s full_vs_exact" % (filters, mode), ee)


@pytest.mark.parametrize("weights", ["random_bn", "sharp"])
@pytest.mark.parametrize("mode", ["f16", "f16x3"])
@pytest.mark.parametrize("filters", [64, 128, 256])
def test_real_positions(filters, mode, weights):
    """Self-play positions (openings to long endgames) at 260 boards, on randomised-BN and on sharp (calibrated) weights."""
    bits, _, planes16 = _real_positions()
    w = _weights(filters, weights)
    P = tr.prepare(w, DEV)
    model = _model(w, mode)
    ee = _check_cell(model, P, mode, planes16[:260].contiguous(), bits[:260].contiguous(),
                     "real %d %s %s" % (filters, mode, weights))
    assert ee <= EXACT_BOUND[mode], ee


def _magnitude_scale(w, planes16, target):
    """s such that the largest activation of the scaled net (block outputs and conv1 outputs) is ``target``."""
    P = tr.prepare(w, DEV)
    x = tr.stem(P, planes16)
    m = x.abs().max().item()
    for i in range(P.blocks):
        x, y = tr.block(P, i, x, mid=True)
        m = max(m, x.abs().max().item(), y.abs().max().item())
    return target / m


# The magnitude edges.  Activations up to 1e-3 put lo, and hi itself below 2^-14, in fp16 subnormals: the split format
# holds 2^-25 absolute there, not 2^-22 relative.  The kernel keeps the subnormals (the chain holds: with lo flushed,
# lo*Whi would be lost, 2^-12 relative), but the format's own rounding now reaches the bounds: conv1's output and, over
# the full depth, every activation the kernel's fp32 and the reference's float64 accumulators round to neighbouring
# subnormals.  (chain max, chain p99.9), full depth vs the emulation, vs exact:
EDGE_BOUND = {
    1e-3: ((4e-5, 4e-5), 5e-4, 5e-3),
    1e4: (None, None, EXACT_BOUND["f16x3"]),
}


@pytest.mark.parametrize("target", [1e-3, 1e4])
@pytest.mark.parametrize("filters", [64, 128, 256])
def test_split_magnitude_edges(filters, target):
    """f16x3 on a net scaled so that its largest activation is ~1e-3 (lo, and the smaller activations' hi, in fp16
    subnormals) or ~1e4: against the same-mode emulation at the ordinary bounds."""
    planes16 = _random_planes(8, seed=30)
    w0 = _weights(filters)
    w = tr.scale_magnitude(w0, _magnitude_scale(w0, planes16, target))
    P = tr.prepare(w, DEV)
    model = _model(w, "f16x3")
    chain, full, exact = EDGE_BOUND[target]
    ee = _check_cell(model, P, "f16x3", planes16, _bits_from_planes(planes16), "edge %d %g" % (filters, target),
                     chain_bound=chain, full_bound=full)
    assert ee <= exact, ee


def _image_offset(filters, mode, tap, cin, cout):
    """Offset of Whi[tap][cin][cout] within one convolution of the weight image (include/chessrl_hip.h): planes of
    [filters rows][4 chunks][8 in], row r holding output channel (r & ~31) + 8*((r & 15) >> 2) + 4*((r >> 4) & 1) + (r & 3)
    and the chunk of input channels 8c .. 8c+7 at position c ^ ((-(r >> 2)) & 3); planes ordered [tap][in/32] ("f16"),
    [tap][Whi, Wlo][in/32] (split, 64 / 128 filters) or [in/32][tap][Whi, Wlo] (split, 256 filters: layer-wise)."""
    rows = np.arange(filters)
    chan = (rows & ~31) + 8 * ((rows & 15) >> 2) + 4 * ((rows >> 4) & 1) + (rows & 3)
    r = int(np.nonzero(chan == cout)[0][0])
    g, c, e = cin // 32, (cin % 32) // 8, cin % 8
    plane = {"f16": tap * (filters // 32) + g}.get(mode)
    if plane is None:
        plane = (g * 9 + tap) * 2 if filters == 256 else tap * 2 * (filters // 32) + g
    return plane * filters * 32 + r * 32 + (c ^ ((-(r >> 2)) & 3)) * 8 + e


@pytest.mark.parametrize("mode", ["f16", "f16x3"])
@pytest.mark.parametrize("filters", [64, 128, 256])
def test_negative_controls_fail_the_bounds(filters, mode):
    w = _weights(filters)
    P = tr.prepare(w, DEV)
    model = _model(w, mode)
    planes16 = _random_planes(8, seed=40)
    skip = _skip(filters, mode)
    rows, x_prev, x_last, _ = _chain(model, P, mode, planes16, planes16, BLOCKS)
    ref = tr.block(P, BLOCKS - 1, x_prev, mode, skip)
    assert _within(_stats(x_last, ref), mode)
    found = {}
    # one fp16 element of the last convolution's weights scaled by 1.01: the centre tap's Whi of the input channel
    # that is largest anywhere (conv1's output of the last block) to the output channel it weighs most
    _, y = tr.block(P, BLOCKS - 1, x_prev, mode, skip, mid=True)
    c = P.conv2[BLOCKS - 1]
    i = int(y.reshape(-1, filters).max(0).values.argmax())
    o = int(c.whi[4, i].abs().argmax())
    image = (model._wtiles3 if mode == "f16x3" else model._wtiles).clone()
    j = _image_offset(filters, mode, 4, i, o)
    seg = image[-9 * filters * filters * (2 if mode == "f16x3" else 1):]
    assert seg[j].double() == c.whi[4, i, o]                     # (the documented image layout finds that weight)
    seg[j] = (seg[j].float() * 1.01).half()
    xw, _ = _run(model, mode, planes16, BLOCKS, image=image)
    found["weight x1.01"] = _stats(xw, ref)
    # one bias entry of the last convolution shifted by 1e-3 of the layer's max |X|, in its most active channel
    bias = model._wbias.clone()
    c = int(x_last.reshape(-1, filters).max(0).values.argmax())
    bias[2 * BLOCKS, c] += 1e-3 * ref.abs().max().item()
    xb, _ = _run(model, mode, planes16, BLOCKS, bias=bias)
    found["bias +1e-3"] = _stats(xb, ref)
    if mode == "f16x3":
        # a reference without one of the three products, against the unmodified kernel
        for drop in ("lo_whi", "hi_wlo"):
            found["drop " + drop] = _stats(x_last, tr.block(P, BLOCKS - 1, x_prev, mode, skip, drop=drop))
    _record("controls %d %s" % (filters, mode), found)
    for name, s in found.items():
        assert not _within(s, mode), (name, s, CHAIN_BOUND[mode])


@pytest.mark.parametrize("mode", ["f16", "f16x3"])
@pytest.mark.parametrize("filters", [64, 128, 256])
def test_geometry_identity_every_batch_and_boards_per_workgroup(filters, mode):
    """A board's trunk output has the same bits at every boards-per-workgroup and batch size (and both plane
    formats); head activations the same bits where the channel groups of the head reduction are the same
    (64 filters at NB 2 vs NB 4 reduce over a different count: a tight bound there)."""
    w = _weights(filters)
    P = tr.prepare(w, DEV)
    model = _model(w, mode)
    planes16 = _random_planes(516, seed=50)
    bits = _bits_from_planes(planes16)
    base, hbase = _run(model, mode, bits, BLOCKS)
    flags = _lib().TRUNK_BITPLANES | (_lib().TRUNK_SPLIT if mode == "f16x3" else 0)
    base_name = _kernel_name(filters, 516, flags)
    report = {}
    for n, small in ((4, 1), (8, 0), (8, 1), (256, 1), (260, 1), (512, 1)):
        with _SmallBatch(small):
            name = _kernel_name(filters, n, flags)
            x, h = _run(model, mode, bits[:n].contiguous(), BLOCKS)
            x16, h16 = _run(model, mode, planes16[:n].contiguous(), BLOCKS)
        assert torch.equal(x, x16) and torch.equal(h, h16)
        same_heads = torch.equal(h, hbase[:n])
        hd = ((h.double() - hbase[:n].double()).abs() / tr.heads_condition(P, base[:n]).clamp(min=1e-30)).max().item()
        report[(n, small)] = (name, torch.equal(x, base[:n]), same_heads, hd)
        assert torch.equal(x, base[:n]), (n, small, name, base_name)
        if filters == 64 and name.split(",")[1] != base_name.split(",")[1]:
            assert hd <= HEADS_BOUND, (n, small, hd)
        else:
            assert same_heads, (n, small, name, base_name, hd)
    _record("geometry %d %s (vs %s)" % (filters, mode, base_name), report)


def test_zz_print_measured():
    """(runs last: the measured values of this file, for the bounds above)"""
    for k in sorted(MEASURED, key=str):
        print("MEASURED %s: %s" % (k, MEASURED[k]))
