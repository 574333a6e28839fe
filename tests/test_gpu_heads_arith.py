"""GPU: the dense-head kernels (chessrl_amd/csrc/heads.hpp, slices.hpp) against the float64 reference of the arithmetic
they claim to perform (oracle/heads_reference.py), through the C-ABI (crl_heads_forward, crl_heads_forward_legal,
crl_heads_forward_legal_raw) on the model's packed images.  The head activations are fed directly as [n][192] fp32.

The reference rounds operands exactly where the kernels do (hi / lo fp16 pairs of weights and activations), so what is
left is the kernels' fp32 summation order and their exp / tanh.  The sharp checks are KERNEL-LOCAL:

* logits: crl_heads_forward_legal_raw leaves raw logits at the listed labels.  Every activation row is repeated 8 times,
  copy k listing the labels of slice k (256 k .. min(256 k + 255, 1967), permuted), so all 1968 logits of every row are
  visible; they are compared with ``logits(P, act, "split")`` relative to |x|.|W| + |b|, over ALL labels and boards.
* slice statistics: m is the maximum of the kernel's own logits bit for bit, s against the float64 sum over them.
* probabilities: against ``prob_from_stats`` (slices.hpp in float64) applied to the kernel's OWN logits and statistics,
  relative, as a function of the depth M - l below the board's maximum.

End to end the two forms (one-pass k_policy_head, sliced k_heads_sliced + k_policy_normalise) are compared with the
float64 softmax of the "split" and "exact" logits: |p / p_ref - 1| relative to (1 + depth + board's largest condition)
-- a logit error e moves a probability by the factor exp(e), the exp's argument is rounded at depth x 2^-24.

Weight sets (tests/heads_util.py): flat (Keras-initialised, logit spread ~6), peaked (spread >= 40 per board), huge
(>= 200: most labels underflow), spread-value (z over -12.5 .. 12.5); activation sets |N(0, 1.5)| with every 7th column
zero, the same at ~1e-3 (lo in fp16 subnormals) and at ~1e3.

The probability tests record the relative error per bin of 10 in depth (test_zz_print_measured prints it); what slope
to expect from __expf, and what an exp with a higher-precision argument reduction would give, stands at PROB_BOUND.
"""

import numpy as np
import pytest
import torch

from oracle import heads_reference as hr
from tests import heads_util as hu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -7.0                   # guard value of every output buffer
TINY = 1e-37                  # relative measures run on probabilities the reference puts above this (fp32 normal range)

# Bounds on |kernel - float64 reference|: about 3x the maximum measured on MI355X over every case of this file (beside
# each bound), the margin of test_gpu_trunk_arith.py.  u = 2^-24, the fp32 unit roundoff.
U = 2.0 ** -24
# a logit: the bias and 12 MFMAs chained through the fp32 accumulator (4 k-steps x 3 products).  Were every MFMA one
# rounding to nearest of an exact 32-product block, 12 u = 7.2e-7 would be the worst case; "flat-tiny" (the accumulator
# is the bias, every block far smaller) measures 16 u: the instruction loses up to an ulp per accumulation, not half.
LOGIT_BOUND = 3e-6            # / (|x|.|W| + |b|), every label of every board; 9.7e-7 (flat-tiny), 2.4e-7 (all others)
SUM_BOUND = 8e-7              # slice sum, relative, against the float64 sum over the kernel's own logits; 2.6e-7
# a probability exp(l - M) / S against prob_from_stats on the kernel's own logits / statistics, relative: a + b x depth.
# This one is the worst case of the format, not 3x a measurement (exp is a fixed function of its argument, no summation
# order is involved), and it holds: __expf(x) is exp2(x * log2 e); l - M rounds once (u |x|), the product with the
# rounded constant once more (1.5 u |x| in the exponent): b = 2.5 u per unit of depth.  a: exp2 (2 u), S (8 products with
# an exp each, summed), 1 / S and the final product: 36 u.  Measured, max per depth bin 0, 10, .. 80: 6.0e-7, 2.0e-6,
# 2.7e-6, 3.8e-6, 5.1e-6, 5.3e-6, 7.3e-6, 7.5e-6, 7.6e-6 -- a slope of 1.0e-7 per unit (1.7 u), at most 0.61 of the bound.
# An exp that reduced its argument in higher precision would keep the subtraction's 1 u = 6e-8 per unit only.
# At depth 20 - 40 that is <= 5e-6 RELATIVE, of probabilities below 2e-9: no prior moves anywhere near the 1e-4 bar.
PROB_BOUND = (36 * U, 2.5 * U)  # (2.1e-6, 1.5e-7 per unit of depth)
# end to end against the softmax of the reference logits, relative to (1 + depth + the board's largest condition)
E2E_BOUND = {"split": 8e-7,   # 2.6e-7
             "exact": 1e-6}   # 3.1e-7
ROWSUM_BOUND = 1.5e-6         # |sum_labels p - 1| (float64 sum of the fp32 outputs); 4.4e-7
VALUE_BOUND = 1e-7            # |v - ref| / (1 + (1 - ref^2) x condition of z); 3.0e-8 (|v - ref| itself: 3.9e-7 flat,
                              # 2.7e-6 spread-value, 1.1e-4 at activations of 1e3, where z's condition is ~1e3)
TANH_BOUND = 6e-8             # |v - tanh(z)| for z exact in fp32 (the one-hot probe); 1.9e-8

CASES = [("flat", "base"), ("flat", "tiny"), ("flat", "big"), ("peaked", "base"), ("huge", "base")]
NO_EXCLUSION = {("flat", "base"), ("flat", "tiny"), ("peaked", "base")}     # nothing below TINY there
MEASURED = {}
_CACHE = {}


def _lib():
    from chessrl_amd import _lib
    return _lib


def _record(key, value):
    MEASURED[key] = value
    print("%s: %s" % (key, value))


def _weights(kind):
    key = ("w", kind)
    if key not in _CACHE:
        flat = hu.flat_weights()
        rows = hu.activations(hu.ROWS, "base")
        if kind == "flat":
            w = flat
        elif kind == "peaked":
            w = hu.scaled_policy(flat, rows, hu.PEAKED_SPREAD)
        elif kind == "huge":
            w = hu.scaled_policy(flat, rows, hu.HUGE_SPREAD)
        elif kind == "value":
            w = hu.spread_value(flat, _value_rows())
        elif kind == "zero":                                  # zero policy kernel and bias: a uniform policy
            w = dict(flat)
            w["policy.dense.kernel"] = np.zeros((128, 1968), np.float32)
            w["policy.dense.bias"] = np.zeros(1968, np.float32)
        elif kind == "nobias":                                # for the one-hot probes
            w = dict(flat)
            w["policy.dense.bias"] = np.zeros(1968, np.float32)
            w["value.dense1.bias"] = np.zeros(256, np.float32)
        else:
            raise ValueError(kind)
        _CACHE[key] = w
    return _CACHE[key]


def _value_rows():
    return hu.activations(1000, "base", seed=9)


def _case(kind):
    """(weights, reference weights on the device, model) of a weight set; built once."""
    key = ("case", kind)
    if key not in _CACHE:
        from chessrl_amd.model import ChessModel
        w = _weights(kind)
        m = ChessModel(weights=w, precision="f16")            # an explicit precision: no probe runs
        assert m.fused and m.precision == "f16"
        _CACHE[key] = (w, hr.prepare(w, DEV), m)
    return _CACHE[key]


def _acts(kind, n=hu.ROWS, seed=5):
    return torch.from_numpy(hu.activations(n, kind, seed)).to(DEV)


def _call(model, kind, act, n, scratch, labels=None, counts=None, value=True, image=None, bias=None, guard=3):
    """One C-ABI call on the first n rows of act.  kind: "full" | "legal" | "raw".  Every output buffer carries
    ``guard`` rows behind the batch that must stay untouched.  Returns (policy / priors [n][...], value [n] or
    None, scratch [n][16] or None)."""
    L = _lib()
    assert act.dtype == torch.float32 and act.is_contiguous() and act.shape[0] >= n and act.shape[1] == 192
    pol = torch.full((n + guard, 1968 if kind == "full" else 256), SENT, device=DEV)
    val = torch.full((n + guard,), SENT, device=DEV) if value else None
    st = torch.full((n + guard, 16), SENT, device=DEV) if scratch else None
    image = model._pol_wp if image is None else image
    bias = model._pol_bias if bias is None else bias
    common = (act, n, image, bias, model._val_w1p, model._val_b1, model._val_w2)
    if kind == "full":
        L.heads_forward(*common, pol, val, st)
    else:
        assert labels.dtype == torch.int16 and labels.shape[0] >= n and labels.shape[1] == 256
        assert counts.dtype == torch.int32 and counts.shape[0] >= n
        fn = L.heads_forward_legal if kind == "legal" else L.heads_forward_legal_raw
        fn(*common, labels, counts, pol, val, st)
    torch.cuda.synchronize()
    assert (pol[n:] == SENT).all(), "policy rows behind the batch were written"
    assert val is None or (val[n:] == SENT).all(), "values behind the batch were written"
    assert st is None or (st[n:] == SENT).all(), "statistics behind the batch were written"
    return pol[:n], (val[:n] if value else None), (st[:n] if scratch else None)


def _sliced(st):
    """Whether the call ran in the sliced form: it then wrote the statistics of every board."""
    touched = st != SENT
    assert bool(touched.all()) or not bool(touched.any())
    return bool(touched.all())


def _SlicedMax(boards):
    return _lib().heads_set_sliced_max(boards)


def _windows(rows, seed=1):
    """labels int16 [8 rows][256], counts int32 [8 rows]: board 8 i + k lists the labels of slice k, permuted."""
    rng = np.random.default_rng(seed)
    labels = np.zeros((rows * 8, 256), np.uint16)
    counts = np.zeros(rows * 8, np.int32)
    for k in range(8):
        cnt = min(256 * k + 256, 1968) - 256 * k
        base = np.tile(np.arange(256 * k, 256 * k + cnt, dtype=np.uint16), (rows, 1))
        labels[k::8, :cnt] = rng.permuted(base, axis=1)
        counts[k::8] = cnt
    assert sorted(set(counts)) == [176, 256]
    return torch.from_numpy(labels.view(np.int16)).to(DEV), torch.from_numpy(counts).to(DEV)


def _from_windows(pri, labels, counts, rows):
    """[rows][1968] from the window boards' rows; slots past a count must be untouched."""
    full = torch.full((rows, 2048), float("nan"), device=DEV)
    for k in range(8):
        cnt = int(counts[k])
        idx = (labels[k::8, :cnt].to(torch.int64) & 0xFFFF)
        full.scatter_(1, idx, pri[k::8, :cnt])
        assert (pri[k::8, cnt:] == SENT).all(), "written past the count"
    assert not torch.isnan(full[:, :1968]).any() and torch.isnan(full[:, 1968:]).all()
    return full[:, :1968].contiguous()


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _local(case):
    """The kernel-local run of a case: the kernel's own raw logits [rows][1968], statistics [rows][8][2] and values
    from crl_heads_forward_legal_raw over the 8 label windows of every activation row."""
    key = ("local", case)
    if key not in _CACHE:
        wk, ak = case
        w, P, model = _case(wk)
        act = _acts(ak)
        rows = act.shape[0]
        rep = act.repeat_interleave(8, 0).contiguous()
        labels, counts = _windows(rows)
        pri, val, st = _call(model, "raw", rep, rows * 8, True, labels, counts)
        assert _sliced(st)
        lg = _from_windows(pri, labels, counts, rows)
        _CACHE[key] = dict(w=w, P=P, model=model, act=act, rep=rep, labels=labels, counts=counts, rows=rows,
                           logits=lg, stats_all=st.reshape(rows, 8, 16), stats=st.reshape(rows, 8, 8, 2)[:, 0].contiguous(),
                           values_all=val.reshape(rows, 8))
    return _CACHE[key]


def _spread(P, act):
    lg = hr.logits(P, act, "split")
    return lg.max(1).values - lg.min(1).values


def _check_preconditions(case, P, act):
    """The named weight sets are what they claim on the activations in use (they cannot silently turn flat)."""
    wk, ak = case
    if ak != "base":
        return
    s = _spread(P, act)
    if wk == "peaked":
        assert s.min().item() >= 40, s.min().item()
        assert s.max().item() + np.log(1968.0) < 85, "peaked must stay within fp32's normal range"
    if wk == "huge":
        assert s.min().item() >= 200, s.min().item()
        p = hr.softmax(hr.logits(P, act, "split"))
        assert (p < TINY).double().mean().item() > 0.5                          # most labels underflow
        assert p.max(1).values.median().item() >= 0.9                           # and the best one takes (nearly) all


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s" % c)
def test_raw_logits_and_slice_statistics_kernel_local(case):
    c = _local(case)
    P, act, lg, st = c["P"], c["act"], c["logits"], c["stats"]
    _check_preconditions(case, P, act)
    if case[1] == "tiny":
        hi, lo = hr.split(act)
        assert ((lo != 0) & (lo.abs() < 2.0 ** -14)).any()                         # lo does sit in fp16 subnormals
    # copies of a row that differ only in their label window: the same statistics and value, bit for bit
    assert torch.equal(_bits(c["stats_all"]), _bits(c["stats_all"][:, :1].expand(-1, 8, -1).contiguous()))
    assert torch.equal(_bits(c["values_all"]), _bits(c["values_all"][:, :1].expand(-1, 8).contiguous()))
    assert torch.isfinite(lg).all() and torch.isfinite(st).all()
    # every logit of every board
    ref, cond = hr.logits(P, act, "split"), hr.logit_condition(P, act)
    err = ((lg.double() - ref).abs() / cond.clamp(min=1e-300)).max().item()
    # m: the maximum of the kernel's own logits of the slice (a maximum is exact); in slice 7 the pad does not win
    own = hr.pad_logits(lg)                                                         # float64 of the fp32 logits
    m_own = own.reshape(-1, 8, 256).max(-1).values
    assert torch.equal(st[..., 0].double(), m_own), "a slice maximum is not the maximum of the slice's logits"
    assert (st[:, 7, 0] > -1e29).all()
    # s: against the float64 sum over the kernel's own logits
    s_ref = hr.slice_stats(lg)[..., 1]
    serr = ((st[..., 1].double() - s_ref).abs() / s_ref).max().item()
    _record("local %s-%s" % case, {"logit": err, "slice_sum": serr, "boards": act.shape[0] * 8, "labels": lg.numel()})
    assert err <= LOGIT_BOUND, err
    assert serr <= SUM_BOUND, serr


def _depth_record(p, p_ref, depth):
    """(max relative error per depth bin of 10 over p_ref >= TINY, excluded count, worst ratio to PROB_BOUND)."""
    live = p_ref >= TINY
    rel = (p.double() / p_ref.clamp(min=1e-300) - 1).abs()
    bins = {}
    b = torch.div(depth, 10, rounding_mode="floor").clamp(max=9).to(torch.int64)
    for k in range(10):
        sel = live & (b == k)
        if sel.any():
            bins[10 * k] = (rel[sel].max().item(), int(sel.sum()))
    ratio = (rel / (PROB_BOUND[0] + PROB_BOUND[1] * depth))[live].max().item()
    return bins, int((~live).sum()), ratio, live


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s" % c)
def test_sliced_probabilities_against_the_formula_on_the_kernels_own_numbers(case):
    c = _local(case)
    model, rows, lg, st = c["model"], c["rows"], c["logits"], c["stats"]
    # the same launch with its normalising pass: FULL rows and LEGAL windows
    full, _, st_full = _call(model, "full", c["rep"], rows * 8, True)
    assert _sliced(st_full)
    assert _same_bits(st_full.reshape(rows, 8, 16), c["stats_all"]), "FULL and LEGAL_RAW leave different statistics"
    assert _same_bits(full.reshape(rows, 8, 1968), full.reshape(rows, 8, 1968)[:, :1].expand(-1, 8, -1).contiguous())
    pri, _, st_leg = _call(model, "legal", c["rep"], rows * 8, True, c["labels"], c["counts"])
    assert _same_bits(st_leg.reshape(rows, 8, 16), c["stats_all"])
    p = full[::8].contiguous()
    assert _same_bits(_from_windows(pri, c["labels"], c["counts"], rows), p), "LEGAL and FULL differ"
    assert torch.isfinite(p).all() and (p >= 0).all()
    p_ref = hr.prob_from_stats(lg, st)
    M = st[..., 0].double().max(1).values
    depth = M.unsqueeze(1) - lg.double()
    assert (depth >= 0).all()
    bins, excluded, ratio, live = _depth_record(p, p_ref, depth)
    _record("prob %s-%s" % case, {"per_depth_bin (max rel, labels)": bins, "excluded_below_1e-37": excluded,
                                  "of": p.numel(), "worst / bound": ratio})
    assert (p[~live] < 1e-36).all()
    if case in NO_EXCLUSION:
        assert excluded == 0
    assert ratio <= 1.0, ratio


def _e2e(p, P, act, mode):
    """max of |p / p_ref - 1| / (1 + depth + the board's largest condition) over p_ref >= TINY; the excluded count."""
    lg = hr.logits(P, act, mode)
    p_ref = hr.softmax(lg)
    depth = lg.max(1, keepdim=True).values - lg
    cond = hr.logit_condition(P, act).max(1, keepdim=True).values
    live = p_ref >= TINY
    assert (p[~live] < 1e-36).all()
    rel = (p.double() / p_ref.clamp(min=1e-300) - 1).abs() / (1 + depth + cond)
    return rel[live].max().item(), int((~live).sum())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s" % c)
def test_probabilities_end_to_end_both_forms(case):
    wk, ak = case
    w, P, model = _case(wk)
    act = _acts(ak, n=100, seed=6)
    n = act.shape[0]
    rng = np.random.default_rng(3)
    labels = np.stack([rng.permutation(1968)[:256] for _ in range(n)]).astype(np.uint16)
    counts = rng.integers(0, 219, n).astype(np.int32)
    lab_d, cnt_d = torch.from_numpy(labels.view(np.int16)).to(DEV), torch.from_numpy(counts).to(DEV)
    out, rec = {}, {}
    for form in ("sliced", "onepass"):
        p, v, st = _call(model, "full", act, n, form == "sliced")
        assert (st is not None and _sliced(st)) == (form == "sliced")
        pri, v2, _ = _call(model, "legal", act, n, form == "sliced", lab_d, cnt_d)
        assert _same_bits(v, v2)
        pc, pric = p.cpu().numpy(), pri.cpu().numpy()
        for b in range(n):                                                  # FULL and LEGAL: the same bits
            assert np.array_equal(pric[b, :counts[b]].view(np.uint32), pc[b, labels[b, :counts[b]]].view(np.uint32)), b
            assert (pric[b, counts[b]:] == SENT).all()
        assert torch.isfinite(p).all() and (p >= 0).all() and (p <= 1).all()
        rec[form] = {"split": _e2e(p, P, act, "split"), "exact": _e2e(p, P, act, "exact"),
                     "rowsum": (p.double().sum(1) - 1).abs().max().item()}
        out[form] = p
    # one-pass against sliced: another summation order, the same bound
    lg = hr.logits(P, act, "split")
    p_ref = hr.softmax(lg)
    live = p_ref >= TINY
    scale = 1 + (lg.max(1, keepdim=True).values - lg) + hr.logit_condition(P, act).max(1, keepdim=True).values
    rec["onepass_vs_sliced"] = (((out["onepass"].double() - out["sliced"].double()).abs() / p_ref.clamp(min=1e-300)) / scale)[live].max().item()
    _record("e2e %s-%s" % case, rec)
    for form in ("sliced", "onepass"):
        for mode in ("split", "exact"):
            assert rec[form][mode][0] <= E2E_BOUND[mode], (form, mode, rec[form][mode])
            if case in NO_EXCLUSION:
                assert rec[form][mode][1] == 0
        assert rec[form]["rowsum"] <= ROWSUM_BOUND, (form, rec[form]["rowsum"])
    assert rec["onepass_vs_sliced"] <= E2E_BOUND["split"]


def _value_error(v, P, act, drop=None):
    ref = hr.value(P, act, "split", drop)
    return ((v.double() - ref).abs() / (1 + (1 - ref * ref) * hr.value_condition(P, act))).max().item()


@pytest.mark.parametrize("case", [("flat", "base"), ("flat", "tiny"), ("flat", "big"), ("value", "base")],
                         ids=lambda c: "%s-%s" % c)
def test_value_head_from_every_launch_shape(case):
    wk, ak = case
    w, P, model = _case(wk)
    act = torch.from_numpy(_value_rows()).to(DEV) if wk == "value" else _acts(ak, n=1000, seed=9)
    n = act.shape[0]
    if wk == "value":
        z = hr.value_preact(P, act, "split")
        assert z.abs().max().item() >= 12 and z.abs().min().item() <= 0.05
        assert z.max().item() >= 12 and z.min().item() <= -12                     # saturated +1 and -1 are among them
    p_s, v_s, st = _call(model, "full", act, n, True)                             # sliced: slice 8
    assert _sliced(st)
    p_o, v_o, _ = _call(model, "full", act, n, False)                             # one-pass: the riding workgroups
    assert _same_bits(v_s, v_o), "the two launch shapes run value_head_block: the same bits"
    for sc, p in ((True, p_s), (False, p_o)):                                     # policy only: no value is written,
        p2, v2, _ = _call(model, "full", act, n, sc, value=False)                 # the policy keeps its bits
        assert v2 is None and _same_bits(p2, p)
    assert torch.isfinite(v_s).all() and (v_s.abs() <= 1).all()
    if wk == "value":
        assert (v_s == 1).any() and (v_s == -1).any()
    err = _value_error(v_s, P, act)
    _record("value %s-%s" % case, {"error": err, "max |v - ref|": (v_s.double() - hr.value(P, act, "split")).abs().max().item(),
                                   "vs exact": (v_s.double() - hr.value(P, act, "exact")).abs().max().item()})
    assert err <= VALUE_BOUND, err


# ---- bit-exact probes: no tolerance ------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["flat", "peaked"])
def test_probe_zero_activations_give_the_bias(kind):
    w, P, model = _case(kind)
    rows = 3
    act = torch.zeros((rows, 192), device=DEV)
    labels, counts = _windows(rows, seed=2)
    pri, _, st = _call(model, "raw", act.repeat_interleave(8, 0).contiguous(), rows * 8, True, labels, counts)
    lg = _from_windows(pri, labels, counts, rows)
    bias = torch.from_numpy(np.asarray(w["policy.dense.bias"], np.float32)).to(DEV)
    assert _same_bits(lg, bias.unsqueeze(0).expand(rows, -1).contiguous())


def _uniform_probe(model, bias=None):
    """Zero weights: (both forms' probabilities, the sliced statistics) on random activations."""
    act = _acts("base", n=hu.ROWS, seed=8)
    p_s, _, st = _call(model, "full", act, act.shape[0], True, bias=bias)
    p_o, _, _ = _call(model, "full", act, act.shape[0], False, bias=bias)
    return p_s, p_o, st.reshape(-1, 8, 2)


def _uniform_holds(p_s, p_o, st):
    want = torch.full_like(p_s, float(np.float32(1.0) / np.float32(1968.0)))
    sums = torch.tensor([256.0] * 7 + [176.0], device=DEV).expand(st.shape[0], -1)
    return {"sliced 1/1968": _same_bits(p_s, want), "onepass 1/1968": _same_bits(p_o, want),
            "slice sums": torch.equal(st[..., 1], sums) and bool((st[..., 0] == 0).all()),
            "sliced rowsum": (p_s.double().sum(1) - 1).abs().max().item() <= ROWSUM_BOUND,
            "onepass rowsum": (p_o.double().sum(1) - 1).abs().max().item() <= ROWSUM_BOUND}


def test_probe_zero_weights_give_the_uniform_policy():
    """Every probability is fp32(1 / 1968) in both forms; s = 256 for slices 0-6 and 176 for slice 7: the pad."""
    _, _, model = _case("zero")
    held = _uniform_holds(*_uniform_probe(model))
    assert all(held.values()), held


def test_probe_one_hot_rows_pin_every_policy_weight():
    """Zero bias, x = e_i for all 128 i (each with the 8 label windows: 1024 boards): logit[i][label] is
    fp32(Whi[i][label]) + fp32(Wlo[i][label]) bit for bit -- all 128 x 1968 packed weights, individually."""
    w, P, model = _case("nobias")
    act = torch.zeros((128, 192), device=DEV)
    act[torch.arange(128), torch.arange(128)] = 1.0
    labels, counts = _windows(128, seed=3)
    pri, _, _ = _call(model, "raw", act.repeat_interleave(8, 0).contiguous(), 1024, True, labels, counts)
    lg = _from_windows(pri, labels, counts, 128)
    want = P.policy.whi + P.policy.wlo                                           # exact in fp32 (test_heads_reference.py)
    assert torch.equal(want.float().double(), want)
    assert torch.equal(lg.double(), want), "%d packed policy weights are not where the kernel reads them" % \
        int((lg.double() != want).sum())
    nz = want != 0
    assert torch.equal(_bits(lg)[nz], _bits(want.float())[nz])


def test_probe_one_hot_rows_pin_every_value_weight():
    """b1 = 0, x = e_i for all 64 i, w2 one-hot at hidden unit j (rewritten in place, all 256 j: every tile and every
    q): value[i] is tanh(relu(Whi + Wlo)[i][j] + b2) within tanhf's error; both launch shapes, the same bits."""
    w, P, model = _case("nobias")
    act = torch.zeros((64, 192), device=DEV)
    act[torch.arange(64), 128 + torch.arange(64)] = 1.0
    keep = model._val_w2.clone()
    got = torch.empty((256, 64), device=DEV)
    try:
        for j in range(256):
            w2 = torch.zeros(257, device=DEV)
            w2[j] = 1.0
            w2[256] = keep[256]
            model._val_w2.copy_(w2)
            _, v_s, _ = _call(model, "full", act, 64, True)
            _, v_o, _ = _call(model, "full", act, 64, False)
            assert _same_bits(v_s, v_o), j
            got[j] = v_s
    finally:
        model._val_w2.copy_(keep)
        torch.cuda.synchronize()
    h = torch.relu(P.value1.whi + P.value1.wlo)                                    # [64 i][256 j], exact in fp32
    b2 = float(keep[256].item())
    z = (h.float() + torch.tensor(b2, dtype=torch.float32, device=DEV)).double()   # the kernel's fp32 sum, exactly
    err = (got.t().double() - torch.tanh(z)).abs().max().item()
    err_unrounded = (got.t().double() - torch.tanh(h + b2)).abs().max().item()
    _record("value one-hot", {"|v - tanh(fp32(z + b2))|": err, "|v - tanh(z + b2)|": err_unrounded, "weights": h.numel()})
    assert (h > 0).any() and (h == 0).any()
    assert err <= TANH_BOUND, err
    # a wrong weight moves z by the weight's size: far beyond the bound wherever the ReLU is open
    assert (P.value1.whi + P.value1.wlo).abs().median().item() >= 1000 * TANH_BOUND


# ---- batch and count edges ------------------------------------------------------------------------------------

def _edge_runs(kind):
    """The reference runs of the edge tests: 2048 boards sliced and 2049 boards one-pass (the default dispatch on
    both sides of its boundary), and each batch in the other form."""
    key = ("edge", kind)
    if key not in _CACHE:
        w, P, model = _case(kind)
        act = _acts("base", n=2049, seed=7)
        p_s, v_s, st = _call(model, "full", act, 2048, True)
        assert _sliced(st)
        p_o, v_o, st_o = _call(model, "full", act, 2049, True)                    # default dispatch: one-pass
        assert not _sliced(st_o)
        _CACHE[key] = dict(P=P, model=model, act=act, sliced=(p_s, v_s), onepass=(p_o, v_o))
    return _CACHE[key]


@pytest.mark.parametrize("kind", ["flat", "peaked"])
def test_dispatch_boundary_2048_2049_against_the_reference(kind):
    """2048: the largest sliced batch; 2049: the smallest one-pass batch (129 policy workgroups + 17 value workgroups,
    the last with one live wave).  Every board against the reference, in both forms."""
    e = _edge_runs(kind)
    P, model, act = e["P"], e["model"], e["act"]
    assert _lib().heads_raw_supported(2048) is True and _lib().heads_raw_supported(2049) is False
    with _SlicedMax(4096):                                                        # 2049 boards forced into slices
        p_f, v_f, st_f = _call(model, "full", act, 2049, True)
        assert _sliced(st_f)
    assert _lib().heads_raw_supported(2049) is False                              # (restored)
    p1, v1, _ = _call(model, "full", act, 2048, False)                            # 2048 boards one-pass
    assert _same_bits(p_f[:2048], e["sliced"][0]) and _same_bits(v_f[:2048], e["sliced"][1])
    assert _same_bits(p1, e["onepass"][0][:2048]) and _same_bits(v1, e["onepass"][1][:2048])
    assert _same_bits(v_f, e["onepass"][1])                                       # the value: one arithmetic
    rec = {}
    for name, (p, v) in (("sliced 2049", (p_f, v_f)), ("onepass 2049", e["onepass"])):
        rec[name] = {"split": _e2e(p, P, act, "split")[0], "exact": _e2e(p, P, act, "exact")[0],
                     "rowsum": (p.double().sum(1) - 1).abs().max().item(), "value": _value_error(v, P, act)}
    _record("boundary %s" % kind, rec)
    for name, r in rec.items():
        assert r["split"] <= E2E_BOUND["split"] and r["exact"] <= E2E_BOUND["exact"], (name, r)
        assert r["rowsum"] <= ROWSUM_BOUND and r["value"] <= VALUE_BOUND, (name, r)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 2048, 2049])
@pytest.mark.parametrize("kind", ["flat", "peaked"])
def test_a_board_keeps_its_bits_at_every_batch_size_and_position(kind, n):
    e = _edge_runs(kind)
    model, act = e["model"], e["act"]
    p, v, st = _call(model, "full", act, n, True)                                 # default dispatch
    assert _sliced(st) == (n <= 2048)
    ref_p, ref_v = e["sliced" if n <= 2048 else "onepass"]
    assert _same_bits(p, ref_p[:n]) and _same_bits(v, ref_v[:n])
    if n <= 17:
        p, v, _ = _call(model, "full", act, n, False)                             # one-pass
        assert _same_bits(p, e["onepass"][0][:n]) and _same_bits(v, e["onepass"][1][:n])
        for scratch, form, last in ((True, "sliced", 2048), (False, "onepass", 2049)):
            for first in (3, last - n):                                           # another position in the batch
                sub = act[first:first + n].contiguous()
                p, v, _ = _call(model, "full", sub, n, scratch)
                assert _same_bits(p, e[form][0][first:first + n]) and _same_bits(v, e[form][1][first:first + n])


@pytest.mark.parametrize("form", ["sliced", "raw", "onepass"])
def test_legal_count_edges(form):
    """counts 0, 1, 218, 256, 300 (clamped to 256) and -3 (clamped to 0): nothing is written past the count, the
    listed labels carry the full policy's bits.  The over-count boards are last, guard rows behind them."""
    w, P, model = _case("peaked")
    counts = np.array([0, 1, 218, 256, 17, 35, 0, 256, 1, 60, 218, 5, 99, 256, 128, 64, 33, -3, 7, 300, -3, 300], np.int32)
    n = len(counts)
    act = _acts("base", n=n, seed=10)
    rng = np.random.default_rng(4)
    labels = np.stack([rng.permutation(1968)[:256] for _ in range(n + 3)]).astype(np.uint16)    # guard rows too: owned
    lab_d = torch.from_numpy(labels.view(np.int16)).to(DEV)
    cnt_d = torch.from_numpy(np.concatenate([counts, [256, 256, 256]]).astype(np.int32)).to(DEV)
    sliced = form != "onepass"
    full, val, st_full = _call(model, "full", act, n, sliced)
    pri, val2, st = _call(model, "raw" if form == "raw" else "legal", act, n, sliced, lab_d, cnt_d)
    assert _same_bits(val, val2)
    eff = np.clip(counts, 0, 256)
    fullc, pric = full.cpu().numpy(), pri.cpu().numpy()
    if form == "raw":
        assert _same_bits(st, st_full)
        prob = hr.prob_from_stats(pri.double(), st.reshape(n, 8, 2)).cpu().numpy()
        top = st.reshape(n, 8, 2)[..., 0].double().max(1).values.cpu().numpy()
    for b in range(n):
        k = eff[b]
        assert (pric[b, k:] == SENT).all(), (b, counts[b])
        if form == "raw":
            got = fullc[b, labels[b, :k]].astype(np.float64)
            depth = top[b] - pric[b, :k].astype(np.float64)
            assert (prob[b, :k] >= TINY).all()
            ok = np.abs(got - prob[b, :k]) <= (PROB_BOUND[0] + PROB_BOUND[1] * depth) * prob[b, :k]
            assert ok.all(), b
        else:
            assert np.array_equal(pric[b, :k].view(np.uint32), fullc[b, labels[b, :k]].view(np.uint32)), (b, counts[b])


# ---- the consumers of slices.hpp in the search ----------------------------------------------------------------

def test_search_trees_are_identical_in_all_three_policy_formats_on_a_peaked_head():
    """CRL_POLICY_FULL / LEGAL / LEGAL_RAW (search.hpp gather_priors and argmax_policy normalise on read through
    crl_slices::norm_of / prob) with a PEAKED policy head: the same trees bit for bit, both moves."""
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.model import ChessModel
    from tests.test_gpu_search import move_ids, random_prefix_games
    games = random_prefix_games(24, 70, seed=29)
    w0 = hu.flat_weights()
    base = ChessModel(weights=w0, precision="f16")
    eng = LockstepEngine(base, n_games=24, max_sims=4, use_graph=False)
    eng.load_moves([move_ids(g) for g in games])
    eng.ctx.encode(eng.planes_s1.data_ptr())
    eng.ctx.sync()
    _, hp = base._run_fused(eng.planes_s1)
    torch.cuda.synchronize()
    eng.close()
    # the dense kernel only (the trunk stays what it was), scaled on the MEDIAN root: the roots' activations differ widely
    w = hu.scaled_policy(w0, hp.cpu().numpy(), 70.0, stat=np.median)
    model = ChessModel(weights=w, precision="f16")
    sims, out = 40, []
    for legal, raw in ((False, False), (True, False), (True, None)):
        eng = LockstepEngine(model, n_games=24, max_sims=sims, legal_priors=legal, use_graph=False, raw_priors=raw)
        assert eng.legal_priors == legal and eng.raw_priors == (raw is None)
        eng.load_moves([move_ids(g) for g in games])
        eng.search(sims)
        first = eng.root_children()
        chosen = np.where(first["nchild"] > 0, np.maximum(first["visits"].argmax(1), 0), -1).astype(np.int32)
        bm, am = eng.advance(chosen)
        eng.search(sims)
        out.append((first, bm, am, eng.root_children(), eng.ctx.counters()))
        eng.close()
    (a1, abm, aam, a2, ac) = out[0]
    # the FULL run's root priors come from the model's full policy vectors: the legal moves' spread on the roots
    spreads = []
    for g in range(24):
        k = int(a1["nchild"][g])
        if k >= 2:
            pr = a1["priors"][g, :k].astype(np.float64)
            spreads.append(200.0 if pr.min() <= 0 else float(np.log(pr.max() / pr.min())))     # (0: underflowed)
    _record("search peaked: legal-move spread on the roots (min, median, max)",
            (min(spreads), float(np.median(spreads)), max(spreads), len(spreads)))
    assert len(spreads) >= 12 and np.sum(np.array(spreads) >= 20) * 2 >= 24
    for (b1, bbm, bam, b2, bc) in out[1:]:
        for a, b in ((a1, b1), (a2, b2)):
            assert np.array_equal(a["nchild"], b["nchild"]) and np.array_equal(a["visits"], b["visits"])
            assert np.array_equal(a["values"].view(np.uint64), b["values"].view(np.uint64))
            assert np.array_equal(a["priors"].view(np.uint32), b["priors"].view(np.uint32))
            assert np.array_equal(a["replies"], b["replies"]) and np.array_equal(a["moves"], b["moves"])
        assert np.array_equal(abm, bbm) and np.array_equal(aam, bam)
        assert {k: int(v) for k, v in ac.items()} == {k: int(v) for k, v in bc.items()}


# ---- negative controls: each must FAIL the bound it is aimed at ---------------------------------------------------

def _logit_error(lg, P, act, drop=None):
    return ((lg.double() - hr.logits(P, act, "split", drop)).abs() / hr.logit_condition(P, act)).max().item()


def test_negative_controls_fail_the_bounds():
    c = _local(("flat", "base"))
    w, P, model, act, rows = c["w"], c["P"], c["model"], c["act"], c["rows"]
    lg, st = c["logits"], c["stats"]
    assert _logit_error(lg, P, act) <= LOGIT_BOUND
    found = {}
    # the reference without one of the three products, against the unmodified kernels: policy and value
    for drop in ("lo_whi", "hi_wlo"):
        found["logits, drop " + drop] = (_logit_error(lg, P, act, drop), LOGIT_BOUND)
        found["value, drop " + drop] = (_value_error(c["values_all"][:, 0], P, act, drop), VALUE_BOUND)
    assert _value_error(c["values_all"][:, 0], P, act) <= VALUE_BOUND

    def rerun(image=None, bias=None):
        pri, _, _ = _call(model, "raw", c["rep"], rows * 8, True, c["labels"], c["counts"], image=image, bias=bias)
        return _from_windows(pri, c["labels"], c["counts"], rows)

    # one fp16 element of the packed policy kernel scaled by 1.01: Whi of the largest activation's input, at the label
    # that input weighs most
    i = int(act[:, :128].max(0).values.argmax())
    o = int(P.policy.whi[i].abs().argmax())
    image = model._pol_wp.clone()
    j = hr.fragment_offset(o, i, 4, 0)
    assert image[j].double() == P.policy.whi[i, o]                               # (the documented layout finds that weight)
    image[j] = (image[j].float() * 1.01).half()
    found["Whi element x1.01"] = (_logit_error(rerun(image=image), P, act), LOGIT_BOUND)
    # one Wlo element zeroed: the one whose product with an activation of this batch is largest
    contrib = act[:, :128].double().max(0).values.unsqueeze(1) * P.policy.wlo.abs()
    i, o = divmod(int(contrib.argmax()), 1968)
    image = model._pol_wp.clone()
    j = hr.fragment_offset(o, i, 4, 1)
    assert image[j].double() == P.policy.wlo[i, o] and image[j] != 0
    image[j] = 0
    found["Wlo element zeroed"] = (_logit_error(rerun(image=image), P, act), LOGIT_BOUND)
    # one bias entry shifted by 1e-3 of the logit scale
    bias = model._pol_bias.clone()
    ref = hr.logits(P, act, "split")
    bias[777] += 1e-3 * ref.abs().max().item()
    found["bias +1e-3"] = (_logit_error(rerun(bias=bias), P, act), LOGIT_BOUND)
    # statistics with two slices' maxima swapped (their sums left), fed to prob_from_stats: on the peaked head, where
    # the slices' maxima differ
    cp = _local(("peaked", "base"))
    full, _, _ = _call(cp["model"], "full", cp["rep"], cp["rows"] * 8, True)
    p = full[::8].contiguous()
    depth = cp["stats"][..., 0].double().max(1).values.unsqueeze(1) - cp["logits"].double()
    assert _depth_record(p, hr.prob_from_stats(cp["logits"], cp["stats"]), depth)[2] <= 1.0
    swapped = cp["stats"].clone()
    swapped[:, 2, 0], swapped[:, 5, 0] = cp["stats"][:, 5, 0], cp["stats"][:, 2, 0]
    found["slice maxima swapped"] = (_depth_record(p, hr.prob_from_stats(cp["logits"], swapped), depth)[2], 1.0)
    # ... and whole slices swapped: M and S are symmetric in the slices, but the bit-exact slice-maximum probe is not
    whole = cp["stats"][:, [0, 1, 5, 3, 4, 2, 6, 7]]
    m_own = hr.pad_logits(cp["logits"]).reshape(-1, 8, 256).max(-1).values
    assert torch.equal(cp["stats"][..., 0].double(), m_own) and not torch.equal(whole[..., 0].double(), m_own)
    _record("controls", found)
    for name, (err, bound) in found.items():
        assert err > bound, (name, err, bound)
    # a pad bias of 0 instead of -1e30: fails the uniform and sum-to-one probes
    _, _, zero = _case("zero")
    bias = zero._pol_bias.clone()
    assert (bias[1968:] == np.float32(-1e30)).all()
    bias[1968:] = 0
    held = _uniform_holds(*_uniform_probe(zero, bias=bias))
    _record("controls: pad bias 0", held)
    assert not any(held.values()), held


def test_zz_print_measured():
    """(runs last: the measured values of this file, for the bounds above)"""
    for k in sorted(MEASURED, key=str):
        print("MEASURED %s: %s" % (k, MEASURED[k]))
