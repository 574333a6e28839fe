"""CPU: the three host-side pieces ChessModel is built from -- the weight images (chessrl_amd/packing.py), the
precision rules (chessrl_amd/precision.py) and the argument checks of the typed stream-level wrappers
(chessrl_amd/_lib.py).  None of them needs a device."""
import hashlib
import json
import math
import os

import numpy as np
import pytest
import torch

from chessrl_amd import _lib, packing, precision

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packing_digests.json")))


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: "%dx%d-%s" % (c["blocks"], c["filters"], c["requested"]))
def test_packed_images_are_the_recorded_ones_byte_for_byte(case):
    """The digests were recorded from ChessModel._pack_fused before the packing moved here (golden file: produced_by)."""
    from oracle import tower_oracle
    w = tower_oracle.init_weights(case["blocks"], case["filters"], case["seed"], randomize_bn=True)
    req = case["requested"]
    images = packing.pack_weights(w, case["blocks"], case["filters"], want_f16=req in ("auto", "f16", "hybrid"),
                                  want_x3=req in ("auto", "f16x3", "hybrid"))
    assert tuple(GOLDEN["names"]) == packing.NAMES and len(images) == len(packing.NAMES)
    h = hashlib.sha256()
    for name, x in zip(packing.NAMES, images):
        assert x.device.type == "cpu"
        h.update(name.encode())
        h.update(str(x.dtype).encode())
        h.update(x.contiguous().numpy().tobytes())
    assert h.hexdigest() == case["sha256"]
    assert (images[0].numel() == 8) == (req == "f16x3") and (images[1].numel() == 8) == (req == "f16")


def test_log_distance_speaks_only_about_entries_both_arithmetics_have():
    from chessrl_amd.model import ChessModel
    for fn in (precision.log_distance, ChessModel._log_distance):
        assert fn(torch.tensor([0.0, 0.5]), torch.tensor([0.1, 0.5])) == 0.0
        assert fn(torch.tensor([0.0]), torch.tensor([0.1])) is None
        assert fn(torch.tensor([0.2]), torch.tensor([0.0])) is None
    assert abs(precision.log_distance(torch.tensor([0.2, 0.5]), torch.tensor([0.1, 0.5])) - math.log(2.0)) < 1e-6


def test_choose_mode():
    tol = 8e-4
    assert precision.choose_mode("auto", 8e-4, 1e-5, tol, "hybrid") == "f16"              # at the tolerance: kept
    assert precision.choose_mode("auto", 8.01e-4, 1e-5, tol, "hybrid") == "hybrid"
    assert precision.choose_mode("auto", 1e-5, 8.01e-4, tol, "f16x3") == "f16x3"          # the value counts as well
    # after the guard has fired the probe must pass with margin
    assert precision.probe_tolerance(tol, 0.5, False) == tol and precision.probe_tolerance(tol, 0.5, True) == 4e-4
    assert precision.choose_mode("auto", 5e-4, 1e-5, precision.probe_tolerance(tol, 0.5, False), "hybrid") == "f16"
    assert precision.choose_mode("auto", 5e-4, 1e-5, precision.probe_tolerance(tol, 0.5, True), "hybrid") == "hybrid"
    # a NaN distance is within nothing
    assert precision.choose_mode("auto", float("nan"), 0.0, tol, "hybrid") == "hybrid"
    assert precision.choose_mode("auto", 0.0, float("nan"), tol, "hybrid") == "hybrid"
    # a mode asked for by name is that mode, whatever the probe says
    for name in ("f16", "f16x3", "hybrid"):
        assert precision.choose_mode(name, 1.0, 1.0, tol, "hybrid") == name
        assert precision.choose_mode(name, 0.0, 0.0, tol, "f16x3") == name


def test_widened_margin():
    k, cap = 2.0, 8.0
    assert precision.widened_margin(1e-3, 1e-3, 4e-4, k, cap) == (1e-3, False)            # below the margin in force
    assert precision.widened_margin(1e-3, 1e-3, 5e-4, k, cap) == (1e-3, False)            # exactly at it
    assert precision.widened_margin(1e-3, 1e-3, 2e-3, k, cap) == (4e-3, False)            # widened to k x dlog
    assert precision.widened_margin(1e-3, 1e-3, 1.0, k, cap) == (8e-3, True)              # capped at cap x the probe's
    assert precision.widened_margin(9e-3, 1e-3, 1.0, k, cap) == (9e-3, True)              # the cap lies below: no change
    assert precision.widened_margin(4e-3, 1e-3, 2e-3, k, cap) == (4e-3, False)            # never shrinks
    m, capped = precision.widened_margin(float("nan"), 1e-3, 1.0, k, cap)                 # a NaN margin stays (lists all)
    assert math.isnan(m) and not capped


def test_reply_rule_on_hand_made_rows():
    junk = 5.0                                                        # beyond the legal count: must never be looked at
    rows16 = [[0.9, junk, junk, junk],                                # one legal move
              [0.7, 0.2, 0.1, junk],                                  # gap log 3.5 >= margin, same argmax
              [0.4, 0.35, 0.25, junk],                                # gap log(8/7) < margin: listed (and it differs)
              [float("nan"), 0.3, 0.2, junk],                         # NaN gap: listed
              [0.7, 0.2, 0.1, junk],                                  # gap >= margin but f16x3 chooses another move
              [junk, junk, junk, junk]]                               # no legal move (a row that needs no policy)
    rows48 = [[0.9, junk, junk, 2 * junk],
              [0.6, 0.3, 0.1, junk],
              [0.35, 0.4, 0.25, junk],
              [0.5, 0.3, 0.2, junk],
              [0.2, 0.7, 0.1, 2 * junk],
              [0.0, junk, 0.0, 0.0]]
    counts = torch.tensor([1, 3, 3, 3, 3, 0], dtype=torch.int32)
    listed, differ, unlisted, gap = precision.reply_rule(torch.tensor(rows16), torch.tensor(rows48), counts, 0.5)
    assert listed.tolist() == [False, False, True, True, False, False]
    assert differ.tolist() == [False, False, True, False, True, False]
    assert unlisted.tolist() == [False, False, False, False, True, False]
    assert abs(float(gap[1]) - math.log(3.5)) < 1e-6 and abs(float(gap[2]) - math.log(8.0 / 7.0)) < 1e-6
    assert math.isnan(float(gap[3])) and abs(float(gap[4]) - math.log(3.5)) < 1e-6
    # the margin is compared with >=: a gap exactly at the margin is not listed, a NaN margin lists every board with a choice
    assert not precision.reply_rule(torch.tensor(rows16), torch.tensor(rows48), counts, float(gap[1]))[0][1]
    assert precision.reply_rule(torch.tensor(rows16), torch.tensor(rows48), counts, float("nan"))[0].tolist() == \
        [False, True, True, True, True, False]


# ---- the typed wrappers of the stream-level entry points ---------------------------------------------------------
HEADS = dict(n_boards=4, dev_policy_wp_f16=16, dev_policy_bias_f32=32, dev_value_w1p_f16=48, dev_value_b1_f32=64,
             dev_value_w2b2_f32=80)


def test_wrappers_refuse_bad_pointers_before_the_library_is_reached(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    strided = torch.zeros((4, 8))[:, ::2]
    assert not strided.is_contiguous()
    with pytest.raises(ValueError, match="dev_head_act_f32 is not contiguous"):
        _lib.heads_forward(strided, dev_policy_out_f32=96, **HEADS)
    with pytest.raises(ValueError, match="dev_policy_out_f32 must not be NULL"):
        _lib.heads_forward(8, dev_policy_out_f32=None, **HEADS)
    with pytest.raises(ValueError, match="dev_stats_out_f32 must not be NULL"):            # required by the raw form only
        _lib.heads_forward_legal_raw(8, dev_labels=1, dev_counts=2, dev_logits_out_f32=3, dev_value_out_f32=None,
                                     dev_stats_out_f32=None, **HEADS)
    with pytest.raises(ValueError, match="dev_planes must not be NULL"):
        _lib.trunk_forward_x(64, 0, None, 1, 2, None, 4, 1, 3, 4, None)
    with pytest.raises(ValueError, match="dev_list is not contiguous"):
        _lib.trunk_forward_indexed(64, 1, 2, 3, 4, 1, 5, 6, 7, torch.zeros(16, dtype=torch.int32)[::2])
    with pytest.raises(ValueError, match="dev_log_margin_f32 must not be NULL"):
        _lib.reply_margin(1, 2, 4, None, 0, 3)
    with pytest.raises(ValueError, match="dev_ring must not be NULL"):
        _lib.stamp(None, 16, 1)


def test_wrappers_marshal_in_header_order_and_name_the_entry_point_that_failed(monkeypatch):
    calls = []

    class FakeLibrary(object):
        def __getattr__(self, name):
            return lambda *args: calls.append((name, [getattr(a, "value", a) for a in args])) or (-1 if args[2] == 13 else 0)

    monkeypatch.setattr(_lib, "lib", FakeLibrary)
    act = torch.zeros((4, 192))
    _lib.heads_forward(act, dev_policy_out_f32=96, hip_stream=7, **HEADS)                  # value and scratch may be NULL
    assert calls[-1] == ("crl_heads_forward", [7, act.data_ptr(), 4, 16, 32, 48, 64, 80, 96, None, None])
    _lib.trunk_forward_x(128, 3, 1000, 2000, 3000, None, 8, 2, 4000, 5000, 6000, 7000, 4096, hip_stream=9)
    assert calls[-1] == ("crl_trunk_forward_x", [9, 128, 3, 1000, 2000, 3000, None, 8, 2, 4000, 5000, 6000, 7000, 4096])
    _lib.reply_margin(100, 200, 8, 300, 1, 400, hip_stream=np.int64(5))
    assert calls[-1] == ("crl_reply_margin", [5, 100, 200, 8, 300, 1, 400])
    with pytest.raises(_lib.HipLibraryError, match=r"crl_heads_forward failed \(-1\)"):
        _lib.heads_forward(act, 13, 16, 32, 48, 64, 80, 96, hip_stream=7)
