"""CPU: the layer hand-over of k_trunk_x16 (csrc/tower_x16.hpp) in the compiled ISA.

The hand-over is what a wave runs between the last MFMA of a convolution and the first of the next: the barrier
behind the tap loop, the epilogue (conv1: convert + packed ReLU; conv2 and the stem: + skip stream, max, convert),
the activation writes, the barrier in front of the next layer.  All eight waves of a workgroup are in it at once, so
every VALU instruction there runs with the MFMA pipe idle.  The fp32 skip stream `res` (PT x CT x 4 registers) and
the retired accumulators live across it; with a three-way epilogue (stem / conv1 / conv2) hipcc chained phi copies of
both -- 192 v_mov_b32 among the 419 vector instructions of the 128-filter NB = 4 kernel's hand-over.  The epilogue
has two shapes now (the stem is a conv2 with a -0 skip stream and a -inf floor) and the hand-over copies nothing.

Found in the ISA as: from the first s_barrier behind the kernel's last MFMA to the last branch back to a label in
front of its first MFMA (the head of the layer loop).  Every path through a layer's hand-over lies in that range, so
"no v_mov_b32 in the range" covers the stem's, conv1's and conv2's.  The arithmetic that has to be there is counted
too (per wave: one v_add_f32 and one v_max_f32 per element of conv2, one v_cvt_pk_f16_f32 per two elements of
either shape, one v_pk_max_f16 per two elements of conv1, one ds_write_b128 per eight): a range that is not the
epilogue, or an epilogue that lost or gained arithmetic, fails as well.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# template arguments -> (MFMAs in the kernel's text, elements of a wave tile = 4 PT CT; None: split epilogue)
KERNELS = {
    "128,4,1,0,1,0,0,0": (1056, 64),        # C3 (rank tiles: 2 rank halves x 9 taps unrolled, 48 MFMAs skipped each)
    "128,2,1,0,1,0,0,0": (96, 32),          # its NB = 2 sibling
    "64,2,1,0,0,0,0,0": (216, 16),          # 64 filters, plain ring (C2 at up to 512 boards)
    "64,4,1,0,0,1,0,0": (96, 32),           # 64 filters, group pipeline
    "128,2,1,0,1,0,1,0": (224, None),       # split precision: hi / lo stores, fp32 ReLU
}
SIG = "(const unsigned char *, const unsigned char *, const float *, float *, int, const float *, const float *, float *)"
SOURCE = '#include "tower_x16.hpp"\nnamespace crl_tower {\n' + "".join(
    "template __global__ void k_trunk_x16<%s>%s;\n" % (t.replace(",", ", "), SIG) for t in KERNELS) + "}\n"


def _checker():
    import importlib
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    return importlib.import_module("lds_race_check")


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{template arguments: (instructions, labels, the kernel's metadata text)}"""
    from chessrl_amd import _lib
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("handover")
    src, asm = str(d / "kernels.hip"), str(d / "kernels.s")
    with open(src, "w") as f:
        f.write(SOURCE)
    flags = [f for f in _lib.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    subprocess.check_call(["hipcc"] + flags + ["-I", os.path.join(ROOT, "chessrl_amd", "csrc"), "-S",
                                               "--offload-device-only", src, "-o", asm], stderr=subprocess.DEVNULL)
    chk = _checker()
    meta = {}
    for block in open(asm).read().split("- .agpr_count")[1:]:
        m = re.search(r"\.name:\s+\S*k_trunk_x16I(.*?)EEv", block)
        meta[m.group(1).replace("Li", "").replace("E", ",").rstrip(",")] = block
    out = {t: chk.parse_kernel(seg) + (meta[t],) for f, t, seg in chk.kernels_of(asm) if f == "k_trunk_x16"}
    assert sorted(out) == sorted(KERNELS)
    return out


def _handover(ins, labels):
    """The instructions from the barrier behind the last MFMA to the last branch back in front of the first MFMA --
    and, where hipcc has rotated the layer loop so that the epilogue's closing barrier heads it, on to that barrier."""
    mfma = [i for i, x in enumerate(ins) if x[0].startswith("v_mfma")]
    start = next(i for i in range(mfma[-1], len(ins)) if ins[i][0] == "s_barrier")
    back = [i for i in range(start, len(ins)) if ins[i][0].startswith(("s_branch", "s_cbranch"))
            and labels.get(ins[i][1][0], len(ins)) < mfma[0]]
    assert back, "no branch back to the layer loop's head"
    region = ins[start:back[-1] + 1]
    if _count(region, "s_barrier") < 2:
        head = labels[ins[back[-1]][1][0]]
        close = next(i for i in range(head, mfma[0]) if ins[i][0] == "s_barrier")
        region = region + ins[head:close + 1]
    return region


def _count(region, prefix):
    return sum(1 for x in region if x[0].startswith(prefix))


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_register_copy_on_any_path_through_the_hand_over(compiled, kernel):
    ins, labels, _ = compiled[kernel]
    region = _handover(ins, labels)
    assert _count(region, "s_barrier") == 2 and _count(region, "v_mfma") == 0, "not the layer hand-over"
    copies = [x[4] for x in region if x[0].startswith(("v_mov_b32", "v_mov_b64", "v_pk_mov_b32", "v_accvgpr"))]
    print("%s: %d instructions, %d vector, %d copies" % (kernel, len(region), _count(region, "v_"), len(copies)))
    assert copies == []           # the stem's path too: it is the conv2 path


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_hand_over_holds_the_epilogue_arithmetic(compiled, kernel):
    ins, labels, _ = compiled[kernel]
    region = _handover(ins, labels)
    n = KERNELS[kernel][1]
    if n is None:
        # split (fp32 ReLU): conv1 = n max, each behind a canonicalising max(x, x) of the MFMA result (IEEE mode);
        # conv2 = n adds + n max; both: hi = cvt(v), lo = cvt(v - float(hi)) (the subtractions count as adds)
        n = 32
        assert _count(region, "v_add_f32") + 2 * _count(region, "v_pk_add_f32") >= n
        assert _count(region, "v_max_f32") == 3 * n
        assert _count(region, "ds_write_b128") == 2 * (2 * n // 8)
        return
    got = {op: _count(region, op) for op in ("v_add_f32", "v_pk_add_f32", "v_max_f32", "v_cvt_pk_f16_f32",
                                             "v_pk_max_f16", "ds_write_b128")}
    assert got["v_add_f32"] + 2 * got["v_pk_add_f32"] == n, got          # conv2 (and the stem, on a -0 skip stream)
    assert got["v_max_f32"] == n, got                                      # conv2's ReLU / the stem's floor of -inf
    assert got["v_cvt_pk_f16_f32"] == 2 * (n // 2), got                    # conv1 + conv2
    assert got["v_pk_max_f16"] == n // 2, got                              # conv1's ReLU on packed halves
    assert got["ds_write_b128"] == 2 * (n // 8), got


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_mfma_count_registers_and_no_scratch(compiled, kernel):
    ins, _, meta = compiled[kernel]
    assert _count(ins, "v_mfma") == KERNELS[kernel][0]
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 256          # two waves per SIMD
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", meta).group(1)) == 0
    assert _count(ins, "scratch_") == 0 and _count(ins, "buffer_") == 0
