"""CPU: WHEN the rank-tile trunk kernels k_trunk_x16<128, 4, *, 0, 1, 0, 0, 0> request their weight tiles
(csrc/tower_x16.hpp, CRL_TRUNK_DMA_PHASE), under the ISA emulation of tools/lds_race_check.py -- stem + 2 residual
blocks = 5 convolutions, all 8 waves of a workgroup.

A tap's sync (vmcnt(0), s_barrier at the start of the tap's last sub-step) frees two ring slots; every wave then
requests 4 pieces of 1 KiB (tiles t+3, t+4).  Waves w and w + 4 share a SIMD and leave the barrier together.  The lower
rank half (waves 0-3) requests directly behind the barrier.  The upper half (waves 4-7) does so too with phase 0; with
the library's phase 2 it requests a whole sub-step later, at the start of the next tap -- and in a layer's last tap
behind the first-half MFMAs of the sync's own sub-step, because the next layer's activations do not exist yet.

The distance is measured on the executed path, per wave: the MFMAs between a barrier and the first LDS-DMA request
behind it (lds_race_check.sync_to_dma).  What phase 2 promises the upper half, per convolution of nine taps: a sub-step
is 4 position blocks x 4 channel blocks = 16 MFMAs, 12 in taps 6-8 where this half skips the block that is off the
board (dy = +1); the last tap's first half is 2 blocks less the skipped one = 4 MFMAs.  The build with
-DCRL_TRUNK_DMA_PHASE=0 gives 0 on both halves, which proves the counter.  The last two syncs of a launch request
nothing (no tile t+3): 9 * 5 - 2 = 43 requesting syncs per wave.
"""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_trunk_rank_tiles_cpu import CONVS, KERNELS, RING_AT, SOURCE, _checker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNCS = 9 * CONVS - 2                           # tap syncs that request tiles
PIECES = 4                                      # per wave and sync: two tiles of 16 KiB over 8 waves, 1 KiB each
# MFMAs the upper rank half issues between a tap's sync and its first request, taps 0 .. 8 of a convolution
PROMISE = {0: [0] * 9, 1: [8] * 6 + [4] * 3, 2: [16] * 6 + [12, 12, 4]}
LIBRARY_PHASE = 2


def _build(tmp_path_factory, phase):
    """{kernel: (findings, stats, kernel text)} of both plane formats; phase None = the library's build."""
    from chessrl_amd import _lib
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("dma_phase_%s" % phase)
    src, asm = str(d / "two_kernels.hip"), str(d / "two_kernels.s")
    with open(src, "w") as f:
        f.write(SOURCE)
    flags = [f for f in _lib.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    assert not any("CRL_TRUNK_DMA_PHASE" in f or "CRL_TRUNK_STAMPS" in f for f in flags)
    extra = [] if phase is None else ["-DCRL_TRUNK_DMA_PHASE=%d" % phase]
    subprocess.check_call(["hipcc"] + flags + extra + ["-I", os.path.join(ROOT, "chessrl_amd", "csrc"), "-S",
                                                       "--offload-device-only", src, "-o", asm],
                          stderr=subprocess.DEVNULL)
    chk = _checker()
    segs = {t: sg for f, t, sg in chk.kernels_of(asm) if f == "k_trunk_x16"}
    assert sorted(segs) == sorted(KERNELS)
    meta = {}
    for block in open(asm).read().split("- .agpr_count")[1:]:
        m = re.search(r"\.name:\s+\S*k_trunk_x16I(.*?)EEv", block)
        meta[m.group(1).replace("Li", "").replace("E", ",").rstrip(",")] = block
    out = {}
    for t in KERNELS:
        ins, labels = chk.parse_kernel(segs[t])
        out[t] = chk.check_workgroup(ins, labels, (CONVS - 1) // 2, ring_at=RING_AT) + (ins, meta[t])
    return out


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    return _build(tmp_path_factory, None)


@pytest.fixture(scope="module")
def phase0(tmp_path_factory):
    return _build(tmp_path_factory, 0)


@pytest.fixture(scope="module")
def seeded(tmp_path_factory):
    return _build(tmp_path_factory, -1)


def _expected(phase, wave):
    per_conv = PROMISE[phase] if wave >= 4 else [0] * 9
    return (per_conv * CONVS)[:SYNCS]


@pytest.mark.parametrize("kernel", KERNELS)
def test_library_build_lower_half_requests_at_the_sync_upper_half_a_sub_step_later(library, kernel):
    findings, stats, _, _ = library[kernel]
    assert findings == []
    for wave, dist in enumerate(stats["sync_to_dma_mfma_per_wave"]):
        print("wave %d: %s" % (wave, dist[:9]))
        assert len(dist) == SYNCS, (wave, len(dist))
        want = _expected(LIBRARY_PHASE, wave)
        if wave < 4:
            assert dist == want, (wave, dist)
        else:
            assert all(d >= w for d, w in zip(dist, want)), (wave, dist, want)
            assert min(dist) >= 4


@pytest.mark.parametrize("kernel", KERNELS)
def test_phase_0_requests_at_the_sync_on_both_halves(phase0, kernel):
    findings, stats, _, _ = phase0[kernel]
    assert findings == []
    for wave, dist in enumerate(stats["sync_to_dma_mfma_per_wave"]):
        assert dist == [0] * SYNCS, (wave, dist)


@pytest.mark.parametrize("kernel", KERNELS)
def test_same_pieces_mfmas_waits_and_barriers_as_phase_0(library, phase0, kernel):
    _, stats, ins, meta = library[kernel]
    _, stats0, ins0, _ = phase0[kernel]
    # tiles 0 .. 3 (two pieces each) in front of the loop, 4 pieces per requesting sync, and the five bias rows
    # from waves 0 and 1
    per_wave = [4 * 2 + PIECES * SYNCS + (CONVS if w < 2 else 0) for w in range(8)]
    assert stats0["dma_per_wave"] == per_wave, stats0["dma_per_wave"]
    assert stats["dma_per_wave"] == stats0["dma_per_wave"]
    assert stats["dma_transfers"] == stats0["dma_transfers"] == sum(per_wave)
    for key in ("mfma_per_wave", "act_frag_reads_per_wave", "w_frag_reads_per_wave", "epochs"):
        assert stats[key] == stats0[key], key
    assert stats["mfma_per_wave"] == [2640] * 8

    def texts(code, prefix):
        return sorted(x[4] for x in code if x[4].startswith(prefix))
    for prefix in ("s_barrier", "s_waitcnt vmcnt", "v_mfma", "global_load_lds"):
        a, b = texts(ins, prefix), texts(ins0, prefix)
        assert len(a) == len(b), (prefix, len(a), len(b))
    assert [x[4] for x in ins if "vmcnt" in x[4]] == [x[4] for x in ins0 if "vmcnt" in x[4]]
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 256
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", meta).group(1)) == 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_requests_in_front_of_the_sync_are_found(seeded, kernel):
    """The seeded build (-DCRL_TRUNK_DMA_PHASE=-1, assembly only): the upper half requests before vmcnt(0) and the
    barrier, into slots whose tiles the workgroup is still reading in that epoch."""
    findings, stats, _, _ = seeded[kernel]
    assert any("LDS-DMA transfer into it is in flight" in f for f in findings), findings
    assert stats["mfma_per_wave"] == [2640] * 8
