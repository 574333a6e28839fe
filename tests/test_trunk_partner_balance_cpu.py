"""CPU: the partner balance of the rank-tile trunk kernels, k_trunk_x16<128, 4, *, 1, 1, 0, 0, 0> (csrc/tower_x16.hpp,
ALT = 1), under the ISA emulation of tools/lds_race_check.py -- stem + 2 residual blocks = 5 convolutions, all 8 waves
of a workgroup, both plane formats.

Waves w and w + 4 share a SIMD.  ALT = 1 has two compile-time choices; the library ships ONE of them:

  * requests (CRL_TRUNK_ALT_REQ = 2, shipped): behind a tap's sync only the lower rank half (waves 0-3) issues LDS-DMA
    -- its own four 1-KiB pieces directly behind the barrier, the four of its partner a sub-step later -- and the upper
    half issues no weight request inside the loop.  Tiles 0 .. 3 in front of the loop stay with every wave (two pieces
    each: 8 per wave); 9 * 5 - 2 = 43 syncs request tiles; waves 0 and 1 also move the five bias rows.  MFMAs and
    fragment reads are those of ALT = 0: 2640 per wave, 660 activation and 720 weight fragment reads.
  * edge ranks (CRL_TRUNK_ALT_EDGE = 1, in the harness only: it measured no gain, docs/history/experiments.md round
    13): the upper half owns ranks {0, 7, 1, 6} and skips a block in all six dy != 0 taps, the lower half owns
    {2, 3, 4, 5} and never skips: 5 * 576 = 2880 against 5 * 480 = 2400 MFMAs, 720 against 600 activation fragment
    reads, the same total of 21 120.  That build is emulated here as well: it proves the counters and keeps the harness
    variant race-free.

Neither adds or removes a barrier: the number of barrier epochs is that of the ALT = 0 kernel in the same assembly.
"""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_trunk_rank_tiles_cpu import CONVS, RING_AT, _checker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BALANCED = ("128,4,0,1,1,0,0,0", "128,4,1,1,1,0,0,0")
PRODUCTION = "128,4,1,0,1,0,0,0"
SYNCS = 9 * CONVS - 2                           # tap syncs that request tiles
PROLOGUE = 4 * 2                                # tiles 0 .. 3, two 1-KiB pieces per wave each

SOURCE = """#include "tower_x16.hpp"
namespace crl_tower {
#define CRL_INST(BITS, ALT) template __global__ void k_trunk_x16<128, 4, BITS, ALT, 1, 0, 0, 0>( \\
    const unsigned char *, const unsigned char *, const float *, float *, int, const float *, const float *, float *);
CRL_INST(0, 1) CRL_INST(1, 1) CRL_INST(1, 0)
}
"""


def _build(tmp_path_factory, edge):
    """{kernel: (findings, stats, metadata)} of the two ALT = 1 kernels and the ALT = 0 bitboard kernel; edge None =
    the library's build."""
    from chessrl_amd import _lib
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("partner_balance_%s" % edge)
    src, asm = str(d / "three_kernels.hip"), str(d / "three_kernels.s")
    with open(src, "w") as f:
        f.write(SOURCE)
    flags = [f for f in _lib.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    assert not any("CRL_TRUNK_ALT" in f for f in flags)
    extra = [] if edge is None else ["-DCRL_TRUNK_ALT_EDGE=%d" % edge]
    subprocess.check_call(["hipcc"] + flags + extra + ["-I", os.path.join(ROOT, "chessrl_amd", "csrc"), "-S",
                                                       "--offload-device-only", src, "-o", asm],
                          stderr=subprocess.DEVNULL)
    chk = _checker()
    segs = {t: sg for f, t, sg in chk.kernels_of(asm) if f == "k_trunk_x16"}
    assert sorted(segs) == sorted(BALANCED + (PRODUCTION,))
    meta = {}
    for block in open(asm).read().split("- .agpr_count")[1:]:
        m = re.search(r"\.name:\s+\S*k_trunk_x16I(.*?)EEv", block)
        meta[m.group(1).replace("Li", "").replace("E", ",").rstrip(",")] = block
    out = {}
    for t in segs:
        ins, labels = chk.parse_kernel(segs[t])
        out[t] = chk.check_workgroup(ins, labels, (CONVS - 1) // 2, ring_at=RING_AT) + (meta[t],)
    return out


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    return _build(tmp_path_factory, None)


@pytest.fixture(scope="module")
def edge(tmp_path_factory):
    return _build(tmp_path_factory, 1)


def _resources(meta):
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 256
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", meta).group(1)) == 0


def _requests(stats):
    """Choice 2 in both builds: the lower half requests for both, the upper half nothing inside the loop."""
    want = [PROLOGUE + 8 * SYNCS + (CONVS if w < 2 else 0) for w in range(4)] + [PROLOGUE] * 4
    assert stats["dma_per_wave"] == want, stats["dma_per_wave"]
    assert stats["dma_transfers"] == sum(want) == 8 * PROLOGUE + 8 * 4 * SYNCS + 2 * CONVS   # as many as ALT = 0 moves
    for wave, dist in enumerate(stats["sync_to_dma_mfma_per_wave"]):
        # the lower half's first request follows the barrier at once; the upper half has no requesting sync at all
        assert dist == ([0] * SYNCS if wave < 4 else []), (wave, dist)


@pytest.mark.parametrize("kernel", BALANCED)
def test_library_build_lower_half_requests_for_both_and_the_counts_are_those_of_production(library, kernel):
    findings, stats, meta = library[kernel]
    assert findings == []
    assert stats["mfma_per_wave"] == [2640] * 8, stats
    assert stats["mfma"] == 21120
    assert stats["w_frag_reads_per_wave"] == [720] * 8, stats
    assert stats["act_frag_reads_per_wave"] == [660] * 8, stats
    _requests(stats)
    _, production, _ = library[PRODUCTION]
    assert stats["epochs"] == production["epochs"]
    assert stats["mfma"] == production["mfma"] and stats["dma_transfers"] == production["dma_transfers"]
    assert production["dma_per_wave"][4:] == [PROLOGUE + 4 * SYNCS] * 4        # (what the upper half no longer issues)
    _resources(meta)


@pytest.mark.parametrize("kernel", BALANCED)
def test_edge_rank_build_moves_the_skipped_blocks_to_the_upper_half(edge, kernel):
    findings, stats, meta = edge[kernel]
    assert findings == []
    assert stats["mfma_per_wave"] == [2880] * 4 + [2400] * 4, stats
    assert stats["mfma"] == 21120
    assert stats["w_frag_reads_per_wave"] == [720] * 8, stats
    assert stats["act_frag_reads_per_wave"] == [720] * 4 + [600] * 4, stats
    _requests(stats)
    assert stats["epochs"] == edge[PRODUCTION][1]["epochs"]
    _resources(meta)
