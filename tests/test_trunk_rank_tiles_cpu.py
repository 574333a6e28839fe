"""CPU: the rank tiles of k_trunk_x16<128, 4, *, 0, 1, 0, 0, 0> (csrc/tower_x16.hpp) under the ISA emulation of
tools/lds_race_check.py -- stem + 2 residual blocks = 5 convolutions, all 8 waves of a workgroup.

A wave owns 4 position blocks x 4 channel blocks; a convolution is 9 taps x 4 sub-steps of 32 input channels, so the
board tiles issue 9 * 4 * 16 = 576 MFMAs and 9 * 4 * 4 = 144 activation and as many weight fragment reads per
wave and convolution.  With rank tiles one block of every wave is off the board in three taps (dy = -1 for the lower
rank half, dy = +1 for the upper): 3 * 4 * 4 = 48 MFMAs and 3 * 4 = 12 activation fragment reads are not issued,
the weight fragment reads stay.  The same counts on a build with CRL_TRUNK_RANKPAIR=0 give the board tiles' numbers,
which proves the counter.
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("128,4,0,0,1,0,0,0", "128,4,1,0,1,0,0,0")
CONVS = 5
# Geo16<128, 4>: 4 boards of 64 rows of 288 bytes, 16 zero rows, two bias rows of 128 floats, rounded up to 1 KiB
RING_AT = ((4 * 64 * 288 + 16 * 288 + 2 * 128 * 4 + 1023) // 1024) * 1024

# the two instantiations alone, with the library's flags: the header is the kernels' only source
SOURCE = """#include "tower_x16.hpp"
namespace crl_tower {
template __global__ void k_trunk_x16<128, 4, 0, 0, 1, 0, 0, 0>(const unsigned char *, const unsigned char *, const float *,
                                                              float *, int, const float *, const float *, float *);
template __global__ void k_trunk_x16<128, 4, 1, 0, 1, 0, 0, 0>(const unsigned char *, const unsigned char *, const float *,
                                                              float *, int, const float *, const float *, float *);
}
"""


def _checker():
    import importlib
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    return importlib.import_module("lds_race_check")


@pytest.fixture(scope="module", params=[1, 0], ids=["rank_tiles", "board_tiles"])
def emulated(request, tmp_path_factory):
    """{kernel: (findings, stats)} of both plane formats for CRL_TRUNK_RANKPAIR = 1 / 0."""
    from chessrl_amd import _lib
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("rank_tiles_%d" % request.param)
    src, asm = str(d / "two_kernels.hip"), str(d / "two_kernels.s")
    with open(src, "w") as f:
        f.write(SOURCE)
    flags = [f for f in _lib.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    subprocess.check_call(["hipcc"] + flags + ["-DCRL_TRUNK_RANKPAIR=%d" % request.param, "-I",
                                               os.path.join(ROOT, "chessrl_amd", "csrc"), "-S", "--offload-device-only",
                                               src, "-o", asm], stderr=subprocess.DEVNULL)
    chk = _checker()
    segs = {t: sg for f, t, sg in chk.kernels_of(asm) if f == "k_trunk_x16"}
    assert sorted(segs) == sorted(KERNELS)
    out = {}
    for t in KERNELS:
        ins, labels = chk.parse_kernel(segs[t])
        out[t] = chk.check_workgroup(ins, labels, (CONVS - 1) // 2, ring_at=RING_AT)
    return request.param, out


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_finding_and_every_wave_issues_the_counted_mfmas_and_fragment_reads(emulated, kernel):
    rank_tiles, results = emulated
    findings, stats = results[kernel]
    assert findings == []
    mfma = CONVS * (9 * 4 * 16 - (3 * 4 * 4 if rank_tiles else 0))
    act = CONVS * (9 * 4 * 4 - (3 * 4 if rank_tiles else 0))
    w = CONVS * 9 * 4 * 4
    assert mfma == (2640 if rank_tiles else 2880)
    assert stats["mfma_per_wave"] == [mfma] * 8, stats
    assert stats["mfma"] == 8 * mfma
    assert stats["w_frag_reads_per_wave"] == [w] * 8, stats
    assert stats["act_frag_reads_per_wave"] == [act] * 8, stats
