// tower_x16.hpp -- the fused residual trunk (design: tower_common.hpp) on v_mfma_f32_16x16x32_f16
// (the round-1 kernels on v_mfma_f32_32x32x16_f16 left the tree in round 6; git history has them).
//
// Why: the trunk is matrix-pipe bound on a POWER-limited clock.  With the same 64x64 wave tile,
// the same LDS bytes per MAC and the same 64 accumulator registers, a 16x16x32 loop sustains
// 1.14x the FLOP/s of the 32x32x16 loop on MI355X (tools/ubench/mfma_shapes.hip: 1780 vs 1554
// TFLOP/s with every operand re-read from LDS; MI355X_MICROARCH.md, DVFS give-back item 7: equal
// cycles per FLOP, higher held clock).  Results are NOT bit-identical to the 32x32x16 kernels:
// the K = 32 contraction of one instruction sums in a different order (both accumulate fp32).
//
// What changes against the round-1 32x32x16 kernels:
//   * a wave tile of MT x NT 32x32 blocks becomes PT x CT = 2MT x 2NT blocks of 16 positions x 16
//     channels; a sub-step is 32 input channels: PT + CT fragment reads feed PT*CT MFMAs;
//   * fragment lanes: lane l = 16 q + r reads row r of its block, 16-byte quarter q of the 64-byte
//     K block.  Activation rows are padded to (2 mod 16) 16-byte units (288 / 544 bytes): the 16
//     lanes of a ds_read_b128 group -- 8 rows at quarter q, 8 at q+1 -- then cover all 64 banks;
//   * a weight tile is one 64-byte-row plane per 32 input channels, rows in the order the
//     accumulators want them (Geo16::row_channel), chunk swizzle (-(row >> 2)) & 3; the host packs
//     the global image in exactly that order, so the DMA source is contiguous;
//   * the accumulator of block (pt, ct) holds, per lane, 4 consecutive channels of position
//     16 pt + r; channel blocks 2g and 2g+1 are interleaved (Geo16::chan_of) so that a lane's 4 + 4
//     values are 8 consecutive channels and the epilogue writes 16-byte words in place;
//   * the head convolutions reduce 4 CG partial sums per output (4 lane quarters x CG waves).
#pragma once
#include "tower_common.hpp"

namespace crl_tower {

// SPLIT = 1 (precision mode "f16x3"): every activation is kept as TWO fp16 numbers, hi = fp16(x) and
// lo = fp16(x - hi), side by side in its LDS row ([hi: F channels | lo: F channels]), the folded
// weights likewise as two fp16 images, and a product is hi.Whi + hi.Wlo + lo.Whi (the dropped
// lo.Wlo term is 2^-22 relative): three MFMAs for fp32-grade results -- the same device as
// csrc/heads.hpp.  It is run as a convolution over an EXTENDED input: per spatial tap two weight "parts",
// the planes of Whi and the planes of Wlo, each a virtual tap like the channel halves of a 256-filter
// layer, so the tap loop, the weight ring and the pipeline are the ones below; Whi passes through the ring
// ONCE and every one of its weight sub-steps feeds two MFMA sub-steps, against hi and against lo (the
// stem's 0/1 planes have no lo: one); the weight image lists the planes in that order.
template <int F, int NB_, int SPLIT_ = 0>
struct Geo16 {
    static_assert(F == 64 || F == 128 || F == 256, "supported filter counts");
    static constexpr int SPLIT = SPLIT_;
    static constexpr int LO_OFF = F * 2;                // byte offset of the lo half inside an activation row
    static constexpr int NB = NB_;                      // boards per workgroup
    static constexpr int WPB = 8 / NB;                  // waves per board
    static constexpr int NT = (F == 64 && NB == 2) ? 1 : 2;
    static constexpr int CT = 2 * NT;                   // 16-channel blocks per wave
    static constexpr int CG = F / (16 * CT);            // channel groups (waves splitting the channels)
    static constexpr int PH = WPB / CG;                 // position halves (waves splitting a board)
    static constexpr int PT = 4 / PH;                   // 16-position blocks per wave
    static_assert(NB * CG * PH == 8 && (PH == 1 || PH == 2), "8 waves per workgroup");
    static constexpr int KT = F == 256 ? 32 : 64;       // input channels per weight tile
    static constexpr int SPT = KT / 32;                 // 32-channel sub-steps per tile
    static constexpr int WROW = KT * 2;
    static constexpr int WCH = WROW / 16;
    static constexpr int TILE_BYTES = F * WROW;
    static constexpr int GL = TILE_BYTES / 8192;
    static constexpr int AROW_CH = (SPLIT ? 2 * F : F) < 128 ? 128 : (SPLIT ? 2 * F : F);   // channels a row holds
    static constexpr int AROW = AROW_CH * 2 + 32;
    static constexpr int ABOARD = 64 * AROW;
    static constexpr int ZERO_OFF = NB * ABOARD;
    static constexpr int ZSTRIDE = AROW;                // 16 zero rows laid out like board rows (same bank residues)
    static constexpr int ZERO_BYTES = 16 * ZSTRIDE;
    static constexpr int BIAS_OFF = ZERO_OFF + ZERO_BYTES;          // float [2][F]: this layer's and the next one's
    static constexpr int WRING_OFF = ((BIAS_OFF + 2 * F * 4 + 1023) / 1024) * 1024;
    static constexpr int LDS_BYTES = WRING_OFF + PIPE_RING * TILE_BYTES;
    static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
    static constexpr int lds_bytes(int ring) { return WRING_OFF + ring * TILE_BYTES; }
    // LDS image of a weight tile: one plane per 32-channel sub-step, [SPT][F rows][64 bytes];
    // rows of 16 banks, chunk swizzle (-(row >> 2)) & 3: the 16 lanes of a ds_read_b128 group (8
    // rows at quarter q, 8 at q+1) cover all 64 banks, and the sub-step is an immediate offset.
    static constexpr int WPLANE = F * 64;
    __device__ static int wswz(int row) { return (0 - (row >> 2)) & 3; }
    // Which output channel accumulator row i (= 4 q + j) of channel block ct computes, relative to
    // the wave's first channel: blocks 2g and 2g+1 interleave in units of 4, so that a lane's 4 + 4
    // values of the two blocks are 8 CONSECUTIVE channels 32 g + 8 q .. + 8 and the epilogue writes
    // them as one 16-byte word (half the LDS write instructions, and conflict-free like the reads:
    // same (row, 16-byte quarter) lane map).  The permutation lives in the weight image (row_channel).
    __host__ __device__ static constexpr int chan_of(int ct, int i)
    {
        return 32 * (ct >> 1) + 8 * (i >> 2) + 4 * (ct & 1) + (i & 3);
    }
    // Output channel held by row `row` of a weight plane (rows 16 ct + i of a wave's 16 CT rows): the
    // same bit rotation inside every 32-row block whatever the geometry.  The GLOBAL weight image is
    // stored in exactly the LDS image's order -- planes of [F rows][64 bytes], rows in this order,
    // the four 16-byte chunks of a row at position chunk ^ wswz(row) (chessrl_amd/packing.py:pack_trunk,
    // include/chessrl_hip.h) -- so a tile is one contiguous block that every wave copies in 1-KiB
    // pieces (sixteen 64-byte half lines per piece before: -0.8 % / -1.9 % at 128 / 256 filters).
    __host__ __device__ static constexpr int row_channel(int row)
    {
        return (row & ~31) + chan_of((row >> 4) & 1, row & 15);
    }
};

// Slots of the weight ring: 4 in the plain ring, 5 with pair publishing, with the group pipeline 3 groups of 3
// tiles (4 groups at two boards per workgroup).  The kernel's LDS budget and every launch take it from here.
constexpr int GROUP_TAPS = 3;                           // group pipeline: taps (= weight tiles) per barrier
template <int NB, int PAIR, int GROUP>
constexpr int ring_slots()
{
    return GROUP ? GROUP_TAPS * (NB == 2 ? 4 : 3) : (PAIR ? 5 : PIPE_RING);
}

// stage weight tile t (global image = the plane image above, contiguous) into ring slot `slot`, or t & 3
// when none is given (the plain ring): every wave moves GL pieces of 1 KiB.
template <class G>
__device__ inline void stage_wtile_x16(const unsigned char *wts, lds_byte *lds, int t, int tid, int wave_u,
                                       int slot = -1)
{
    const unsigned char *src = wts + (size_t)t * G::TILE_BYTES;
    const int slot0 = G::WRING_OFF + (slot < 0 ? (t & (PIPE_RING - 1)) : slot) * G::TILE_BYTES;
    const int dst0 = slot0 + wave_u * 1024;             // uniform
#pragma unroll
    for (int j = 0; j < G::GL; j++) {
        const int idx = j * 512 + tid;                  // 16-byte slot of the tile image (global = LDS order)
        const unsigned off = (unsigned)(idx * 16);
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void *)(src + off),
            (__attribute__((address_space(3))) void *)(lds + dst0 + j * 8192), 16, 0, 0);
    }
}

// piece j (of GL) of the same transfer alone: the rank-tile kernels may spread a tile's requests (CRL_TRUNK_DMA_PHASE)
template <class G>
__device__ inline void stage_wpiece_x16(const unsigned char *wts, lds_byte *lds, int t, int tid, int wave_u, int slot,
                                        int j)
{
    const unsigned char *src = wts + (size_t)t * G::TILE_BYTES;
    const int dst0 = G::WRING_OFF + slot * G::TILE_BYTES + wave_u * 1024;      // uniform
    const unsigned off = (unsigned)((j * 512 + tid) * 16);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void *)(src + off),
        (__attribute__((address_space(3))) void *)(lds + dst0 + j * 8192), 16, 0, 0);
}

// bias row of layer `conv` (F floats) -> LDS row conv & 1, by LDS-DMA: F/64 waves move 256 bytes each.
// Being a DMA like the weight tiles it is covered by the same counted vmcnt waits and barriers; no
// register, no ds_write and no compiler-inserted vmcnt(0) (which would drain the weight stream).
template <class G, int F>
__device__ inline void stage_bias_x16(const float *bias, lds_byte *lds, int conv, int lane, int wave_u)
{
    if (wave_u >= F / 64) return;
    // uniform base + unsigned 32-bit lane offset: the SGPR-base addressing form, no 64-bit lane address to keep
    // (the base goes through readfirstlane so that hipcc cannot fold the lane offset into a hoisted,
    // and then spilled, 64-bit per-lane address)
    const unsigned long long a = reinterpret_cast<unsigned long long>(bias + (size_t)conv * F + wave_u * 64);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    const unsigned char *src = reinterpret_cast<const unsigned char *>(((unsigned long long)hi << 32) | lo);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void *)(src + (unsigned)(lane * 4)),
        (__attribute__((address_space(3))) void *)(lds + G::BIAS_OFF + (conv & 1) * F * 4 + wave_u * 256), 4, 0, 0);
}

typedef float f32x4v __attribute__((ext_vector_type(4)));

// Rank tiles (128 filters, four boards per workgroup, pair ring, f16): a wave owns 2 boards x 4 ranks x 64
// channels instead of 1 board x 8 ranks x 64 channels, so that a 16-position MFMA block is ONE rank of a pair
// of boards and a block whose rank + dy is off the board is off the board as a whole: its MFMAs and its
// activation fragment reads are not issued (k_trunk_x16 below).  0 builds the board tiles of before
// (tools/ubench/trunk_r3.hip times both).
#ifndef CRL_TRUNK_RANKPAIR
#define CRL_TRUNK_RANKPAIR 1
#endif
template <int F, int NB, int PAIR, int GROUP, int SPLIT, int IDX>
struct RankTiles {
    static constexpr bool value = CRL_TRUNK_RANKPAIR != 0 && F == 128 && NB == 4 && PAIR == 1 && GROUP == 0 &&
                                  SPLIT == 0 && IDX == 0;
};

// Rank tiles only: WHEN the waves of the upper rank half (w >= 4) request the weight tiles t+3, t+4 (and their share
// of the next bias row) that a tap's sync frees the slots for.  Waves w and w + 4 share a SIMD and leave the sync's
// barrier together; with 0 both then issue their four 1-KiB requests at once and neither feeds the MFMA pipe
// meanwhile.  The lower half always issues directly behind the barrier; the upper half
//   0  does the same (the schedule of round 10, and its assembly byte for byte),
//   1  issues behind the first-half MFMAs of the sync's sub-step, while its partner is back in its MFMAs,
//   2  issues a whole sub-step later, at the start of the next tap (a layer's last tap: as 1),
//   3  issues when 2 does, but one piece behind each of the first two MFMAs of the sub-step's two halves.
// Every request still follows the sync that frees its slot and precedes the next sync's vmcnt(0); no barrier and
// no wait changes, the MFMAs and their order are the same, results are bit-identical.  (-1 is a seeded fault for
// tools/lds_race_check.py: the upper half requests IN FRONT of the sync.  It exists as assembly on a CPU only.)
// The library builds 2: -2.4 % of the 10 x 128 launch at 4096 boards against 0, -1.5 % with 1, -1.1 % with 3
// (tools/ubench/trunk_r3.hip times the variants; docs/history/experiments.md, round 11).
#ifndef CRL_TRUNK_DMA_PHASE
#define CRL_TRUNK_DMA_PHASE 2
#endif
static_assert(CRL_TRUNK_DMA_PHASE >= -1 && CRL_TRUNK_DMA_PHASE <= 3, "CRL_TRUNK_DMA_PHASE: 0 .. 3");

// Rank tiles, ALT = 1 ("partner balance"): work moves from the wave that reaches every tap sync first -- the older wave
// of the SIMD, w < 4, which wins the issue arbitration and then idles at the barrier -- to its partner w + 4, by two
// independent compile-time choices (tools/ubench/trunk_r3.hip times each alone and both against ALT = 0):
//   CRL_TRUNK_ALT_EDGE  1: the upper half owns the edge ranks, slots -> ranks {0, 7, 1, 6}, and skips the rank-0 block in
//                       the dy = -1 taps and the rank-7 block in the dy = +1 taps; the lower half owns ranks {2, 3, 4, 5}
//                       and never skips: 576 / 480 MFMAs per convolution instead of 528 / 528, still 112 per SIMD and
//                       dy != 0 tap.  0: the rank halves of ALT = 0.
//   CRL_TRUNK_ALT_REQ   1: behind a tap's sync the lower half requests its partner's four 1-KiB pieces with its own,
//                       all eight directly behind the barrier; 2: its own four there and the partner's four a sub-step
//                       later (where phase 2 above puts the upper half's).  The upper half then requests nothing inside
//                       the loop and keeps no request state.  0: every wave requests its own, as ALT = 0 does.
// No barrier and no wait moves, every output element sees the same MFMAs in the same tap and K order: the same bits.
// The library builds edge 0, requests 2: -1.1 % of the 10 x 128 launch at 4096 boards against ALT = 0, the lower half's
// wait at a tap sync 670 -> 247 cycles.  Edge 1 alone changes nothing (-0.1 %: the older wave still wins the issue
// arbitration and still waits 559 cycles, the MFMAs it takes over only move inside the SIMD's pipe), with requests 2 it
// gives -0.8 %; requests 1 is SLOWER with either (+0.9 %: eight requests in one clump keep the wave that feeds the pipe
// first off it for 550 cycles).  docs/history/experiments.md, round 13.
#ifndef CRL_TRUNK_ALT_EDGE
#define CRL_TRUNK_ALT_EDGE 0
#endif
#ifndef CRL_TRUNK_ALT_REQ
#define CRL_TRUNK_ALT_REQ 2
#endif
static_assert(CRL_TRUNK_ALT_EDGE >= 0 && CRL_TRUNK_ALT_EDGE <= 1 && CRL_TRUNK_ALT_REQ >= 0 && CRL_TRUNK_ALT_REQ <= 2,
              "CRL_TRUNK_ALT_EDGE: 0 / 1, CRL_TRUNK_ALT_REQ: 0 .. 2");
// edge ranks: the rank that slot s of rank half hh is
__host__ __device__ constexpr int edge_rank(int hh, int s)
{
    return hh ? (s == 0 ? 0 : (s == 1 ? 7 : (s == 2 ? 1 : 6))) : 2 + s;
}

// What run_tap gets as its rank half where the half has a request schedule of its own: the sync whose requests are
// not issued yet (its tile, its ring slot, whether the next bias row goes with them: plain integers, the taps are
// straight-line code) and the function that issues pieces [P0, P1) of them.  Every other body gets a bare constant,
// so the kernels without rank halves hold none of this.
struct TrunkDmaSync { int t = 0, slot = 0; bool bias = false; };
template <int HH, class P>
struct RankHalfDma {
    static constexpr int value = HH;
    TrunkDmaSync &sync;
    P &pieces;
};
// (through overloads: run_tap names them in statements that a body without a schedule of its own discards, but
// the bare constant must still be a valid argument while that body is being instantiated)
template <class H, class A, class B>
__device__ __forceinline__ void half_pieces(const H &, A, B) {}
template <int HH, class P, class A, class B>
__device__ __forceinline__ void half_pieces(const RankHalfDma<HH, P> &h, A a, B b) { h.pieces(a, b); }
template <class H>
__device__ __forceinline__ void half_record(const H &, bool, int, int) {}
template <int HH, class P>
__device__ __forceinline__ void half_record(const RankHalfDma<HH, P> &h, bool bias, int t, int slot)
{
    h.sync.bias = bias;
    h.sync.t = t;
    h.sync.slot = slot;
}

#if defined(CRL_TRUNK_STAMPS)
// Harness diagnostic (tools/ubench/trunk_r3.hip -DCRL_TRUNK_STAMPS, never in the library, phases 0 .. 2): every wave
// of a rank-tile kernel sums, over its tap syncs, the cycles from the sync's vmcnt wait to the end of its barrier and
// the cycles its weight requests take to issue, wherever the schedule puts them, and lane 0 stores the sums to a
// buffer of their own that nothing reads: [loop, sync wait, requests, syncs, one stamp's own cost] per wave.  A stamp
// drains the wave's LDS reads (s_memtime returns out of order with them), so the build is slower: read its shares.
__device__ unsigned long long *crl_trunk_stamp_buf = nullptr;
__device__ __forceinline__ unsigned long long trunk_stamp()
{
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#endif

//   planes  fp16 [n_boards][64][128], or 128 plane bitboards per board (BITS)
//   wts     fp16 weight planes in consumption order [conv][tap][in-ch/32][F rows][4 chunks][8 in],
//           rows and chunks in the LDS image's order (Geo16::row_channel, wswz)
//   bias    f32 [n_convs][F];  head_w f32 [3][F];  head_b f32 [3]
//   out     f32 [n_boards][64][F] or nullptr;  head_out f32 [n_boards][192] or nullptr
// PAIR = 1 (128 and 256 filters): ONE barrier per TWO weight tiles over a ring of five slots.  The
// sync sits at the start of the last sub-step of every odd tile t: tiles t+1, t+2 (moved at the
// previous sync) are published, tiles t+3, t+4 go into the slots of the dead tiles t-2, t-1.
// GROUP = 1 (64 filters).  There a wave tile is 2x2 / 2x4 blocks: a sub-step is 4 / 8 MFMAs per
// wave and a weight tile (one tap, 8 KiB) lasts 256 / 512 cycles.  The half-sub-step pipeline then
// leaves 2-4 MFMAs between a fragment read and its use (LDS latency is 10x that) and the ring of
// four looks one or two taps ahead of the L2 latency of the weight DMA: the loops ran at 30-45 % of
// their MFMA pace.  GROUP runs the taps in groups of three (one weight tile each, the stem's 128
// planes as two virtual taps of 64): ONE barrier per group, a weight ring of 3 (4 at two boards per
// workgroup) groups, so a tile is requested two (three) groups before it is read, and inside a
// group the six sub-steps run back to back with their fragments fetched TWO sub-steps ahead into
// three register buffers, across tap boundaries (not across layers: those activations do not exist yet).
// IDX = 1 (the fall-back launch of the hybrid precision mode, crl_trunk_forward_indexed): the launch covers a
// LIST of boards.  `out` is then not an output but the list, int32 [LIST_HEADER + n]: [0] = number of listed boards
// (a workgroup beyond it exits at once: the grid is sized for the worst case, the list is written on the
// device), [1 .. 3] unused here (statistics, csrc/heads.hpp), [LIST_HEADER + k] = the board (row of `planes` and of `head_out`) the k-th resident board
// is.  A list that does not fill the last workgroup is padded with its last entry (the same board computed
// twice writes the same values twice).  Nothing else changes: the production kernels (IDX = 0) compile as
// they did.
template <int F, int NB, int BITS = 0, int ALT = 0, int PAIR = 0, int GROUP = 0, int SPLIT = 0, int IDX = 0>
__global__ __launch_bounds__(512, 2) void k_trunk_x16(const unsigned char *__restrict__ planes,
                                                       const unsigned char *__restrict__ wts,
                                                       const float *__restrict__ bias,
                                                       float *__restrict__ out, int n_blocks,
                                                       const float *__restrict__ head_w,
                                                       const float *__restrict__ head_b,
                                                       float *__restrict__ head_out)
{
    // ALT selected diagnostic variants until round 7; 1 is the partner balance of the rank tiles (above)
    static_assert(ALT == 0 || (ALT == 1 && RankTiles<F, NB, PAIR, GROUP, SPLIT, IDX>::value), "ALT = 1: rank tiles only");
    constexpr bool EDGE = ALT == 1 && CRL_TRUNK_ALT_EDGE != 0;
    constexpr int REQ = ALT == 1 ? CRL_TRUNK_ALT_REQ : 0;
    typedef Geo16<F, NB, SPLIT> G;
    static_assert(!SPLIT || !GROUP, "split precision runs the plain / pair pipelines");
    constexpr int PT = G::PT, CT = G::CT;
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds_raw[];
    lds_byte *lds = (lds_byte *)lds_raw;
    const int lds_base = (int)(size_t)lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int board_w = wave / G::WPB;
    const int obase = (16 * CT) * ((wave / G::PH) % G::CG);      // first output channel of this wave
    const int pbase = 32 * (wave % G::PH);              // first position of this wave
    const int r = lane & 15, q = lane >> 4;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    // Rank tiles (RP): wave w = pair (w >> 1) & 1 of the workgroup's boards, channel group w & 1, rank half w >> 2.
    // Block ("slot") pt is one rank: lanes r < 8 are file r of the pair's first board, lanes r >= 8 file r - 8 of
    // its second.  The upper half enumerates its ranks in reverse -- slot s = rank s for half 0, rank 7 - s for
    // half 1 -- so that the block that leaves the board is slot 0 for both: rank 0 under dy = -1, rank 7 under
    // dy = +1.  Waves w and w + 4 are the two waves of one SIMD (waves go to the four SIMDs round robin; the
    // requesting halves of csrc/tower_layer.hpp rest on the same assignment): same pair and channel group,
    // opposite rank halves, so in each of the six dy != 0 taps every SIMD has exactly one wave that skips -- 112
    // MFMAs per tap and SIMD instead of 128 -- and no wave waits at the tap's barrier for a partner with more work.
    constexpr bool RP = RankTiles<F, NB, PAIR, GROUP, SPLIT, IDX>::value;
    const int rp_half = wave_u >> 2;                    // RP: 0 = ranks 0-3 (slot = rank), 1 = ranks 7-4
    const int board = RP ? 2 * ((wave >> 1) & 1) + (r >> 3) : board_w;           // RP: per lane
    // position of the lane in block 0 and the step to the next block, in positions (= activation rows)
    // (EDGE: the lane's file alone; the slots' ranks are the table edge_rank, see slot_pos below)
    const int pos0 = EDGE ? (r & 7) : (RP ? (rp_half ? 56 : 0) + (r & 7) : pbase + r);
    const int pstep = RP ? (rp_half ? -8 : 8) : 16;
    const int n_convs = 1 + 2 * n_blocks;
    // SPLIT: two weight parts per tap (the planes of Whi, then of Wlo)
    const int tiles_stem = 9 * (SPLIT ? 2 : 1) * (128 / G::KT), tiles_conv = 9 * (SPLIT ? 2 : 1) * (F / G::KT);
    const int n_tiles = tiles_stem + 2 * n_blocks * tiles_conv;
    const size_t wg_board0 = (size_t)blockIdx.x * G::NB;
    int rows[G::NB];                                    // IDX: the listed boards this workgroup holds (wave-uniform)
    if constexpr (IDX) {
        static_assert(BITS == 1, "the indexed launch reads plane bitboards");
        const int *list = reinterpret_cast<const int *>(out);
        const int listed = __builtin_amdgcn_readfirstlane(list[0]);
        if ((int)wg_board0 >= listed) return;           // before any DMA or barrier: the whole workgroup leaves
#pragma unroll
        for (int b = 0; b < G::NB; b++) {
            const int k = (int)wg_board0 + b < listed ? (int)wg_board0 + b : listed - 1;
            rows[b] = __builtin_amdgcn_readfirstlane(list[LIST_HEADER + k]);
        }
    }

    static_assert(!PAIR || F == 128 || F == 256, "pair publishing: even tile counts per layer");
    constexpr int GK = GROUP_TAPS;                      // GROUP: taps (= tiles) per barrier
    constexpr int GR = ring_slots<NB, PAIR, GROUP>();   // ring slots
    constexpr int GRG = GR / GK;                        // GROUP: groups in the weight ring
    static_assert(G::lds_bytes(GR) <= 160 * 1024, "LDS budget");
    static_assert(!GROUP || (F == 64 && !PAIR && G::SPT == 2 && G::GL == 1 && 2 * (PT + CT) < 16),
                  "group pipeline: 64 filters");
    stage_bias_x16<G, F>(bias, lds, 0, lane, wave_u);   // oldest transfer: landed when tile 0 has
    if constexpr (GROUP) {
#pragma unroll
        for (int k = 0; k < GK * (GRG - 1); k++) stage_wtile_x16<G>(wts, lds, k, tid, wave_u, k);   // groups 0 .. GRG-2
    } else {
        stage_wtile_x16<G>(wts, lds, 0, tid, wave_u, PAIR ? 0 : -1);
        stage_wtile_x16<G>(wts, lds, 1, tid, wave_u, PAIR ? 1 : -1);
        stage_wtile_x16<G>(wts, lds, 2, tid, wave_u, PAIR ? 2 : -1);
        if constexpr (PAIR) stage_wtile_x16<G>(wts, lds, 3, tid, wave_u, 3);
    }

    {   // planes (128 channels = 16 chunks per position) -> padded LDS rows; zero rows
        if constexpr (IDX) {
            expand_bitplanes_rows<G::NB, G::AROW, G::ABOARD>(planes, lds, rows, tid);
        } else if constexpr (BITS) {
            expand_bitplanes<G::NB, G::AROW, G::ABOARD>(planes, lds, wg_board0, tid);
        } else {
            const u32x4 *src = reinterpret_cast<const u32x4 *>(planes + wg_board0 * BOARD_BYTES);
#pragma unroll
            for (int i = 0; i < G::NB * 2; i++) {
                const int c16 = i * 512 + tid;
                const int p = (c16 >> 4) & 63, c = c16 & 15, b = c16 >> 10;
                u32x4 v = src[c16];
                *reinterpret_cast<__attribute__((address_space(3))) u32x4 *>(
                    lds + b * G::ABOARD + p * G::AROW + (c << 4)) = v;
            }
        }
        for (int i = tid; i < G::ZERO_BYTES / 16; i += 512)
            *reinterpret_cast<__attribute__((address_space(3))) u32x4 *>(lds + G::ZERO_OFF + i * 16) =
                u32x4{0u, 0u, 0u, 0u};
    }
    // tile 0 landed (tiles 1,2 may be in flight).
    // PAIR: tiles 0 AND 1 landed (1 is first read before the first sync), 2 and 3 in flight
    if constexpr (GROUP) wait_vmcnt<GK * (GRG - 2)>();              // group 0 landed, groups 1 .. GRG-2 in flight
    else wait_vmcnt<2 * G::GL>();
    wait_lgkm<0>();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);

    // position of the lane in block pt: p = pbase + 16 pt + r, i.e. file r & 7, rank (pbase >> 3) + 2 pt + (r >> 3)
    // (RP: file r & 7, rank = slot pt or 7 - pt for every lane of the block; ABOARD and 8 AROW are both 0 mod 256
    // bytes, so a lane group reads and writes the bank residues of the board tiles)
    const int px = r & 7, py0 = (pbase >> 3) + (r >> 3);
    const int base0 = lds_base + board * G::ABOARD + pos0 * G::AROW + q * 16;   // block 0's own row
    const int zero_q = lds_base + G::ZERO_OFF + q * 16;
    const int act_row0 = board * G::ABOARD + pos0 * G::AROW;           // the lane's row in block 0
    const int row_step = pstep * G::AROW;               // bytes from a block's row to the next block's
    // block pt's distance from block 0's row, in positions and in bytes of activation rows
    auto slot_pos = [&](int pt) {
        if constexpr (EDGE) return 8 * (rp_half ? edge_rank(1, pt) : edge_rank(0, pt));
        else return pstep * pt;
    };
    auto slot_row = [&](int pt) {
        if constexpr (EDGE) return 8 * G::AROW * (rp_half ? edge_rank(1, pt) : edge_rank(0, pt));
        else return pt * row_step;
    };
    // which lanes have an on-board neighbour to the left / right, and (per block) above / below
    // (RP: above / below is a property of the whole block -- it is computed or skipped, never masked)
    const unsigned long long xm_left = __ballot(px >= 1), xm_right = __ballot(px <= 6);
    unsigned long long ym_up[PT], ym_down[PT];
#pragma unroll
    for (int pt = 0; pt < PT; pt++) {
        ym_up[pt] = RP ? ~0ull : __ballot(py0 + 2 * pt >= 1);
        ym_down[pt] = RP ? ~0ull : __ballot(py0 + 2 * pt <= 6);
    }
    // Weight fragment address: row o = obase + 16 ct + r of a tile plane, quarter q.  The swizzle
    // (-(o >> 2)) & 3 does not depend on ct (16 ct >> 2 is a multiple of 4), so ONE per-lane address
    // serves every channel block, sub-step and tile of a tap through the immediate offset
    // ct * 1024 + sub-step plane + tile slot; only the tap's first ring slot is added per tap.
    const int w0 = lds_base + G::WRING_OFF + (obase + r) * 64 + ((q ^ G::wswz(obase + r)) << 4);
    static_assert((16 * 64) == 1024 && G::TILE_BYTES * 2 + G::WPLANE + 3 * 1024 < 65536, "ds_read immediate");

    f32x4v res[PT][CT];                                 // fp32 residual stream
#pragma unroll
    for (int a = 0; a < PT; a++)
#pragma unroll
        for (int b = 0; b < CT; b++) res[a][b] = f32x4v{-0.f, -0.f, -0.f, -0.f};   // x + -0 == x bit for bit: the stem's add

    constexpr int HP = PT / 2;                          // position blocks per half sub-step

#if defined(CRL_TRUNK_STAMPS)
    static_assert(CRL_TRUNK_DMA_PHASE >= 0 && CRL_TRUNK_DMA_PHASE <= 2, "stamps: not between the MFMAs of phase 3");
    unsigned long long st_wait = 0, st_req = 0, st_syncs = 0;
    const unsigned long long st_t0 = trunk_stamp(), st_self = trunk_stamp() - st_t0;
#endif
    int t = 0;                                          // tile of the K-step being computed
    int slot_tap = 0;                                   // PAIR: ring slot (t mod 5) of the tap's first tile
    auto slot_add = [](int s, int k) { const int x = s + k; return x >= 5 ? x - 5 : x; };
    for (int conv = 0; conv < n_convs; conv++) {
        // the accumulators start from this layer's bias (LDS row conv & 1, staged one layer ahead):
        // the first MFMA of every chain takes it as its C operand, the epilogue adds nothing
        f32x4v acc[PT][CT];
#pragma unroll
        for (int ct = 0; ct < CT; ct++) {
            const f32x4 bv = *reinterpret_cast<const __attribute__((address_space(3))) f32x4 *>(
                lds + G::BIAS_OFF + (conv & 1) * F * 4 + (obase + G::chan_of(ct, 0) + 8 * q) * 4);
#pragma unroll
            for (int pt = 0; pt < PT; pt++) acc[pt][ct] = f32x4v{bv[0], bv[1], bv[2], bv[3]};
        }
        bool bias_staged = false;                       // next layer's bias goes out with the first tile sync

        // Fragment registers: a sub-step (32 channels) runs as two halves of PT/2 position blocks
        // against all CT channel blocks.  xa / xb: the activation fragments of the two halves;
        // w[2]: this sub-step's weight fragments and the next one's.  Half 0 prefetches xb (HP
        // reads); half 1 prefetches the next sub-step's xa and weights (HP + CT reads).
        half8 xa[HP], xb[HP], w[2][CT];
        int ab[2][PT];                                  // [current tap, next tap][pt]

        // one (virtual) tap = NS sub-steps of 32 input channels; sub-step i reads channel block i of
        // the tap's activation rows and sub-step i % SPT of weight tile t_tap0 + i / SPT
        // DUP = 2 (split precision, the Whi planes of a residual conv): every weight sub-step is used by
        // TWO MFMA sub-steps, first against the hi half of the activation rows, then against the lo
        // half LO_OFF bytes further -- the products hi.Whi and lo.Whi share one pass of Whi through the
        // ring and one set of weight fragment reads.  NS counts MFMA sub-steps, NS / DUP weight sub-steps.
        // SK / NSK (rank tiles): block 0 of this tap / of the next tap is off the board as a whole.  Its
        // fragment xa[0] is not read and its CT MFMAs are not issued; every lgkmcnt immediate below counts the
        // reads that are really issued (xb is always HP reads, the next xa HP - its skip).
        auto run_tap = [&](auto NSC, auto DUPC, bool first_tap, bool last_tap, auto SKC, auto NSKC, auto HHC) {
            constexpr int NS = decltype(NSC)::value, DUP = decltype(DUPC)::value;
            // the request schedule of this body: the upper rank half's, if it has one of its own
            constexpr int DPH = (RP && decltype(HHC)::value == 1 && REQ == 0) ? CRL_TRUNK_DMA_PHASE : 0;
            constexpr int NP = 2 * G::GL;                // pieces per wave and sync: tiles t+3 and t+4
            constexpr std::integral_constant<int, 0> p0{};
            constexpr std::integral_constant<int, 1> p1{};
            constexpr std::integral_constant<int, 2> p2{};
            constexpr std::integral_constant<int, NP> pn{};
            static_assert(DPH == 0 || (PAIR && NS == 4 && DUP == 1 && G::SPT == 2 && NP == 4), "one sync per tap, in sub-step 3");
            constexpr int SK = decltype(SKC)::value ? 1 : 0, NSK = decltype(NSKC)::value ? 1 : 0;
            // edge ranks: SKC = 2 says that the block that leaves the board is slot 1; the tap then runs slots 0 and
            // 1 in the other order (ab[] holds the rows in that order, vtap_rows_edge), so the hand-placed schedule
            // below still skips the FIRST block of the first half.  PM(pt): the accumulator block that is.
            constexpr bool SW = decltype(SKC)::value == 2;
            static_assert(!SW || (EDGE && G::PT == 4), "swapped slots belong to the edge ranks");
            auto PM = [](int pt) constexpr { return SW && pt < 2 ? 1 - pt : pt; };
            // ALT = 1 requests: the upper half issues none (NOREQ), the lower half its partner's with its own (REQ 1:
            // all behind the barrier, REQ 2: the partner's where phase 2 puts them)
            constexpr bool NOREQ = REQ != 0 && decltype(HHC)::value == 1;
            constexpr bool LATE4 = REQ == 2 && decltype(HHC)::value == 0;
            static_assert(RP || (SK == 0 && NSK == 0), "whole blocks leave the board only with rank tiles");
            static_assert(DUP == 1 || (SPLIT && DUP == 2), "shared weight sub-steps belong to the split kernels");
            const int t_tap0 = t;
            auto fetch_xa = [&](auto IC, bool next_tap, auto SC) {
                constexpr int i = decltype(IC)::value;
#pragma unroll
                for (int pt = decltype(SC)::value; pt < HP; pt++)
                    xa[pt] = lds_read16_asm<(i / DUP) * 64 + (i % DUP) * G::LO_OFF>(ab[next_tap ? 1 : 0][pt]);
            };
            auto fetch_xb = [&](auto IC) {
                constexpr int i = decltype(IC)::value;
#pragma unroll
                for (int pt = 0; pt < HP; pt++)
                    xb[pt] = lds_read16_asm<(i / DUP) * 64 + (i % DUP) * G::LO_OFF>(ab[0][HP + pt]);
            };
            // Ring of four: a tap's tiles sit in consecutive slots (a tap is 1, 2 or 4 tiles and
            // starts on a multiple of that), so slot and sub-step are immediates on top of the tap's
            // first slot.  Ring of five (PAIR): one base register per tile of the tap (slots wrap).
            constexpr int NSW = NS / DUP;                // weight sub-steps of the tap
            constexpr int TPT = NSW / G::SPT;
            static_assert((TPT == 1 || TPT == 2 || TPT == 4) && PIPE_RING == 4 && NSW % 2 == 0, "ring");
            int wv[PAIR ? TPT : 1], wv_nxt;
            if constexpr (PAIR) {
#pragma unroll
                for (int k = 0; k < TPT; k++) wv[k] = w0 + slot_add(slot_tap, k) * G::TILE_BYTES;
                wv_nxt = w0 + slot_add(slot_tap, TPT) * G::TILE_BYTES;
            } else {
                wv[0] = w0 + (t_tap0 & (PIPE_RING - 1)) * G::TILE_BYTES;
                wv_nxt = w0 + ((t_tap0 + TPT) & (PIPE_RING - 1)) * G::TILE_BYTES;
            }
            auto fetch_w1 = [&](auto IC, auto CC, bool next_tap, half8 (&dst)[CT]) {     // IC: weight sub-step
                constexpr int i = decltype(IC)::value, ct = decltype(CC)::value;
                constexpr int off = ct * 1024 + (i % G::SPT) * G::WPLANE + (PAIR ? 0 : (i / G::SPT) * G::TILE_BYTES);
                dst[ct] = lds_read16_asm<off>(next_tap ? wv_nxt : wv[PAIR ? i / G::SPT : 0]);
            };
            auto fetch_w = [&](auto IC, bool next_tap, half8 (&dst)[CT]) {
                static_for<0, CT>([&](auto CC) { fetch_w1(IC, CC, next_tap, dst); });
            };
            if (first_tap) {
                fetch_xa(std::integral_constant<int, 0>{}, false, std::integral_constant<int, SK>{});
                fetch_w(std::integral_constant<int, 0>{}, false, w[0]);
            }
            static_for<0, NS>([&](auto IC) {
                constexpr int i = decltype(IC)::value;
                constexpr int wi = i / DUP;              // weight sub-step of this MFMA sub-step
                constexpr bool w_first = i % DUP == 0, w_last = i % DUP == DUP - 1;
                constexpr int s = wi % G::SPT;
                constexpr int cur = wi % 2, nxt = 1 - cur;
                if constexpr (!w_first) {
                    // second use of this weight sub-step: no tile event
                } else if constexpr (PAIR) {
                    if constexpr (s == G::SPT - 1 && ((wi / G::SPT) & 1) == 1) {
                        // start of the last sub-step of an odd tile t: tiles t+1, t+2 (moved at the
                        // previous sync, the only transfers in flight) are published; tiles <= t-1
                        // are dead and their slots take tiles t+3, t+4
                        if constexpr (DPH != 0) {         // the requests go out later (seeded fault: now)
                            half_record(HHC, !bias_staged, t, slot_add(slot_tap, wi / G::SPT));
                            bias_staged = true;
                            if constexpr (DPH < 0) half_pieces(HHC, p0, pn);
                        }
#if defined(CRL_TRUNK_STAMPS)
                        const unsigned long long s0 = trunk_stamp();
#endif
                        wait_vmcnt<0>();
                        __builtin_amdgcn_s_barrier();
                        __builtin_amdgcn_sched_barrier(0);
#if defined(CRL_TRUNK_STAMPS)
                        const unsigned long long s1 = trunk_stamp();
                        st_wait += s1 - s0;
                        st_syncs++;
#endif
                        if constexpr (DPH == 0 && !NOREQ) {
                        if (!bias_staged) {
                            bias_staged = true;
                            if (conv + 1 < n_convs) stage_bias_x16<G, F>(bias, lds, conv + 1, lane, wave_u);
                        }
                        const int slot_cur = slot_add(slot_tap, wi / G::SPT);
                        if (t + 3 < n_tiles) stage_wtile_x16<G>(wts, lds, t + 3, tid, wave_u, slot_add(slot_cur, 3));
                        if (t + 4 < n_tiles) stage_wtile_x16<G>(wts, lds, t + 4, tid, wave_u, slot_add(slot_cur, 4));
                        if constexpr (REQ == 1) {         // and the pieces of the partner wave w + 4 (thread tid + 256)
                            if (t + 3 < n_tiles) stage_wtile_x16<G>(wts, lds, t + 3, tid + 256, wave_u + 4, slot_add(slot_cur, 3));
                            if (t + 4 < n_tiles) stage_wtile_x16<G>(wts, lds, t + 4, tid + 256, wave_u + 4, slot_add(slot_cur, 4));
                        }
                        if constexpr (LATE4) half_record(HHC, false, t, slot_cur);   // the partner's go out a sub-step later
#if defined(CRL_TRUNK_STAMPS)
                        st_req += trunk_stamp() - s1;
#endif
                        }
                    }
                } else if constexpr (s == G::SPT - 1) {
                    // publish tile t+1 before the half that prefetches its first fragments;
                    // recycle tile t-1's slot
                    if (t + 2 < n_tiles) wait_vmcnt<G::GL>();
                    else wait_vmcnt<0>();
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                    if (!bias_staged) {
                        bias_staged = true;
                        if (conv + 1 < n_convs) stage_bias_x16<G, F>(bias, lds, conv + 1, lane, wave_u);
                    }
                    if (t + 3 < n_tiles) stage_wtile_x16<G>(wts, lds, t + 3, tid, wave_u);
                }
                // phase 2: the previous tap's sync was a whole sub-step ago
                if constexpr ((DPH == 2 || LATE4) && i == 0) { if (!first_tap) half_pieces(HHC, p0, pn); }
                // ---- half 0: position blocks [0, HP)
                fetch_xb(IC);
                wait_lgkm<HP>();                         // xa and w[cur] have landed
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (DPH == 3 && (i == 0 || i == NS - 1)) {     // phase 3: behind the half's first two MFMAs
                    const bool now = i == 0 ? !first_tap : last_tap;
                    static_for<SK * CT, HP * CT>([&](auto KC) {
                        constexpr int k = decltype(KC)::value, pt = k / CT, ct = k % CT;
                        acc[PM(pt)][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[cur][ct], xa[pt], acc[PM(pt)][ct], 0, 0, 0);
                        if constexpr (k == SK * CT) { if (now) half_pieces(HHC, p0, p1); }
                        if constexpr (k == SK * CT + 1) { if (now) half_pieces(HHC, p1, p2); }
                    });
                } else {
#pragma unroll
                for (int pt = SK; pt < HP; pt++)
#pragma unroll
                    for (int ct = 0; ct < CT; ct++)
                        acc[PM(pt)][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[cur][ct], xa[pt], acc[PM(pt)][ct], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                // phase 1 (and a layer's last tap in phase 2): the partner wave is back in its MFMAs
                if constexpr (DPH == 1 && i == NS - 1) half_pieces(HHC, p0, pn);
                if constexpr ((DPH == 2 || LATE4) && i == NS - 1) { if (last_tap) half_pieces(HHC, p0, pn); }
                // ---- half 1: position blocks [HP, PT); prefetch the next sub-step
                constexpr bool wrap = i + 1 >= NS;
                bool issued = false;
                // the next sub-step's activation fragments before the wait; its CT weight fragments
                // one by one behind the first CT MFMAs of this half: a wave that issues all HP + CT
                // reads in one clump keeps its MFMAs waiting behind 6 KiB of LDS transfers, -1.1 ..
                // -1.6 % of kernel time at 128 and 256 filters (round 3, docs/history/experiments.md)
                if (!wrap || !last_tap) {
                    issued = true;
                    if constexpr (wrap) fetch_xa(std::integral_constant<int, 0>{}, true, std::integral_constant<int, NSK>{});
                    else fetch_xa(std::integral_constant<int, i + 1>{}, false, std::integral_constant<int, SK>{});
                }
                if (!issued) wait_lgkm<0>();
                else wait_lgkm<HP - (wrap ? NSK : SK)>();            // xb has landed
                __builtin_amdgcn_sched_barrier(0);
                static_for<0, HP * CT>([&](auto KC) {
                    constexpr int k = decltype(KC)::value, pt = k / CT, ct = k % CT;
                    acc[HP + pt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[cur][ct], xb[pt], acc[HP + pt][ct], 0, 0, 0);
                    if constexpr (k < CT && w_last) {                 // the next MFMA sub-step has new weights
                        __builtin_amdgcn_sched_barrier(0);
                        if (issued) {
                            if constexpr (wrap) fetch_w1(std::integral_constant<int, 0>{}, KC, true, w[nxt]);
                            else fetch_w1(std::integral_constant<int, wi + 1>{}, KC, false, w[nxt]);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if constexpr (DPH == 3 && k < 2 && (i == 0 || i == NS - 1)) {
                        if (i == 0 ? !first_tap : last_tap)
                            half_pieces(HHC, std::integral_constant<int, 2 + k>{}, std::integral_constant<int, 3 + k>{});
                    }
                });
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (s == G::SPT - 1 && w_last) t++;
            });
        };

        // A spatial tap with more than 128 input channels runs as Cin/128 "virtual taps" of 128
        // channels each (same neighbour rows, channel offset 256 bytes further): every virtual tap
        // is NS = 4 sub-steps, one unrolled body for the stem and the 128- and 256-filter layers.
        // (GROUP: virtual taps of 64 channels, so it is the stem's 128 planes that split in two)
        const int hshift = GROUP ? (conv == 0 ? 1 : 0) : ((conv != 0 && F == 256) ? 1 : 0);
        constexpr int chstep = GROUP ? 128 : 256;       // bytes between the channel halves of a spatial tap
        // SPLIT: a spatial tap is parts x pieces virtual taps (pieces = channel halves as above); part 0 =
        // the planes of Whi, used against hi and -- in the residual convs, whose input has a lo half -- in
        // the same pass against lo (run_tap DUP = 2); part 1 = the planes of Wlo against hi
        const int parts = SPLIT ? 2 : 1;
        const int per_tap = parts << hshift;
        const int nv = 9 * per_tap;
        // Activation row address of block pt for virtual tap v: the lane's own row shifted by
        // (8 dy + dx) rows when that neighbour is on the board, else the zero row whose index has
        // the same residue mod 16 (same banks).  The zero-row address and the file test do not
        // depend on pt: per block only the rank test and one select remain.
        int base0_tap = base0, r_tap = r;               // (RP: per tap, see there)
        auto vtap_rows = [&](int v, int (&dst)[PT]) {
            int tap, choff;
            if constexpr (SPLIT) {
                // order inside a spatial tap: part (Whi, Wlo) major, channel piece minor; the lo half of
                // the rows is an immediate of the reads (run_tap)
                tap = v / per_tap;
                const int rem = v - tap * per_tap;
                choff = (rem & ((1 << hshift) - 1)) * chstep;
            } else {
                tap = v >> hshift;
                choff = (v & ((1 << hshift) - 1)) * chstep;
            }
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
            const int shift = 8 * dy + dx;
            const int zrow = zero_q + ((r_tap + shift) & 15) * G::ZSTRIDE + choff;
            const int inb = base0_tap + shift * G::AROW + choff;
            // on-board tests as wave masks in SGPRs (computed once per kernel): per block only a
            // scalar AND, one add and one select remain
            const unsigned long long xm = dx < 0 ? xm_left : (dx > 0 ? xm_right : ~0ull);
#pragma unroll
            for (int pt = 0; pt < PT; pt++) {
                const unsigned long long m = xm & (dy < 0 ? ym_up[pt] : (dy > 0 ? ym_down[pt] : ~0ull));
                const int row = inb + pt * row_step;
                asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(dst[pt]) : "v"(zrow), "v"(row), "s"(m));
            }
        };
        // the same with edge ranks, for tap v of rank half hh: block pt is slot pt -- in the upper half's dy = +1 taps
        // slots 0 and 1 the other way round, the rank-7 block first (run_tap, SW) -- and its row lies
        // 8 edge_rank(hh, slot) rows behind the lane's file in rank 0: a constant per body.  A rank test there is none:
        // a block is on the board as a whole or it is skipped (its row is then computed and never read).
        auto vtap_rows_edge = [&](auto HC, auto VC, int (&dst)[PT]) {
            constexpr int hh = decltype(HC)::value, v = decltype(VC)::value;
            constexpr int dy = v / 3 - 1, dx = v % 3 - 1, shift = 8 * dy + dx;
            const int zrow = zero_q + ((r_tap + shift) & 15) * G::ZSTRIDE;
            const int inb = base0_tap + shift * G::AROW;
            const unsigned long long m = dx < 0 ? xm_left : (dx > 0 ? xm_right : ~0ull);
#pragma unroll
            for (int pt = 0; pt < PT; pt++) {
                const int slot = (hh == 1 && dy > 0 && pt < 2) ? 1 - pt : pt;
                const int row = inb + 8 * edge_rank(hh, slot) * G::AROW;
                asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(dst[pt]) : "v"(zrow), "v"(row), "s"(m));
            }
        };
        if constexpr (GROUP) {
            constexpr int FR = PT + CT;                 // fragment reads of one sub-step
            half8 fx[3][PT], fw[3][CT];                 // sub-step i lives in buffer i % 3
            const int n_groups = n_tiles / GK;
            for (int g0 = 0; g0 < nv; g0 += GK) {       // virtual taps g0 .. g0+2 = tiles t .. t+2
                const bool more = g0 + GK < nv;         // the layer has another group
                int rows[GK + 1][PT], wb[GK + 1];
#pragma unroll
                for (int k = 0; k <= GK; k++) {
                    vtap_rows(g0 + k < nv ? g0 + k : 0, rows[k]);
                    int slot = slot_tap + k;
                    slot = slot >= GR ? slot - GR : slot;
                    wb[k] = w0 + slot * G::TILE_BYTES;
                }
                // sub-step j of the group (j >= 6: of the next group) -> buffer j % 3
                auto fetch = [&](auto JC) {
                    constexpr int j = decltype(JC)::value, b = j % 3, k = j / 2, pl = j % 2;
#pragma unroll
                    for (int pt = 0; pt < PT; pt++) fx[b][pt] = lds_read16_asm<pl * 64>(rows[k][pt]);
                    static_for<0, CT>([&](auto CC) {
                        constexpr int ct = decltype(CC)::value;
                        fw[b][ct] = lds_read16_asm<ct * 1024 + pl * G::WPLANE>(wb[k]);
                    });
                };
                if (g0 == 0) {                          // cold start of a layer
                    fetch(std::integral_constant<int, 0>{});
                    fetch(std::integral_constant<int, 1>{});
                }
                static_for<0, 2 * GK>([&](auto IC) {
                    constexpr int i = decltype(IC)::value;
                    if constexpr (i == 2 * GK - 2) {
                        // ---- the group's sync, before the first fetch from the next group's tiles:
                        // group tg+1 has landed everywhere, nobody reads group tg-1 any more -> its
                        // slots take group tg + GRG - 1
                        const int tg = t / GK;
                        if (tg + 1 < n_groups) {
                            if (tg + GRG - 2 < n_groups) wait_vmcnt<GK * (GRG - 3)>();   // younger groups stay in flight
                            else wait_vmcnt<0>();
                            __builtin_amdgcn_s_barrier();
                            __builtin_amdgcn_sched_barrier(0);
                            if (!bias_staged) {
                                bias_staged = true;
                                if (conv + 1 < n_convs) stage_bias_x16<G, F>(bias, lds, conv + 1, lane, wave_u);
                            }
                            if (tg + GRG - 1 < n_groups) {
                                int slot = slot_tap - GK;                       // slots of group tg-1
                                slot = slot < 0 ? slot + GR : slot;
#pragma unroll
                                for (int k = 0; k < GK; k++)
                                    stage_wtile_x16<G>(wts, lds, (tg + GRG - 1) * GK + k, tid, wave_u, slot + k);
                            }
                        }
                    }
                    // fetch sub-step i+2 (the last two reach into the next group of this layer)
                    if constexpr (i + 2 < 2 * GK) fetch(std::integral_constant<int, i + 2>{});
                    else if (more) fetch(std::integral_constant<int, i + 2>{});
                    // sub-step i's fragments have landed: at most the younger fetches stay outstanding
                    if constexpr (i + 2 < 2 * GK) wait_lgkm<2 * FR>();
                    else if constexpr (i == 2 * GK - 2) { if (more) wait_lgkm<2 * FR>(); else wait_lgkm<FR>(); }
                    else { if (more) wait_lgkm<2 * FR>(); else wait_lgkm<0>(); }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int pt = 0; pt < PT; pt++)
#pragma unroll
                        for (int ct = 0; ct < CT; ct++)
                            acc[pt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fw[i % 3][ct], fx[i % 3][pt], acc[pt][ct], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                });
                t += GK;
                slot_tap += GK;
                slot_tap = slot_tap >= GR ? slot_tap - GR : slot_tap;
            }
        } else if constexpr (RP) {
            // The nine taps as straight-line code, once per rank half: half 0 skips block 0 in taps 0-2 (dy = -1),
            // half 1 in taps 6-8 (dy = +1).  Whether a tap and its successor skip is then a compile-time property
            // of every body (SK, NSK), the prefetch across the tap boundary stays, and no fragment read is in flight
            // across a join or a back-edge: the two halves meet again behind the last tap's lgkmcnt(0).
            constexpr std::integral_constant<int, 1> once{};
            auto run_conv = [&](auto HC) {
                constexpr int hh = decltype(HC)::value;
                // (the lane's row and file as values the compiler cannot see through, anew for every tap: the row
                // addresses are constants of the kernel, and with the tap a compile-time number hipcc would
                // otherwise compute them all once, ahead of the layer loop, and spill)
                auto fresh = [&] {
                    base0_tap = base0;
                    r_tap = r;
                    asm volatile("" : "+v"(base0_tap), "+v"(r_tap));
                };
                fresh();
                if constexpr (EDGE) vtap_rows_edge(HC, std::integral_constant<int, 0>{}, ab[1]);
                else vtap_rows(0, ab[1]);
                // pieces [P0, P1) of the 2 GL that tiles t+3, t+4 of the recorded sync are, the bias row in front of piece 0
                TrunkDmaSync dma_sync;
                auto dma_pieces = [&](auto P0C, auto P1C) {
                    __builtin_amdgcn_sched_barrier(0);
#if defined(CRL_TRUNK_STAMPS)
                    const unsigned long long s0 = trunk_stamp();
#endif
                    static_for<decltype(P0C)::value, decltype(P1C)::value>([&](auto PC) {
                        constexpr int p = decltype(PC)::value, k = 3 + p / G::GL;
                        if constexpr (p == 0) {
                            if (dma_sync.bias && conv + 1 < n_convs) stage_bias_x16<G, F>(bias, lds, conv + 1, lane, wave_u);
                        }
                        if (dma_sync.t + k < n_tiles)
                            stage_wpiece_x16<G>(wts, lds, dma_sync.t + k, REQ == 2 ? tid + 256 : tid, REQ == 2 ? wave_u + 4 : wave_u,
                                                slot_add(dma_sync.slot, k), p % G::GL);   // (REQ 2: the partner's, from the lower half)
                    });
#if defined(CRL_TRUNK_STAMPS)
                    st_req += trunk_stamp() - s0;
#endif
                    __builtin_amdgcn_sched_barrier(0);
                };
                const RankHalfDma<hh, decltype(dma_pieces)> half{dma_sync, dma_pieces};
                static_for<0, 9>([&](auto VC) {
                    constexpr int v = decltype(VC)::value;
                    // 0 = no block leaves the board, 1 = slot 0 does, 2 = slot 1 does (edge ranks: the upper half's rank 7)
                    constexpr int sk = EDGE ? (hh == 0 ? 0 : (v < 3 ? 1 : (v >= 6 ? 2 : 0))) : ((hh == 0 ? v < 3 : v >= 6) ? 1 : 0);
                    constexpr bool nsk = v + 1 < 9 && (EDGE ? hh == 1 && (v + 1 < 3 || v + 1 >= 6) : (hh == 0 ? v + 1 < 3 : v + 1 >= 6));
#pragma unroll
                    for (int pt = 0; pt < PT; pt++) ab[0][pt] = ab[1][pt];
                    fresh();
                    if constexpr (EDGE) vtap_rows_edge(HC, std::integral_constant<int, (v + 1 < 9 ? v + 1 : 0)>{}, ab[1]);
                    else vtap_rows(v + 1 < 9 ? v + 1 : 0, ab[1]);
                    run_tap(std::integral_constant<int, 4>{}, once, v == 0, v == 8, std::integral_constant<int, sk>{},
                            std::integral_constant<bool, nsk>{}, half);
                    slot_tap = slot_add(slot_tap, 4 / G::SPT);
                });
            };
            if (rp_half == 0) run_conv(std::integral_constant<int, 0>{});
            else run_conv(std::integral_constant<int, 1>{});
        } else {
        constexpr std::false_type nsk{};
        constexpr std::integral_constant<int, 0> nh{};  // no rank halves: one body
        vtap_rows(0, ab[1]);
        for (int v = 0; v < nv; v++) {
#pragma unroll
            for (int pt = 0; pt < PT; pt++) ab[0][pt] = ab[1][pt];
            vtap_rows(v + 1 < nv ? v + 1 : 0, ab[1]);
            constexpr std::integral_constant<int, 1> once{};
            bool whi_twice = false;                     // SPLIT, part 0 of a residual conv: Whi against hi and lo
            if constexpr (SPLIT) {
                const bool whi = ((v % per_tap) >> hshift) == 0;         // part 0
                whi_twice = conv != 0 && whi;
            }
            if (whi_twice) {
                if constexpr (SPLIT) {
                    constexpr std::integral_constant<int, 2> twice{};
                    if (F == 64) run_tap(std::integral_constant<int, 4>{}, twice, v == 0, v == nv - 1, nsk, nsk, nh);
                    else run_tap(std::integral_constant<int, 8>{}, twice, v == 0, v == nv - 1, nsk, nsk, nh);
                }
            } else if (F == 64 && conv != 0) run_tap(std::integral_constant<int, 2>{}, once, v == 0, v == nv - 1, nsk, nsk, nh);
            else run_tap(std::integral_constant<int, 4>{}, once, v == 0, v == nv - 1, nsk, nsk, nh);
            if constexpr (PAIR) slot_tap = slot_add(slot_tap, 4 / G::SPT);
            // The fragments prefetched for the next tap are in flight across this loop's back-edge, where
            // hipcc -- which cannot see the inline-asm reads -- is free to COPY their registers (phi moves)
            // before the data has landed.  It does so in the split kernels, whose tap loop has several
            // bodies (found in the 64-filter ones as run-to-run differences once a second process delayed
            // the LDS returns); there the reads are drained here.  tools/check_asm_hazards.py walks the ISA of every trunk kernel for such reads and is
            // run by tests/test_host_and_cabi.py on every build.
            if constexpr (SPLIT) wait_lgkm<0>();
        }
        }

        // ---- epilogue ------------------------------------------------------------------------------
        wait_lgkm<0>();
        __builtin_amdgcn_s_barrier();                   // all reads of the activation buffer done
        __builtin_amdgcn_sched_barrier(0);
        // two wave-uniform shapes (branches, not selects: every VALU instruction competes with the
        // partner wave's MFMAs for issue slots): conv1 = ReLU, skip stream untouched; conv2 = + skip, ReLU, new
        // skip.  The stem (linear: no BN, no activation, model.py:33-34) runs as a conv2 whose skip stream is
        // still -0 and whose floor is -inf: max(acc + -0, -inf) is acc bit for bit, the sign of a zero and fp32
        // denormals (kept in this build) included; only a NaN accumulator would come out as -inf.
        // Two shapes, not three, because of the registers: with a branch of its own for the stem hipcc joins the
        // loop-carried res and the retired acc through chains of phi copies -- 192 v_mov_b32 per wave in a conv1
        // hand-over, 64 in a conv2's, MFMA pipe idle.  tests/test_trunk_handover_cpu.py holds the ISA to none.
        const bool conv1 = (conv & 1) != 0;
        const float floor = conv == 0 ? -__builtin_inff() : 0.f;
        // channel blocks 2g, 2g+1 of a position block: 8 consecutive channels per lane, one 16-byte write
        auto store_pair = [&](int pt, int g, const half4 &lo, const half4 &hi) {
            *reinterpret_cast<__attribute__((address_space(3))) half8 *>(
                lds + act_row0 + slot_row(pt) + (obase + 32 * g + 8 * q) * 2) =
                half8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        };
        const half4 zero4 = {(_Float16)0, (_Float16)0, (_Float16)0, (_Float16)0};
        // SPLIT: the value goes back as hi = fp16(v) and lo = fp16(v - hi), lo LO_OFF bytes further
        auto store_split = [&](int pt, int g, const f32x4v &a, const f32x4v &b) {
            half8 hi8, lo8;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                hi8[j] = (_Float16)a[j];
                hi8[4 + j] = (_Float16)b[j];
                lo8[j] = (_Float16)(a[j] - (float)hi8[j]);
                lo8[4 + j] = (_Float16)(b[j] - (float)hi8[4 + j]);
            }
            lds_byte *dst = lds + act_row0 + slot_row(pt) + (obase + 32 * g + 8 * q) * 2;
            *reinterpret_cast<__attribute__((address_space(3))) half8 *>(dst) = hi8;
            *reinterpret_cast<__attribute__((address_space(3))) half8 *>(dst + G::LO_OFF) = lo8;
        };
        if constexpr (SPLIT) {
            // the branch encloses the loops (taken per element it leaves phi copies of res behind each one), and
            // the two sides end in unequal asm comments: hipcc otherwise merges their last tile's stores into one
            // tail and copies res into the tail's registers
            auto write_layer = [&](auto value) {
#pragma unroll
                for (int g = 0; g < CT / 2; g++)
#pragma unroll
                    for (int pt = 0; pt < PT; pt++) store_split(pt, g, value(pt, 2 * g), value(pt, 2 * g + 1));
            };
            if (conv1) {                                // conv1: ReLU
                write_layer([&](int pt, int ct) {
                    f32x4v o;
#pragma unroll
                    for (int j = 0; j < 4; j++) o[j] = fmaxf(acc[pt][ct][j], 0.f);
                    return o;
                });
                asm volatile("; conv1 written");
            } else {                                    // conv2: + skip, ReLU, new skip; stem: + -0, floor -inf
                write_layer([&](int pt, int ct) {
                    const f32x4v sum = acc[pt][ct] + res[pt][ct];
#pragma unroll
                    for (int j = 0; j < 4; j++) res[pt][ct][j] = fmaxf(sum[j], floor);
                    return res[pt][ct];
                });
                asm volatile("; conv2 written");
            }
        } else
        if (conv1) {                                    // conv1 of a block: ReLU, skip stream untouched
#pragma unroll
            for (int g = 0; g < CT / 2; g++)
#pragma unroll
                for (int pt = 0; pt < PT; pt++) {
                    half4 o16[2];                        // convert, then ReLU on packed halves
#pragma unroll
                    for (int h = 0; h < 2; h++) {
#pragma unroll
                        for (int j = 0; j < 4; j++) o16[h][j] = (_Float16)acc[pt][2 * g + h][j];
                        o16[h] = __builtin_elementwise_max(o16[h], zero4);
                    }
                    store_pair(pt, g, o16[0], o16[1]);
                }
        } else {                                        // conv2: + skip, ReLU, new skip; stem: + -0, floor -inf
#pragma unroll
            for (int g = 0; g < CT / 2; g++)
#pragma unroll
                for (int pt = 0; pt < PT; pt++) {
                    half4 o16[2];
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const int ct = 2 * g + h;
                        const f32x4v sum = acc[pt][ct] + res[pt][ct];      // packed fp32 adds
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const float v = fmaxf(sum[j], floor);
                            res[pt][ct][j] = v;
                            o16[h][j] = (_Float16)v;
                        }
                    }
                    store_pair(pt, g, o16[0], o16[1]);
                }
        }
        wait_lgkm<0>();
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    }
#if defined(CRL_TRUNK_STAMPS)
    if constexpr (RP) {
        const unsigned long long st_loop = trunk_stamp() - st_t0;
        unsigned long long *dbg = crl_trunk_stamp_buf;
        if (lane == 0 && dbg) {
            dbg += ((size_t)blockIdx.x * 8 + wave_u) * 5;
            dbg[0] = st_loop; dbg[1] = st_wait; dbg[2] = st_req; dbg[3] = st_syncs; dbg[4] = st_self;
        }
    }
#endif
    if (!IDX && out) {
#pragma unroll
        for (int pt = 0; pt < PT; pt++) {
            const int p = pos0 + slot_pos(pt);
#pragma unroll
            for (int ct = 0; ct < CT; ct++) {
                const int o0 = obase + G::chan_of(ct, 0) + 8 * q;
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; j++) v[j] = res[pt][ct][j];
                *reinterpret_cast<f32x4 *>(out + ((wg_board0 + board) * 64 + p) * F + o0) = v;
            }
        }
    }

    if (head_out) {
        // a position's F channels live in CG waves x 4 lane quarters: 4*CG partial sums per output,
        // added in a fixed order (no float atomics: results are reproducible)
        constexpr int NC = 4 * G::CG;
        float part[PT][3];
#pragma unroll
        for (int pt = 0; pt < PT; pt++)
#pragma unroll
            for (int k = 0; k < 3; k++) part[pt][k] = 0.f;
#pragma unroll
        for (int ct = 0; ct < CT; ct++) {
            const int o0 = obase + G::chan_of(ct, 0) + 8 * q;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const f32x4 wv = *reinterpret_cast<const f32x4 *>(head_w + k * F + o0);
#pragma unroll
                for (int pt = 0; pt < PT; pt++)
#pragma unroll
                    for (int j = 0; j < 4; j++) part[pt][k] += res[pt][ct][j] * wv[j];
            }
        }
        __attribute__((address_space(3))) float *scratch = (__attribute__((address_space(3))) float *)lds;
#pragma unroll
        for (int pt = 0; pt < PT; pt++)
#pragma unroll
            for (int k = 0; k < 3; k++)
                scratch[(((board * 64 + pos0 + slot_pos(pt)) * 3) + k) * NC + (obase / (16 * CT)) * 4 + q] = part[pt][k];
        wait_lgkm<0>();
        __builtin_amdgcn_s_barrier();
        for (int i = tid; i < G::NB * 64 * 3; i += 512) {
            const int k = i % 3, bp = i / 3;
            float v = 0.f;
#pragma unroll
            for (int c = 0; c < NC; c++) v += scratch[i * NC + c];      // fixed order
            v += head_b[k];
            size_t gb = wg_board0 + (bp >> 6);
            if constexpr (IDX) {
                gb = (size_t)rows[0];
#pragma unroll
                for (int b = 1; b < G::NB; b++) gb = (bp >> 6) == b ? (size_t)rows[b] : gb;
            }
            const int pos = bp & 63;
            head_out[gb * 192 + (k < 2 ? pos * 2 + k : 128 + pos)] = fmaxf(v, 0.f);
        }
    }
}

}  // namespace crl_tower
