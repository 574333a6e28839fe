// rollout.hpp -- random playouts on the device: RandomSimulation.run (simulation.py:19-34), the leaf
// evaluator SelfPlayTree.simulate names as its alternative to predict_outcome (mctree.py:272-274).
//
// One wavefront plays one playout (lane = square, as everywhere in search.hpp).  Each ply, in this order:
// wave_movegen, the derived en-passant bit and the hash (as eval_position), the repetition count,
// position_result (every rule of Game.get_result, the fifty-move claim at clock >= 100 included) and -- if
// there is no result and the ply budget is not spent -- the choice of a move and apply_move.
//
// THE CHOICE RULE is CPython's random.choice(moves) = moves[_randbelow(n)], word for word:
//     k = bit_length(n)                       (n <= 218, so k <= 8)
//     repeat: w = next 32-bit word; r = w >> (32 - k)        until r < n
//     the move is mv[r], python-chess generation order
// Every word taken counts as consumed, the rejected ones included.
//
// TWO FORMS share that ply.
//
// k_rollout_games (in-slot, the drop-in semantics): the playout IS the game of the slot, pushed ply by ply
// through game_push (history ring, move record, ply count, result).  Words come from a host-supplied
// uint32 row per slot (one MT19937 output per word is what _randbelow consumes for k <= 32).  It stops when
// the game has a result, when chunks * max_moves plies have been played since the run began, or when the
// words run out -- then the slot is simply a shorter game and the caller resumes with the following words
// (a choice whose words ran out has moved nothing: rejection sampling has no memory).
//
// k_rollout (private, the fast path): count * repetitions independent playouts; nothing of the game state is
// written.  The position lives in registers; the repetition window lives in LDS: a ring of ROLL_RING = 128
// (hash, board) pairs indexed by the playout ply t & 127 (t = 0 is the root, t < 0 its history).  A game that
// goes on has clock < 100 and count_prior looks back `clock` plies, so at most 99 earlier plies matter; a
// position with clock >= 100 is decided by position_result without its count (the claim, or no legal move).
// The root's own reversible history (min(clock, 99) plies, as far as it exists) is copied in once, from the
// game ring or through past_ref from the tree path.  Entries are whole boards compared with same_key behind
// the hash filter: as exact as count_prior.  512 B of moves + 128 * 72 B = 9.5 KiB of LDS per wave.
// A playout still running after max_moves plies is a draw (0), what simulation.py:30-31 intends.
//
// WORDS OF THE PRIVATE FORM: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as
// 1, 2, 3", SC'11), stateless.  One call maps a 128-bit counter (c0, c1, c2, c3) and a 64-bit key (k0, k1) to
// four 32-bit words:
//     ten rounds; before every round but the first  k0 += 0x9E3779B9, k1 += 0xBB67AE85  (mod 2^32);
//     one round:  hi0:lo0 = 0xD2511F53 * c0,  hi1:lo1 = 0xCD9E8D57 * c2   (32 x 32 -> 64 bit products)
//                 (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0)
//     the output is (c0, c1, c2, c3) after the tenth round.
// Key and counter of draw number i (0, 1, 2, ... in the order the choice rule takes words) of a playout:
//     k0 = low 32 bits, k1 = high 32 bits of the slot's 64-bit stream key (a device array the caller owns)
//     c0 = i >> 2          and the word is output number i & 3 of that call
//     c1 = repetition      (0-based)
//     c2 = 0-based index of the simulation within the current search (0 for roots taken from the games)
//     c3 = game ply of the playout's root position (len(game) there)
#pragma once
#include "search.hpp"

namespace crl {

constexpr int ROLL_RING = 128;
constexpr u16 ROLL_SKIPPED = 0xFFFF;       // plies[] of a slot that had no playout to run

struct RollLds {
    u16 mv[MAX_MOVES];
    u64 rh[ROLL_RING];
    Board rb[ROLL_RING];
};

struct Philox4 { u32 w[4]; };

__host__ __device__ inline Philox4 philox4x32_10(u32 c0, u32 c1, u32 c2, u32 c3, u32 k0, u32 k1)
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
        const u32 n0 = (u32)(p1 >> 32) ^ c1 ^ k0, n2 = (u32)(p0 >> 32) ^ c3 ^ k1;
        c1 = (u32)p1; c3 = (u32)p0; c0 = n0; c2 = n2;
    }
    Philox4 o;
    o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
    return o;
}

// earlier occurrences of b among the playout plies t-2, t-4, ... (count_prior over the LDS window);
// `lo` = playout ply of the oldest entry the window holds
__device__ inline int ring_count(const RollLds &s, const Board &b, u64 h, int t, int lo, int lane)
{
    const int clock = (int)st_clock(b.state);
    if (clock < 8 || clock >= 100) return 0;          // (>= 100: position_result does not read the count)
    const int dist = 2 * (lane + 1);                    // clock <= 99: distances 2 .. 98, one pass
    bool hit = false;
    if (dist <= clock && t - dist >= lo) {
        const int i = (t - dist) & (ROLL_RING - 1);
        if (s.rh[i] == h) hit = same_key(s.rb[i], b);
    }
    return popc(__ballot(hit));
}

// from_leaves = 0: the root of row r is the current position of slot g0 + r; 1: the S2 of its pending leaf.
// block = row * reps + repetition.  results[block] = the playout's result, plies[block] = plies played
// (ROLL_SKIPPED and result 0 where the slot has no playout to run).
__global__ __launch_bounds__(64) void k_rollout(Dev d, int from_leaves, int reps, int max_moves, const u64 *keys,
                                                int8_t *results, u16 *plies)
{
    __shared__ RollLds s;
    const int r = blockIdx.x / reps, rep = blockIdx.x - r * reps, g = r + d.g0, lane = threadIdx.x;
    const int p = uni(d.game[g].ply);
    Board b;
    int tp = 0, sim = 0;
    bool run = true;
    if (from_leaves) {
        const int kind = uni(d.game[g].leaf_kind);
        run = !uni(d.game[g].root_dead) && kind == LEAF_NEW_S2;
        if (run) {
            const size_t ni = (size_t)g * d.N + uni(d.game[g].leaf_node);
            run = uni(d.node[ni].meta.result) == RESULT_NONE;
            b = d.node[ni].s2;
            tp = 2 * uni(d.game[g].path_len);
            sim = uni(d.game[g].root_visits) - 1;
        }
    } else {
        b = d.cur[g];
    }
    if (!run) {
        if (lane == 0) { results[blockIdx.x] = 0; plies[blockIdx.x] = ROLL_SKIPPED; }
        return;
    }
    // the root's reversible history, as far as it exists
    const int clock0 = (int)st_clock(b.state);
    int K = clock0 < 99 ? clock0 : 99;
    const int have = tp + (p < HIST_RING - 1 ? p : HIST_RING - 1);
    if (K > have) K = have;
    for (int k = lane + 1; k <= K; k += 64) {
        PastRef pr = past_ref(d, g, tp - k, p, p);
        s.rb[(-k) & (ROLL_RING - 1)] = *pr.b;
        s.rh[(-k) & (ROLL_RING - 1)] = *pr.h;
    }
    const int lo = -K;
    const u64 key = keys[r];
    const u32 k0 = (u32)key, k1 = (u32)(key >> 32);
    u32 draw = 0;
    Philox4 px = philox4x32_10(0, (u32)rep, (u32)sim, (u32)(p + tp), k0, k1);
    __syncthreads();

    int t = 0, result;
    for (;;) {
        MoveGenInfo mi = wave_movegen(b, lane, s.mv);
        b.state = (b.state & ~(1u << 20)) | ((mi.ep_legal ? 1u : 0u) << 20);
        const u64 h = board_hash(b);
        const int rc = 1 + ring_count(s, b, h, t, lo, lane);
        result = position_result(b, mi.n, mi.in_check, rc);
        __syncthreads();                                   // s.mv visible; the window was read
        if (result != RESULT_NONE) break;
        if (t >= max_moves) { result = 0; break; }         // still running: a draw (simulation.py:30-31)
        if (lane == 0) { s.rb[t & (ROLL_RING - 1)] = b; s.rh[t & (ROLL_RING - 1)] = h; }
        const int n = uni(mi.n);
        const int kbits = 32 - __builtin_clz((u32)n);
        u32 x;
        do {
            const u32 i = draw & 3u;
            if (draw && i == 0) px = philox4x32_10(draw >> 2, (u32)rep, (u32)sim, (u32)(p + tp), k0, k1);
            const u32 w = i == 0 ? px.w[0] : i == 1 ? px.w[1] : i == 2 ? px.w[2] : px.w[3];
            draw++;
            x = w >> (32 - kbits);
        } while (x >= (u32)n);
        const u32 mv = s.mv[x];
        __syncthreads();                                   // s.mv read before the next ply rewrites it
        b = apply_move(b, mv);
        t++;
    }
    if (lane == 0) { results[blockIdx.x] = (int8_t)result; plies[blockIdx.x] = (u16)t; }
}

// value[row] = (float)((double)sum of the row's results / reps): integer sum, one rounding chain
__global__ __launch_bounds__(64) void k_rollout_mean(const int8_t *results, int reps, float *value)
{
    const int r = blockIdx.x, lane = threadIdx.x;
    int sum = 0;
    for (int i = lane; i < reps; i += 64) sum += results[(size_t)r * reps + i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) value[r] = (float)__ddiv_rn((double)sum, (double)reps);
}

// The in-slot form.  words[r][0 .. nwords[r]) are the words of row r; played[r] (in/out) = plies played since
// the run began, used[r] = words consumed by this launch, chunk_res[r][c] = Game.get_result() after chunk c
// (plies (c+1) * max_moves of the run): RESULT_NONE where the game went on past that ply, else the result now.
__global__ __launch_bounds__(64) void k_rollout_games(Dev d, const u32 *words, const int32_t *nwords, int stride,
                                                      int chunks, int max_moves, int32_t *played, int32_t *used,
                                                      int8_t *chunk_res)
{
    __shared__ WaveLds s;
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    const int total = chunks * max_moves;
    const int nw = nwords[r] < stride ? nwords[r] : stride;
    int p = played[r], u = 0;
    for (;;) {
        if (uni(d.game[g].game_result) != RESULT_NONE || p >= total) break;
        Board b = d.cur[g];
        MoveGenInfo mi = wave_movegen(b, lane, s.mv);
        __syncthreads();
        const int n = uni(mi.n);
        if (n < 1) break;                                  // (a running game has a legal move)
        const int kbits = 32 - __builtin_clz((u32)n);
        int pick = -1;
        while (u < nw) {
            const u32 x = words[(size_t)r * stride + u] >> (32 - kbits);
            u++;
            if (x < (u32)n) { pick = (int)x; break; }
        }
        if (pick < 0) break;                               // out of words: the caller resumes
        const u32 mv = s.mv[pick];
        __syncthreads();
        game_push(d, g, b, mv, lane, s);
        __threadfence_block();                             // lane 0 wrote cur / ply / result: the next ply reads them
        __syncthreads();
        p++;
    }
    const int res = uni(d.game[g].game_result);
    for (int c = lane; c < chunks; c += 64)
        chunk_res[(size_t)r * chunks + c] = (int8_t)((long long)(c + 1) * max_moves < p ? RESULT_NONE : res);
    if (lane == 0) { played[r] = p; used[r] = u; }
}

}  // namespace crl
