// search.hpp -- device kernels of the lockstep self-play simulation loop.
//
// One 64-lane wavefront (one 64-thread workgroup) per game.  Reference symbols
// (paths relative to /root/reference/src/chessrl/):
//
//   k_search_begin     Tree.__init__                          mctree.py:105-111
//   k_root_priors      _update_prior for the root             mctree.py:298-303
//   k_select_expand    backprop (pending) + select + expand   mctree.py:216-257,278-296
//   k_reply            opponent reply half of expand, Node()  mctree.py:244-250,28-37
//   k_backup           simulate + backprop + child priors     mctree.py:259-303
//   k_root_children    [c.visits for c in root.children]      mctree.py:178,313-315
//   k_advance          gam.move(bm); gam.move(am)             selfplay.py:77-78
//   k_advance_one      gam.move(bm) alone                     gameagent.py, benchmark.py:100-118
//   k_choose_advance_one  argmax of compute_policy + gam.move(bm)   gameagent.py, mctree.py:305-322
//   k_encode_cur       netencoder.get_game_state             netencoder.py:72-91
//   k_legal/k_push/... Game.get_legal_moves/move/get_result   game.py:28-57,92-109
//   k_greedy           AgentDistributed.best_move(real_game)  agentdistributed.py:56-58
//
// The pieces of a simulation are device functions, each defined once here and called by the one-leaf kernels above
// and by the wave schedule (search_wave.hpp); a schedule decides only where a leaf is kept and in which order:
//   best_child         Node.get_value / get_best_child        mctree.py:71-95
//   descent_step       one level of select                    mctree.py:216-231
//   expand_child       expand, our move                       mctree.py:231-243
//   reply_child        expand, the opponent's reply; Node()   mctree.py:244-250,28-37
//   backup_leaf        simulate + backprop + child priors     mctree.py:259-303
//
// Float contract of get_value (mctree.py:71-87), reproduced with explicit
// round-to-nearest intrinsics (and the file is built with -ffp-contract=off):
//   Q = value / (1 + visits)                       float64 divide
//   U = (10 * prior) * (sqrt(sum) / (1 + visits))  10*prior in float32 (numpy>=2) or
//                                                  float64 (numpy 1.x flag); rest float64
//   sum = visits of the child's own children = visits-1 (0 for a terminal child), which
//   is exact in sequential mode: every simulation through a non-terminal node after the
//   one that created it visits exactly one of its children.
#pragma once
#include "movegen.hpp"
#include "slices.hpp"
#include "state.hpp"

namespace crl {

struct WaveLds {
    u16 mv[MAX_MOVES];
    Board enc[9];
    u64 pl[PLANES];
};

__device__ inline int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }

// ---- where does the position `tp` tree-plies after the root live? -------------------------
// tp >= 1: node path_node[(tp+1)/2], S1 if tp is odd else S2.  tp <= 0: game history ring
// at ply ply0 + tp, where ply0 is the game ply of tree-ply 0.
struct PastRef { const Board *b; const u64 *h; bool valid; };

__device__ inline PastRef past_ref(const Dev &d, int g, int tp, int ply0, int ply_ring_top)
{
    PastRef r;
    if (tp >= 1) {
        int node = d.path_node[(size_t)g * d.N + ((tp + 1) >> 1)];
        size_t ni = (size_t)g * d.N + node;
        r.b = (tp & 1) ? &d.node[ni].s1 : &d.node[ni].s2;
        r.h = (tp & 1) ? &d.node[ni].h1 : &d.node[ni].h2;
        r.valid = true;
    } else {
        int p = ply0 + tp;
        r.valid = p >= 0 && p > ply_ring_top - HIST_RING && p <= ply_ring_top;
        size_t hi = (size_t)g * HIST_RING + (p & (HIST_RING - 1));
        r.b = d.hist + hi;
        r.h = d.hist_hash + hi;
    }
    return r;
}

// earlier occurrences of position b (python-chess is_repetition: same _transposition_key),
// looking back over the reversible plies only; lanes test distances 2,4,6,... in parallel
__device__ inline int count_prior(const Dev &d, int g, const Board &b, u64 h, int tp, int ply0,
                                  int ring_top, int lane)
{
    const int clock = (int)st_clock(b.state);
    int cnt = 0;
    if (clock < 8) return 0;                 // a 5th occurrence needs >= 8 reversible plies
    for (int base = 0; 2 * (base + 1) <= clock; base += 64) {
        const int dist = 2 * (base + lane + 1);
        bool hit = false;
        if (dist <= clock) {
            PastRef r = past_ref(d, g, tp - dist, ply0, ring_top);
            if (r.valid && *r.h == h) {
                Board o = *r.b;
                hit = same_key(o, b);
            }
        }
        cnt += popc(__ballot(hit));
    }
    return cnt;
}

struct PosEval { Board b; u64 hash; int n; int result; };

// legal moves (into s.mv), derived ep bit, hash, repetition and Game.get_result of `b`
__device__ inline PosEval eval_position(const Dev &d, int g, Board b, int tp, int ply0,
                                        int ring_top, int lane, WaveLds &s)
{
    MoveGenInfo mi = wave_movegen(b, lane, s.mv);
    b.state = (b.state & ~(1u << 20)) | ((mi.ep_legal ? 1u : 0u) << 20);
    PosEval e;
    e.hash = board_hash(b);
    int rep = 1 + count_prior(d, g, b, e.hash, tp, ply0, ring_top, lane);
    e.result = position_result(b, mi.n, mi.in_check, rep);
    e.n = mi.n;
    e.b = b;
    __syncthreads();                          // s.mv visible to every lane
    return e;
}

// ---- netencoder.get_game_state (netencoder.py:13-91) -> fp16 NHWC [8][8][128] ----------------
// Channels: 0-6 black {no black piece here, P,N,B,R,Q,K}, 7-13 white likewise, then the same
// 14 planes for each of the 8 previous positions (zeros where the move stack is shorter),
// 126 = side to move is white, 127 = zero pad.  Row 0 = rank 8: spatial index = sq ^ 56.
// Lane l always owns channel group l&15, so its 8 plane bitboards stay in registers; each of the
// 16 store iterations writes one contiguous 1 KiB per wave.
__device__ inline void encode_position(const Dev &d, int g, const Board &b, int tp, int ply0,
                                       int ring_top, int lane, WaveLds &s, void *planes_out, int row)
{
    bool valid = false;
    if (lane < 9) {
        Board e = b;
        valid = true;
        if (lane > 0) {
            PastRef r = past_ref(d, g, tp - lane, ply0, ring_top);
            valid = r.valid;
            if (valid) e = *r.b;
        }
        s.enc[lane] = e;
    }
    const u32 vmask = (u32)__ballot(valid);
    __syncthreads();
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int c = lane + 64 * half;
        u64 v = 0;
        if (c < 126) {
            const int i = c / 14, k = c % 14, t = k % 7;
            const Board &e = s.enc[i];
            const u64 occ = occupied(e);
            const u64 own = k >= 7 ? e.white : (occ & ~e.white);
            if ((vmask >> i) & 1) v = t == 0 ? ~own : (e.bb[t - 1] & own);
        } else if (c == 126) {
            v = st_turn(b.state) ? ~0ull : 0ull;
        }
        s.pl[c] = v;
    }
    __syncthreads();
    if (d.plane_fmt) {
        // compact form for the fused trunk (crl_trunk_forward_bitplanes): the 128 plane bitboards,
        // 1 KiB per position instead of 16 KiB; the trunk kernel expands them into LDS itself
        u64 *bits = (u64 *)planes_out + (size_t)row * PLANES;
        bits[lane] = s.pl[lane];
        bits[lane + 64] = s.pl[lane + 64];
        __syncthreads();
        return;
    }
    const int cg = lane & 15;
    u64 p8[8];
#pragma unroll
    for (int k = 0; k < 8; k++) p8[k] = s.pl[cg * 8 + k];
    // (not unrolled: sixteen loop-invariant 64-bit store addresses, hoisted to the top of
    // k_select_expand, were what spilled 28 VGPRs there)
    uint4 *out = (uint4 *)planes_out + (size_t)row * (64 * PLANES * 2 / 16);
#pragma unroll 1
    for (int t = 0; t < 16; t++) {
        const int sq = (t * 4 + (lane >> 4)) ^ 56;
        u32 w[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            w[k] = (((p8[2 * k] >> sq) & 1) ? 0x3C00u : 0u) |
                   (((p8[2 * k + 1] >> sq) & 1) ? 0x3C000000u : 0u);
        out[t * 64 + lane] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    __syncthreads();
}

// ---- shared pieces ---------------------------------------------------------------------------
__device__ inline void dev_error(const Dev &d, int code)
{
    atomicCAS(d.err, 0, code);
}

// Descent hint kept in the spare word of an edge record.  get_best_child needs, of the node it descends
// into, the slot of its edge records and their number -- both in that node's own record, i.e. behind a
// second dependent HBM read per tree level.  Once a node is fully expanded (from then on select only ever
// scans it, mctree.py:216-231) those two numbers are frozen, so they are copied into the parent's edge
// record, which the scan of the level above has just read: one dependent read per level instead of two.
constexpr u32 HINT_FULL = 1u << 31;
constexpr int HINT_EDGE_BITS = 23;                 // edge slots per game < 2^23 (38 000 simulations per move)
constexpr int HINT_EDGE_CAP = 1 << HINT_EDGE_BITS;
__device__ inline u32 hint_pack(int edge0, int nmoves) { return HINT_FULL | ((u32)nmoves << HINT_EDGE_BITS) | (u32)edge0; }
__device__ inline int hint_edge0(u32 hint) { return (int)(hint & ((1u << HINT_EDGE_BITS) - 1)); }
__device__ inline int hint_nmoves(u32 hint) { return (int)((hint >> HINT_EDGE_BITS) & 0xFFu); }
static_assert(MAX_BRANCH < 256, "nmoves fits the hint");

__device__ inline void init_edges(const Dev &d, size_t eb, int edge0, int n, const u16 *mv, int lane)
{
    for (int j = lane; j < n; j += 64) {
        Edge e;
        e.value = 0.0; e.visits = 0;
        e.prior = 1.0f;                      // Node.prior = 1 (mctree.py:35)
        e.move = mv[j]; e.child = CHILD_NONE; e.pad = 0;
        d.edge[eb + edge0 + j] = e;
    }
}

// fmt = CRL_POLICY_FULL: pol is a full policy[row][1968], gathered at the labels of the node's moves;
// fmt = CRL_POLICY_LEGAL: pol is priors[row][MAX_MOVES], entry j for the node's legal move j (the evaluator
// gathered them from the label list the search kernel that created the position wrote);
// fmt = CRL_POLICY_LEGAL_RAW: the same rows holding LOGITS; `stats` are the board's slice statistics and
// the probability is formed here (csrc/slices.hpp: the arithmetic of the normalising pass, same bits)
constexpr int FMT_FULL = 0, FMT_LEGAL = 1, FMT_LEGAL_RAW = 2;

__device__ inline void gather_priors(const Dev &d, int row, size_t eb, int edge0, int n,
                                     const float *pol, int lane, int fmt, const float2 *stats = nullptr)
{
    if (fmt == FMT_LEGAL_RAW) {
        const crl_slices::Norm nm = crl_slices::norm_of(stats + (size_t)row * crl_slices::N_SLICES);
        for (int j = lane; j < n; j += 64)
            d.edge[eb + edge0 + j].prior = crl_slices::prob(pol[(size_t)row * MAX_MOVES + j], nm);
        return;
    }
    const bool legal = fmt == FMT_LEGAL;
    for (int j = lane; j < n; j += 64) {
        size_t e = eb + edge0 + j;
        if (legal) {
            d.edge[e].prior = pol[(size_t)row * MAX_MOVES + j];
            continue;
        }
        int lab = label_of(d, d.edge[e].move);
        if (lab >= N_LABELS) { dev_error(d, DERR_LABEL); lab = 0; }
        d.edge[e].prior = pol[(size_t)row * N_LABELS + lab];
    }
}

// labels of the n moves in mv -> lab[row][0..n), count[row] = n (the evaluator's gather list)
__device__ inline void write_labels(const Dev &d, int row, const u16 *mv, int n, u16 *lab, int32_t *count, int lane)
{
    for (int i = lane; i < n; i += 64) {
        int l = label_of(d, mv[i]);
        if (l >= N_LABELS) { dev_error(d, DERR_LABEL); l = 0; }
        lab[(size_t)row * MAX_MOVES + i] = (u16)l;
    }
    if (lane == 0) count[row] = n;
}

// index of the first maximum of policy[label(m)] over the n moves in mv (np.argmax)
__device__ inline int argmax_policy(const Dev &d, int row, const u16 *mv, int n, const float *pol,
                                    int lane, int fmt, const float2 *stats = nullptr)
{
    float best = -__builtin_inff();
    int bi = 0x7FFFFFFF;
    crl_slices::Norm nm = {0.f, 0.f};
    if (fmt == FMT_LEGAL_RAW) nm = crl_slices::norm_of(stats + (size_t)row * crl_slices::N_SLICES);
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        if (i < n) {
            float p;
            if (fmt == FMT_LEGAL_RAW) {
                // the argmax runs over the PROBABILITIES the normalising pass would have stored (two
                // logits may round to one probability; np.argmax then takes the first)
                p = crl_slices::prob(pol[(size_t)row * MAX_MOVES + i], nm);
            } else if (fmt == FMT_LEGAL) {
                p = pol[(size_t)row * MAX_MOVES + i];
            } else {
                int lab = label_of(d, mv[i]);
                if (lab >= N_LABELS) { dev_error(d, DERR_LABEL); lab = 0; }
                p = pol[(size_t)row * N_LABELS + lab];
            }
            if (p > best || bi == 0x7FFFFFFF) { best = p; bi = i; }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        float ob = __shfl_xor(best, o);
        int oi = __shfl_xor(bi, o);
        bool take = oi != 0x7FFFFFFF && (bi == 0x7FFFFFFF || ob > best || (ob == best && oi < bi));
        if (take) { best = ob; bi = oi; }
    }
    return bi;
}

// push a legal move onto the game (python-chess Board.push + result bookkeeping)
__device__ inline void game_push(const Dev &d, int g, const Board &b, u32 mv, int lane, WaveLds &s)
{
    const int p = d.game[g].ply;
    Board nb = apply_move(b, mv);
    PosEval e = eval_position(d, g, nb, 0, p + 1, p, lane, s);
    if (lane == 0) {
        if (p + 1 > d.MAXPLY) { dev_error(d, DERR_PLY_POOL); }
        else {
            size_t hi = (size_t)g * HIST_RING + ((p + 1) & (HIST_RING - 1));
            d.hist[hi] = e.b;
            d.hist_hash[hi] = e.hash;
            d.rec_moves[(size_t)g * d.MAXPLY + p] = (u16)mv;
            d.cur[g] = e.b;
            d.game[g].ply = p + 1;
            d.game[g].game_result = (int8_t)e.result;
            d.game[g].root_dead = 1;
        }
    }
}

// ---- Game seam kernels -------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_set_positions(Dev d, const Board *in, const uint8_t *mask,
                                                      int n, int use_start)
{
    __shared__ WaveLds s;
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    if (r >= n || (mask && !mask[r])) return;
    Board b;
    if (use_start) {
        b.bb[PAWN] = 0x00FF00000000FF00ull; b.bb[KNIGHT] = 0x4200000000000042ull;
        b.bb[BISHOP] = 0x2400000000000024ull; b.bb[ROOK] = 0x8100000000000081ull;
        b.bb[QUEEN] = 0x0800000000000008ull; b.bb[KING] = 0x1000000000000010ull;
        b.white = 0xFFFFull;
        b.state = mk_state(1, 15, NO_EP, 0, 0);
        b.pad = 0;
    } else {
        b = in[r];
        b.state &= 0xFFFFFu;
        b.pad = 0;
    }
    if (lane == 0) d.game[g].ply = 0;
    PosEval e = eval_position(d, g, b, 0, 0, -1, lane, s);
    if (lane == 0) {
        d.cur[g] = e.b;
        d.hist[(size_t)g * HIST_RING] = e.b;
        d.hist_hash[(size_t)g * HIST_RING] = e.hash;
        d.game[g].game_result = (int8_t)e.result;
        d.game[g].root_dead = 1;
        d.game[g].leaf_kind = LEAF_NONE;
    }
}

__global__ __launch_bounds__(64) void k_legal_moves(Dev d, u16 *moves, int32_t *counts)
{
    __shared__ WaveLds s;
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    Board b = d.cur[g];
    MoveGenInfo mi = wave_movegen(b, lane, s.mv);
    __syncthreads();
    for (int j = lane; j < mi.n; j += 64) moves[(size_t)r * MAX_MOVES + j] = s.mv[j];
    if (lane == 0) counts[r] = mi.n;
}

// the legality test of Game.move (game.py:92-109): is mv one of b's legal moves?  (s.mv is free again on return)
__device__ inline bool is_legal_move(const Board &b, u32 mv, int lane, WaveLds &s)
{
    MoveGenInfo mi = wave_movegen(b, lane, s.mv);
    __syncthreads();
    bool found = false;
    for (int j = lane; j < mi.n; j += 64) found = found || s.mv[j] == mv;
    const bool legal = __ballot(found) != 0;
    __syncthreads();
    return legal;
}

__global__ __launch_bounds__(64) void k_push(Dev d, const u16 *moves, uint8_t *ok)
{
    __shared__ WaveLds s;
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    const u32 mv = moves[r];
    if (mv == NO_MOVE) { if (lane == 0) ok[r] = 0; return; }
    Board b = d.cur[g];
    const bool legal = is_legal_move(b, mv, lane, s);
    if (lane == 0) ok[r] = legal ? 1 : 0;
    if (legal) game_push(d, g, b, mv, lane, s);
}

// k_push with nobody waiting for ok[]: the moves come from another context's move boundary on the same stream
// (k_choose_advance_one's bm), ok may be NULL, and a refused move is a device error that the next synchronising call
// reports.
__global__ __launch_bounds__(64) void k_push_dev(Dev d, const u16 *moves, uint8_t *ok)
{
    __shared__ WaveLds s;
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    const u32 mv = moves[r];
    if (mv == NO_MOVE) { if (lane == 0 && ok) ok[r] = 0; return; }
    Board b = d.cur[g];
    const bool legal = is_legal_move(b, mv, lane, s);
    if (lane == 0) {
        if (ok) ok[r] = legal ? 1 : 0;
        if (!legal) dev_error(d, DERR_STATE);
    }
    if (legal) game_push(d, g, b, mv, lane, s);
}

// DatasetGame.loads / augment_game (dataset.py:21-57): replay a recorded move list, each move through
// the same legality test as Game.move; one launch for every game's whole list.
__global__ __launch_bounds__(64) void k_push_seq(Dev d, const u16 *seq, const int32_t *counts, int stride,
                                                   int32_t *pushed)
{
    __shared__ WaveLds s;
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    const int n = counts[r] < stride ? counts[r] : stride;
    int i = 0;
    for (; i < n; i++) {
        const u32 mv = seq[(size_t)r * stride + i];
        if (mv == NO_MOVE) break;
        Board b = d.cur[g];
        if (!is_legal_move(b, mv, lane, s)) break;
        game_push(d, g, b, mv, lane, s);
        __threadfence_block();               // lane 0 wrote cur / ply / history ring: the next ply reads them
        __syncthreads();
    }
    if (lane == 0) pushed[r] = i;
}

// len(Game) and Game.get_result() of every slot of the window, as contiguous arrays for the host
__global__ __launch_bounds__(64) void k_game_scalars(Dev d, int32_t *plies, int8_t *results)
{
    const int r = blockIdx.x, g = r + d.g0;
    if (threadIdx.x == 0) { plies[r] = d.game[g].ply; results[r] = d.game[g].game_result; }
}

__global__ __launch_bounds__(64) void k_encode_cur(Dev d, void *planes)
{
    __shared__ WaveLds s;
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    Board b = d.cur[g];
    const int p = d.game[g].ply;
    encode_position(d, g, b, 0, p, p, lane, s, planes, r);
}

__global__ __launch_bounds__(64) void k_greedy(Dev d, const float *pol, const uint8_t *mask,
                                               int push, u16 *moves_out)
{
    __shared__ WaveLds s;
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    if (lane == 0) moves_out[r] = NO_MOVE;
    if (mask && !mask[r]) return;
    Board b = d.cur[g];
    MoveGenInfo mi = wave_movegen(b, lane, s.mv);
    __syncthreads();
    if (mi.n == 0) return;                    // legal[argmax([])] would raise; game is over
    const int bi = argmax_policy(d, r, s.mv, mi.n, pol, lane, FMT_FULL);    // always a full policy
    const u32 mv = s.mv[bi];
    __syncthreads();
    if (lane == 0) moves_out[r] = (u16)mv;
    if (push && d.game[g].game_result == RESULT_NONE) game_push(d, g, b, mv, lane, s);
}

// Game.get_copy (game.py:79-80): deep copy incl. the move stack, slot src of context sd -> slot dst of context d
// (within one context sd is d, and the ply-pool test cannot fail)
__device__ inline void copy_game(const Dev &d, int dst, const Dev &sd, int src, int lane)
{
    const int p = sd.game[src].ply;
    if (p > d.MAXPLY) { if (lane == 0) dev_error(d, DERR_PLY_POOL); return; }
    for (int i = lane; i < HIST_RING; i += 64) {
        d.hist[(size_t)dst * HIST_RING + i] = sd.hist[(size_t)src * HIST_RING + i];
        d.hist_hash[(size_t)dst * HIST_RING + i] = sd.hist_hash[(size_t)src * HIST_RING + i];
    }
    for (int i = lane; i < p; i += 64)
        d.rec_moves[(size_t)dst * d.MAXPLY + i] = sd.rec_moves[(size_t)src * sd.MAXPLY + i];
    if (lane == 0) {
        d.cur[dst] = sd.cur[src];
        d.game[dst].ply = p;
        d.game[dst].game_result = sd.game[src].game_result;
        d.game[dst].root_dead = 1;
        d.game[dst].leaf_kind = LEAF_NONE;
    }
}

__global__ __launch_bounds__(64) void k_copy_game(Dev d, int dst, int src)
{
    copy_game(d, dst, d, src, threadIdx.x);
}

// Tree.__init__ (mctree.py:105-109: ``Node(root.get_copy())``) when the caller's Game lives in another
// context (the Game arena) than the search engine: the same deep copy across two contexts of one GPU.
__global__ __launch_bounds__(64) void k_copy_game_across(Dev d, int dst, Dev sd, int src)
{
    copy_game(d, dst, sd, src, threadIdx.x);
}

// ---- SelfPlayTree seam kernels -------------------------------------------------------------------
// keep != 0 (crl_search_begin_kept): a root that k_reroot kept (GameRow.pad) is left as it is -- Tree(Node),
// mctree.py:98-111 -- and only the pending-simulation fields are reset; every other slot gets a fresh tree
__global__ __launch_bounds__(64) void k_search_begin(Dev d, void *planes, int keep)
{
    __shared__ WaveLds s;
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    const size_t nb = (size_t)g * d.N, eb = (size_t)g * d.ECAP;
    const bool kept = keep && uni(d.game[g].root_kept) && !uni(d.game[g].root_dead);
    if (lane == 0) { d.game[g].leaf_kind = LEAF_NONE; d.game[g].path_len = 0; }
    if (d.game[g].game_result != RESULT_NONE) {
        if (lane == 0) { d.game[g].root_dead = 1; d.game[g].n_nodes = 0; d.game[g].root_visits = 0; d.game[g].root_kept = 0; }
        return;
    }
    Board b = d.cur[g];
    const int p = d.game[g].ply;
    if (kept) {                                   // the tower evaluates every row: give it this root's planes
        encode_position(d, g, b, 0, p, p, lane, s, planes, r);
        return;
    }
    MoveGenInfo mi = wave_movegen(b, lane, s.mv);
    __syncthreads();
    init_edges(d, eb, 0, mi.n, s.mv, lane);
    if (lane == 0) {
        NodeMeta m;
        m.edge0 = 0; m.nmoves = (u16)mi.n; m.nexp = 0; m.result = RESULT_NONE; m.has_s2 = 1;
        m.parent = 0; m.parent_edge = -1;
        d.node[nb].meta = m;
        d.node[nb].s2 = b;
        d.node[nb].h2 = board_hash(b);
        d.game[g].n_nodes = 1;
        d.game[g].edge_top = mi.n;
        d.game[g].root_visits = 1;                // Tree.__init__: root.visits = 1
        d.game[g].root_dead = 0;
        d.game[g].root_kept = 0;
        d.path_node[nb] = 0;
    }
    __syncthreads();
    encode_position(d, g, b, 0, p, p, lane, s, planes, r);
}

__global__ __launch_bounds__(64) void k_root_priors(Dev d, const float *pol)
{
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    if (d.game[g].root_dead) return;
    if (uni(d.game[g].root_kept)) {                     // a kept root: its edges hold the priors gathered when the node was
        if (lane == 0) d.game[g].root_kept = 0;         // created; no root evaluation is counted
        return;
    }
    NodeMeta m = d.node[(size_t)g * d.N].meta;
    gather_priors(d, r, (size_t)g * d.ECAP, m.edge0, m.nmoves, pol, lane, FMT_FULL);   // the root's policy is always full
    if (lane == 0) d.counters[(size_t)g * CNT_N + CNT_EVALS] += 1;
}

// what backed-up leaves add to the per-game counters
struct SimCounts { unsigned long long sims = 0, depth = 0, evals = 0, term = 0, nodes = 0, branch = 0; };

// simulate + backprop (+ priors of the new node's future children) of ONE leaf (mctree.py:259-303): `kind` is
// LEAF_TERMINAL_HIT, LEAF_NEW_S1_OVER or LEAF_NEW_S2, `path` the plen edges that lead to it, `row` its evaluator row
__device__ inline void backup_leaf(const Dev &d, int g, int row, int lane, int kind, int leaf, int plen,
                                   const int32_t *path, const float *pol2, const float *val2, int fmt,
                                   const float2 *stats, SimCounts &n)
{
    const size_t eb = (size_t)g * d.ECAP;
    const NodeMeta m = d.node[(size_t)g * d.N + leaf].meta;
    double v;
    if (m.result != RESULT_NONE) {
        v = (double)m.result;                          // state.get_result() (mctree.py:268)
    } else {
        v = (double)val2[row];                         // python float of the f32 value head
        gather_priors(d, row, eb, m.edge0, m.nmoves, pol2, lane, fmt, stats);
        n.evals += 1;                                  // policy/value(S2)
    }
    if (kind == LEAF_NEW_S2) n.evals += 1;             // policy(S1) chose the reply
    for (int l = lane; l < plen; l += 64) {
        Edge *e = d.edge + eb + path[l];
        e->visits += 1;
        e->value = __dadd_rn(e->value, v);
    }
    n.sims += 1;
    n.depth += plen;
    if (kind == LEAF_TERMINAL_HIT) n.term += 1;
    else { n.nodes += 1; n.branch += m.nmoves; }
}

__device__ inline void add_counts(const Dev &d, int g, const SimCounts &n)     // one lane
{
    d.game[g].root_visits += (int)n.sims;
    unsigned long long *c = d.counters + (size_t)g * CNT_N;
    c[CNT_SIMS] += n.sims; c[CNT_DEPTH] += n.depth; c[CNT_EVALS] += n.evals;
    if (n.term) c[CNT_TERMINAL] += n.term;
    if (n.nodes) { c[CNT_NODES] += n.nodes; c[CNT_BRANCH] += n.branch; }
}

// ... for the pending simulation
__device__ inline void backup_pending(const Dev &d, int g, int row, int lane, const float *pol2,
                                      const float *val2)
{
    const int kind = uni(d.game[g].leaf_kind);
    if (kind == LEAF_NONE) return;
    if (kind == LEAF_NEW_REPLY) { dev_error(d, DERR_STATE); return; }
    SimCounts n;
    backup_leaf(d, g, row, lane, kind, uni(d.game[g].leaf_node), uni(d.game[g].path_len),
                d.path_edge + (size_t)g * d.N, pol2, val2, d.policy_fmt, d.stats_s2, n);
    if (lane == 0) {
        d.game[g].leaf_kind = LEAF_NONE;
        add_counts(d, g, n);
    }
    __syncthreads();
}

__global__ __launch_bounds__(64) void k_backup(Dev d, const float *pol2, const float *val2)
{
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    if (d.game[g].root_dead) return;
    backup_pending(d, g, r, lane, pol2, val2);
}

// ---- the pieces of one simulation, shared by the one-leaf kernels below and the waves of search_wave.hpp ---------
// Where a descent stands: the node, its depth, and what select needs of the node's record (wave-uniform).
struct Descent {
    int node = 0, level = 0;
    int edge0 = 0, nmoves = 0, nexp = 0, result = RESULT_NONE, parent_edge = -1;
    bool need_meta = true;                                             // false: the parent's edge record said it all
};

__device__ inline void descent_load_meta(const Dev &d, int g, Descent &x)
{
    if (!x.need_meta) return;
    const NodeMeta m = d.node[(size_t)g * d.N + x.node].meta;
    x.edge0 = uni(m.edge0); x.nmoves = uni(m.nmoves); x.nexp = uni(m.nexp);
    x.result = uni(m.result); x.parent_edge = uni(m.parent_edge);
}

// get_best_child (mctree.py:89-95): argmax of get_value over the node's edge run, first max in children order, i.e.
// the LARGEST legal index among equals.  The value is Q + U of the float contract at the top of this file.  VLOSS (the
// wave schedule) makes it (Q + U) - vloss, vloss = how many of the wave's `cnt` leaf edges in `ledge` (LDS) are this
// edge, and counts no children for a child without visits.
struct BestChild { int j, child; u32 hint; };                          // legal index, the edge's child word and hint

template <bool VLOSS>
__device__ inline BestChild best_child(const Dev &d, int g, int edge0, int nmoves, int lane,
                                       const int *ledge = nullptr, int cnt = 0)
{
    const bool legacy = (d.flags & 1u) != 0;
    const Edge *run = d.edge + (size_t)g * d.ECAP + edge0;
    double best = -__builtin_inf();
    int bj = -1, bchild = 0;
    u32 bhint = 0;
    for (int base = 0; base < nmoves; base += 64) {
        const int j = base + lane;
        if (j < nmoves) {
            const Edge e = run[j];                                     // one 24-byte record per lane
            const int n = e.visits;
            const bool term = (e.child & CHILD_TERMINAL) != 0;
            const double den = (double)(1 + n);
            const double q = __ddiv_rn(e.value, den);
            const bool childless = VLOSS ? (term || n == 0) : term;
            const double sumv = childless ? 0.0 : (double)(n - 1);
            const double cp = legacy ? __dmul_rn(10.0, (double)e.prior)
                                     : (double)__fmul_rn(10.0f, e.prior);
            const double u = __dmul_rn(cp, __ddiv_rn(__dsqrt_rn(sumv), den));
            double sc = __dadd_rn(q, u);
            if constexpr (VLOSS) {
                int vl = 0;
                for (int k = 0; k < cnt; k++) vl += ledge[k] == edge0 + j ? 1 : 0;
                sc = __dsub_rn(sc, (double)vl);
            }
            if (bj < 0 || sc > best || (sc == best && j > bj)) { best = sc; bj = j; bchild = e.child; bhint = e.pad; }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oj = __shfl_xor(bj, o);
        const int oc = __shfl_xor(bchild, o);
        const u32 oh = __shfl_xor(bhint, o);
        const bool take = oj >= 0 && (bj < 0 || ob > best || (ob == best && oj > bj));
        if (take) { best = ob; bj = oj; bchild = oc; bhint = oh; }
    }
    BestChild bc;
    bc.j = uni(bj); bc.child = uni(bchild); bc.hint = uni(bhint);      // the winner's record held them
    return bc;
}

// step into the chosen child: the path grows, and the edge record tells what is known of the child without its own
// record.  false: the path pool is exhausted (nothing was written).
__device__ inline bool descent_step(const Dev &d, int g, int lane, Descent &x, const BestChild &bc)
{
    const size_t nb = (size_t)g * d.N;
    const int child = bc.child & CHILD_NONE;
    if (x.level + 1 >= d.N) { dev_error(d, DERR_NODE_POOL); return false; }
    if (lane == 0) {
        d.path_edge[nb + x.level] = x.edge0 + bc.j;
        d.path_node[nb + x.level + 1] = (u16)child;
    }
    x.level++;
    x.node = child;
    x.need_meta = false;
    if (bc.child & CHILD_TERMINAL) {                                   // the child's state ended the game: as its
        x.result = 0;                                                  // record would say (any value but RESULT_NONE)
    } else if (bc.hint & HINT_FULL) {                                  // fully expanded: straight to its edge records
        x.edge0 = hint_edge0(bc.hint); x.nmoves = hint_nmoves(bc.hint); x.nexp = x.nmoves;
        x.result = RESULT_NONE;
    } else {
        x.need_meta = true;
    }
    return true;
}

// expand (mctree.py:231-243), our half: the next unexpanded move of node x.node becomes node c.  Everything up to the
// encoded planes of S1 in row `row` of planes1; the caller records the leaf where its schedule keeps it.  kind:
// LEAF_NEW_S1_OVER, LEAF_NEW_REPLY (then s.mv holds the n legal moves of S1), or LEAF_NONE when a pool is exhausted
// (nothing was written).  `fence`: the wave schedule's block fence in front of the barrier that publishes the path.
struct NewLeaf { int kind, edge, n; };

__device__ inline NewLeaf expand_child(const Dev &d, int g, int row, int lane, WaveLds &s, Descent &x, int c, int ply,
                                       void *planes1, bool fence)
{
    const size_t nb = (size_t)g * d.N, eb = (size_t)g * d.ECAP;
    NewLeaf lf;
    lf.kind = LEAF_NONE; lf.n = 0;
    lf.edge = x.edge0 + (x.nmoves - 1 - x.nexp);                       // list.pop(): last first
    if (c >= d.N || x.level + 1 >= d.N) { dev_error(d, DERR_NODE_POOL); return lf; }
    const u32 mv = d.edge[eb + lf.edge].move;
    if (lane == 0) {
        d.node[nb + x.node].meta.nexp = (u16)(x.nexp + 1);
        if (x.nexp + 1 == x.nmoves && x.parent_edge >= 0)              // fully expanded from now on: leave the hint
            d.edge[eb + x.parent_edge].pad = hint_pack(x.edge0, x.nmoves);
        d.path_edge[nb + x.level] = lf.edge;
        d.path_node[nb + x.level + 1] = (u16)c;
    }
    x.level++;
    Board parent = d.node[nb + x.node].s2;
    Board s1 = apply_move(parent, mv);
    if (fence) __threadfence_block();
    __syncthreads();                                                   // path_node visible
    PosEval e = eval_position(d, g, s1, 2 * x.level - 1, ply, ply, lane, s);
    NodeMeta cm;
    cm.edge0 = 0; cm.nmoves = (u16)e.n; cm.nexp = 0; cm.result = (int8_t)e.result;
    cm.has_s2 = 0; cm.parent = (u16)x.node; cm.parent_edge = lf.edge;
    if (lane == 0) {
        d.node[nb + c].s1 = e.b;
        d.node[nb + c].h1 = e.hash;
        d.node[nb + c].meta = cm;
    }
    lf.n = e.n;
    if (e.result != RESULT_NONE) {                                     // game ended on our move
        if (lane == 0) {
            d.node[nb + c].s2 = e.b;
            d.node[nb + c].h2 = e.hash;
            d.edge[eb + lf.edge].child = (u16)(c | CHILD_TERMINAL);
        }
        lf.kind = LEAF_NEW_S1_OVER;
    } else {
        if (lane == 0) d.edge[eb + lf.edge].child = (u16)c;
        lf.kind = LEAF_NEW_REPLY;
        __syncthreads();
        encode_position(d, g, e.b, 2 * x.level - 1, ply, ply, lane, s, planes1, row);   // (leaves s.mv alone)
    }
    return lf;
}

// expand, the opponent's half (mctree.py:244-250) and Node() of the new state (mctree.py:28-37), in two pieces: the
// choice of the reply (reply_child below: the net's greedy move; k_reply_opponent of opponent.hpp: the built-in
// opponent's) and everything after it, reply_tail: node c, reached by a path of `level` edges, whose state after our
// move is s1, gets `reply`, its S2, an edge run from slot edge0 on and the planes of S2 in row `row` of planes2.
// Returns the length of the run, -1 when the edge pool is exhausted (nothing was written).
__device__ inline int reply_tail(const Dev &d, int g, int row, int lane, WaveLds &s, int c, int level, int ply,
                                 const Board &s1, u32 reply, int edge0, int fmt, uint8_t *kind, void *planes2)
{
    const size_t nb = (size_t)g * d.N, eb = (size_t)g * d.ECAP;
    Board s2 = apply_move(s1, reply);
    PosEval e = eval_position(d, g, s2, 2 * level, ply, ply, lane, s);
    if (edge0 + e.n > d.ECAP) { dev_error(d, DERR_EDGE_POOL); return -1; }
    init_edges(d, eb, edge0, e.n, s.mv, lane);
    if (fmt != FMT_FULL && e.result == RESULT_NONE) write_labels(d, row, s.mv, e.n, d.lab_s2, d.lab_n2, lane);
    if (lane == 0) {
        NodeMeta m = d.node[nb + c].meta;
        m.edge0 = edge0; m.nmoves = (u16)e.n; m.nexp = 0; m.result = (int8_t)e.result; m.has_s2 = 1;
        d.node[nb + c].meta = m;
        d.node[nb + c].s2 = e.b;
        d.node[nb + c].h2 = e.hash;
        d.node[nb + c].reply = (u16)reply;
        d.game[g].edge_top = edge0 + e.n;
        if (e.result != RESULT_NONE) d.edge[eb + m.parent_edge].child = (u16)(c | CHILD_TERMINAL);
        *kind = LEAF_NEW_S2;
    }
    __syncthreads();
    encode_position(d, g, e.b, 2 * level, ply, ply, lane, s, planes2, row);
    return e.n;
}

// the net's reply: agent.best_move(S1, real_game=True) picks it from row `row` of pol1 among the n1 legal moves mv1
__device__ inline int reply_child(const Dev &d, int g, int row, int lane, WaveLds &s, int c, int level, int ply,
                                  const u16 *mv1, int n1, int edge0, const float *pol1, int fmt, const float2 *stats,
                                  uint8_t *kind, void *planes2)
{
    Board s1 = d.node[(size_t)g * d.N + c].s1;
    const int bi = argmax_policy(d, row, mv1, n1, pol1, lane, fmt, stats);   // legal[argmax(policy masked to legal)]
    return reply_tail(d, g, row, lane, s, c, level, ply, s1, mv1[bi], edge0, fmt, kind, planes2);
}

__global__ __launch_bounds__(64, 4) void k_select_expand(Dev d, const float *pol2, const float *val2,
                                                      void *planes1)
{
    __shared__ WaveLds s;
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    if (lane == 0) d.lab_n1[r] = 0;                     // no policy(S1) wanted unless a reply is needed
    if (d.game[g].root_dead) return;
    backup_pending(d, g, r, lane, pol2, val2);

    const int p = uni(d.game[g].ply);
    if (d.ECAP >= HINT_EDGE_CAP) { dev_error(d, DERR_EDGE_POOL); return; }   // edge slots fit the hint
    Descent x;
    for (;;) {
        descent_load_meta(d, g, x);
        if (x.result != RESULT_NONE) {                                 // is_terminal_state
            if (lane == 0) { d.game[g].leaf_kind = LEAF_TERMINAL_HIT; d.game[g].leaf_node = x.node; }
            break;
        }
        if (x.nexp < x.nmoves) {                                       // not fully expanded
            const int c = uni(d.game[g].n_nodes);                      // wave-uniform: scalar addressing
            const NewLeaf lf = expand_child(d, g, r, lane, s, x, c, p, planes1, false);
            if (lf.kind == LEAF_NONE) break;
            if (lf.kind == LEAF_NEW_REPLY) {
                for (int i = lane; i < lf.n; i += 64) d.s1_moves[(size_t)g * MAX_MOVES + i] = s.mv[i];
                if (d.policy_fmt) write_labels(d, r, s.mv, lf.n, d.lab_s1, d.lab_n1, lane);
                if (lane == 0) d.game[g].s1_n = lf.n;
            }
            if (lane == 0) { d.game[g].n_nodes = c + 1; d.game[g].leaf_node = c; d.game[g].leaf_kind = lf.kind; }
            break;
        }
        if (!descent_step(d, g, lane, x, best_child<false>(d, g, x.edge0, x.nmoves, lane))) break;
    }
    if (lane == 0) d.game[g].path_len = x.level;
}

__global__ __launch_bounds__(64) void k_reply(Dev d, const float *pol1, void *planes2)
{
    __shared__ WaveLds s;
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    if (lane == 0) d.lab_n2[r] = 0;                     // no policy(S2) wanted unless a new node gets priors
    if (d.game[g].root_dead || d.game[g].leaf_kind != LEAF_NEW_REPLY) return;
    reply_child(d, g, r, lane, s, uni(d.game[g].leaf_node), uni(d.game[g].path_len), uni(d.game[g].ply),
                d.s1_moves + (size_t)g * MAX_MOVES, uni(d.game[g].s1_n), uni(d.game[g].edge_top), pol1,
                d.policy_fmt, d.stats_s1, &d.game[g].leaf_kind, planes2);
}

__global__ __launch_bounds__(64) void k_root_children(Dev d, int32_t *nchild, int32_t *visits,
                                                      double *values, float *priors, u16 *moves,
                                                      u16 *replies, int32_t *root_visits)
{
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    const size_t nb = (size_t)g * d.N, eb = (size_t)g * d.ECAP;
    if (d.game[g].root_dead) {
        if (lane == 0) { nchild[r] = 0; root_visits[r] = 0; }
        return;
    }
    NodeMeta m = d.node[nb].meta;
    if (lane == 0) { nchild[r] = m.nexp; root_visits[r] = d.game[g].root_visits; }
    for (int k = lane; k < m.nexp; k += 64) {
        const Edge e = d.edge[eb + m.edge0 + (m.nmoves - 1 - k)];   // children order = reverse legal
        const size_t o = (size_t)r * MAX_MOVES + k;
        const int c = e.child & CHILD_NONE;
        visits[o] = e.visits;
        values[o] = e.value;
        // _update_prior runs only once the node is fully expanded (mctree.py:254-255); until
        // then the reference's children still carry Node.prior = 1
        priors[o] = m.nexp < m.nmoves ? 1.0f : e.prior;
        moves[o] = e.move;
        replies[o] = d.node[nb + c].meta.has_s2 ? d.node[nb + c].reply : NO_MOVE;
    }
}

// gam.move(bm); gam.move(am) (selfplay.py:77-78) with the moves of root child c, reached over edge record ed: the
// game goes on by one ply (the game ended on our move) or two, to ply np; the tree is consumed.  One lane.
// ONE_PLY: gam.move(bm) alone (k_advance_one) -- a child with a reply stops at S1, which is a running position
// (a node gets its reply only where the game went on after our move); am is not written.
template <bool ONE_PLY = false>
__device__ inline void advance_game(const Dev &d, int g, int r, int c, const Edge &ed, const NodeMeta &cm, int np,
                                    u16 *bm, u16 *am)
{
    const NodeRow &n = d.node[(size_t)g * d.N + c];
    const int p = d.game[g].ply;
    size_t hi = (size_t)g * HIST_RING + ((p + 1) & (HIST_RING - 1));
    d.hist[hi] = n.s1;
    d.hist_hash[hi] = n.h1;
    d.rec_moves[(size_t)g * d.MAXPLY + p] = ed.move;
    bm[r] = ed.move;
    if (ONE_PLY && cm.has_s2) {
        d.cur[g] = n.s1;
        d.game[g].ply = np;
        d.game[g].game_result = RESULT_NONE;
        d.game[g].root_dead = 1;
        return;
    }
    if (cm.has_s2) {
        hi = (size_t)g * HIST_RING + ((p + 2) & (HIST_RING - 1));
        d.hist[hi] = n.s2;
        d.hist_hash[hi] = n.h2;
        d.rec_moves[(size_t)g * d.MAXPLY + p + 1] = n.reply;
        am[r] = n.reply;
    }
    d.cur[g] = n.s2;                              // node state (S1 copy when the game ended there)
    d.game[g].ply = np;
    d.game[g].game_result = cm.result;
    d.game[g].root_dead = 1;                      // the tree is consumed: fresh tree per move
}

__global__ __launch_bounds__(64) void k_advance(Dev d, const int32_t *chosen, u16 *bm, u16 *am)
{
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    if (lane != 0) return;
    bm[r] = NO_MOVE; am[r] = NO_MOVE;
    const int k = chosen[r];
    if (k < 0 || d.game[g].root_dead) return;
    const size_t nb = (size_t)g * d.N, eb = (size_t)g * d.ECAP;
    NodeMeta m = d.node[nb].meta;
    if (k >= m.nexp || d.game[g].leaf_kind != LEAF_NONE) { dev_error(d, DERR_STATE); return; }
    const Edge ed = d.edge[eb + m.edge0 + (m.nmoves - 1 - k)];
    const int c = ed.child & CHILD_NONE;
    NodeMeta cm = d.node[nb + c].meta;
    const int np = d.game[g].ply + (cm.has_s2 ? 2 : 1);
    if (np > d.MAXPLY) { dev_error(d, DERR_PLY_POOL); return; }
    advance_game(d, g, r, c, ed, cm, np, bm, am);
}

// gam.move(bm) alone: Agent.best_move in a game whose other side moves for itself (gameagent.py, benchmark.py:100-118).
// k_advance's checks; the game goes on by ONE ply, to S1 of the chosen child, and the tree is consumed.  A child
// without a reply ended the game on our move: exactly k_advance's outcome.
__global__ __launch_bounds__(64) void k_advance_one(Dev d, const int32_t *chosen, u16 *bm)
{
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    if (lane != 0) return;
    bm[r] = NO_MOVE;
    const int k = chosen[r];
    if (k < 0 || d.game[g].root_dead) return;
    const size_t nb = (size_t)g * d.N, eb = (size_t)g * d.ECAP;
    NodeMeta m = d.node[nb].meta;
    if (k >= m.nexp || d.game[g].leaf_kind != LEAF_NONE) { dev_error(d, DERR_STATE); return; }
    const Edge ed = d.edge[eb + m.edge0 + (m.nmoves - 1 - k)];
    const int c = ed.child & CHILD_NONE;
    NodeMeta cm = d.node[nb + c].meta;
    const int np = d.game[g].ply + 1;
    if (np > d.MAXPLY) { dev_error(d, DERR_PLY_POOL); return; }
    advance_game<true>(d, g, r, c, ed, cm, np, bm, nullptr);
}

// The noise-free move boundary of a game whose two sides search for themselves, without the host in between
// (gameagent.py; the choice is compute_policy + np.argmax, mctree.py:305-322): k_root_children, the host's
// choose_children(noise=False) and k_advance_one in one kernel.  One wavefront per slot.  A slot MOVES iff its tree is
// alive, its game has no result, ply < ply_limit[r], the side to move is mover_white and the root has an expanded
// child.  The chosen child is the FIRST MAXIMUM of the root children's visits in children order (reverse legal order
// over the nexp expanded children): the policy visits**(1/tau) / root_visits**(1/tau) is strictly increasing in visits
// for every tau, and np.argmax takes the first maximum.  The slot is then advanced as k_advance_one advances that
// child.  bm[r] / chosen[r] (device): the move and the child, NO_MOVE / -1 for a slot that does not move -- its state
// is untouched.
__global__ __launch_bounds__(64) void k_choose_advance_one(Dev d, int mover_white, const int32_t *ply_limit, u16 *bm,
                                                           int32_t *chosen)
{
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    if (lane == 0) { bm[r] = NO_MOVE; chosen[r] = -1; }
    if (uni(d.game[g].root_dead) || uni(d.game[g].game_result) != RESULT_NONE) return;
    const int p = uni(d.game[g].ply);
    if (p >= uni(ply_limit[r]) || (int)st_turn(uni(d.cur[g].state)) != (mover_white ? 1 : 0)) return;
    const size_t nb = (size_t)g * d.N, eb = (size_t)g * d.ECAP;
    const NodeMeta m = d.node[nb].meta;
    const int nexp = uni((int)m.nexp), first = uni((int)m.edge0) + uni((int)m.nmoves) - 1;
    if (nexp < 1) return;
    int best = -1, bk = 0x7FFFFFFF;                                     // lane-strided scan: roots have up to 218 children
    for (int k = lane; k < nexp; k += 64) {
        const int v = d.edge[eb + first - k].visits;
        if (v > best) { best = v; bk = k; }                            // ascending k: the first maximum of this lane
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int ov = __shfl_xor(best, o), ok = __shfl_xor(bk, o);
        if (ov > best || (ov == best && ok < bk)) { best = ov; bk = ok; }
    }
    if (lane != 0) return;
    const int k = bk;
    if (k >= nexp || d.game[g].leaf_kind != LEAF_NONE) { dev_error(d, DERR_STATE); return; }
    const Edge ed = d.edge[eb + first - k];
    const int c = ed.child & CHILD_NONE;
    const NodeMeta cm = d.node[nb + c].meta;
    const int np = p + 1;
    if (np > d.MAXPLY) { dev_error(d, DERR_PLY_POOL); return; }
    chosen[r] = k;
    advance_game<true>(d, g, r, c, ed, cm, np, bm, nullptr);
}

// ---- Tree(Node) (mctree.py:98-111): the chosen child becomes the root and keeps its subtree --------------------
// k_advance's work, then -- instead of killing the tree -- the subtree below the chosen child is compacted in
// place so that the child is node 0.  Kept iff the child's state is S2 and running and kept nodes + next_sims
// fit the node pool (one simulation creates at most one node); otherwise exactly k_advance's outcome.
//   pass 1  membership + new ids + new edge offsets.  Ids are handed out in creation order (parent < child),
//           so one ascending pass decides keep[i] = keep[parent[i]]; edge runs were allocated in the same order,
//           so the new offset of a run is the exclusive prefix sum of the owned edge counts of the kept nodes.
//           The id map lives in path_node, the new edge0 in path_edge (both dead at a move boundary).
//   pass 2  parent_edge of every kept node (in place, while every record still sits at its old id), then the
//           edge runs move down, ascending, 64 records read before they are written; child ids and descent
//           hints are rewritten on the way.
//   pass 3  node records move to their new ids (ascending, 64 read before written).
// No arithmetic on values: sums, visits and priors move as bit patterns.
constexpr u16 ID_DROPPED = 0xFFFF;

__global__ __launch_bounds__(64) void k_reroot(Dev d, const int32_t *chosen, int next_sims, u16 *bm, u16 *am,
                                               int32_t *kept_nodes, int32_t *kept_children)
{
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    if (lane == 0) { bm[r] = NO_MOVE; am[r] = NO_MOVE; kept_nodes[r] = 0; kept_children[r] = 0; }
    const int k = chosen[r];
    if (k < 0 || d.game[g].root_dead) return;
    const size_t nb = (size_t)g * d.N, eb = (size_t)g * d.ECAP;
    const NodeMeta m = d.node[nb].meta;
    if (k >= m.nexp || d.game[g].leaf_kind != LEAF_NONE) { if (lane == 0) dev_error(d, DERR_STATE); return; }
    const Edge ed = d.edge[eb + m.edge0 + (m.nmoves - 1 - k)];
    const int c = uni(ed.child & CHILD_NONE);
    const NodeMeta cm = d.node[nb + c].meta;
    const int p = uni(d.game[g].ply);
    const int np = p + (cm.has_s2 ? 2 : 1);
    if (np > d.MAXPLY) { if (lane == 0) dev_error(d, DERR_PLY_POOL); return; }
    const int n = uni(d.game[g].n_nodes);
    if (lane == 0) {
        advance_game(d, g, r, c, ed, cm, np, bm, am);
        d.game[g].root_kept = 0;
    }
    if (!cm.has_s2 || cm.result != RESULT_NONE) return;
    __syncthreads();                                                   // node c was read before any record moves

    u16 *map = d.path_node + nb;
    int32_t *ne0 = d.path_edge + nb;
    // ---- pass 1
    int K = 0, E = 0;
    for (int base = c; base < n; base += 64) {
        const int i = base + lane;
        const bool in = i < n;
        int par = 0, owned = 0;
        if (in) {
            const NodeMeta mi = d.node[nb + i].meta;
            par = mi.parent;
            owned = mi.has_s2 ? mi.nmoves : 0;                         // a node whose game ended on our move owns no run
        }
        bool known = !in || i == c || par < base, keep = false;
        if (in) {
            if (i == c) keep = true;
            else if (par < base) keep = par >= c && map[par] != ID_DROPPED;
        }
        for (;;) {                                                     // parents inside this chunk
            const u64 km = __ballot(known), kp = __ballot(keep);
            if (km == ~0ull) break;
            if (!known) {
                const int pl = par - base;
                if ((km >> pl) & 1) { keep = ((kp >> pl) & 1) != 0; known = true; }
            }
        }
        const u64 kp = __ballot(keep);
        const int nid = K + popc(kp & ((1ull << lane) - 1));
        const int x = keep ? owned : 0;
        int incl = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (in) {
            map[i] = keep ? (u16)nid : ID_DROPPED;
            if (keep) ne0[i] = E + incl - x;
        }
        K += popc(kp);
        E += __shfl(incl, 63);
        __threadfence_block();
        __syncthreads();                                               // the next chunk reads this chunk's map entries
    }
    if (K + next_sims > d.N) return;                                   // no room: fresh tree at the next begin

    // ---- pass 2
    for (int base = c; base < n; base += 64) {
        const int i = base + lane;
        bool has_run = false;
        int oe0 = 0, nm = 0, n0 = 0;
        if (i < n && map[i] != ID_DROPPED) {
            const NodeMeta mi = d.node[nb + i].meta;
            if (i != c)
                d.node[nb + i].meta.parent_edge = mi.parent_edge - d.node[nb + mi.parent].meta.edge0 + ne0[mi.parent];
            if (mi.has_s2 && mi.nmoves > 0) { has_run = true; oe0 = mi.edge0; nm = mi.nmoves; n0 = ne0[i]; }
        }
        u64 todo = __ballot(has_run);
        while (todo) {
            const int l = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const int so = __shfl(oe0, l), dn = __shfl(n0, l), cnt = __shfl(nm, l);
            for (int t = 0; t < cnt; t += 64) {
                const int j = t + lane;
                Edge e;
                e.value = 0.0; e.visits = 0; e.prior = 0.f; e.move = 0; e.child = CHILD_NONE; e.pad = 0;
                if (j < cnt) {
                    e = d.edge[eb + so + j];
                    if (e.child != CHILD_NONE) {
                        const int cid = e.child & CHILD_NONE;
                        e.child = (u16)(map[cid] | (e.child & CHILD_TERMINAL));
                        if (e.pad & HINT_FULL) e.pad = hint_pack(ne0[cid], hint_nmoves(e.pad));
                    }
                }
                __syncthreads();                                       // 64 records read before they are written
                if (j < cnt) d.edge[eb + dn + j] = e;
            }
        }
    }
    __threadfence_block();
    __syncthreads();

    // ---- pass 3
    for (int base = c; base < n; base += 64) {
        const int i = base + lane;
        const int nid = i < n ? map[i] : ID_DROPPED;
        const bool kp = nid != ID_DROPPED;
        NodeRow row;
        if (kp) {
            row = d.node[nb + i];
            row.meta.edge0 = row.meta.has_s2 ? ne0[i] : 0;
            if (i == c) { row.meta.parent = 0; row.meta.parent_edge = -1; }
            else row.meta.parent = map[row.meta.parent];
        }
        __syncthreads();
        if (kp) d.node[nb + nid] = row;
    }
    __threadfence_block();
    __syncthreads();
    if (lane == 0) {
        d.game[g].n_nodes = K;
        d.game[g].edge_top = E;
        d.game[g].root_visits = 1;                                     // mctree.py:111
        d.game[g].root_dead = 0;
        d.game[g].path_len = 0;
        d.game[g].root_kept = 1;                                             // root was kept
        d.path_node[nb] = 0;
        kept_nodes[r] = K;
        kept_children[r] = cm.nexp;
    }
}

// crl_copy_game_tree: after k_copy_game, the live tree of slot src goes with the game (grid of workgroups)
__global__ __launch_bounds__(64) void k_copy_tree(Dev d, int dst, int src)
{
    if (d.game[src].root_dead) return;
    const int tid = blockIdx.x * 64 + threadIdx.x, stride = gridDim.x * 64;
    const size_t nbs = (size_t)src * d.N, nbd = (size_t)dst * d.N;
    const size_t ebs = (size_t)src * d.ECAP, ebd = (size_t)dst * d.ECAP;
    const int n = d.game[src].n_nodes, et = d.game[src].edge_top;
    for (int i = tid; i < n; i += stride) d.node[nbd + i] = d.node[nbs + i];
    for (int i = tid; i < et; i += stride) d.edge[ebd + i] = d.edge[ebs + i];
    if (tid == 0) {
        d.game[dst].n_nodes = n;
        d.game[dst].edge_top = et;
        d.game[dst].root_visits = d.game[src].root_visits;
        d.game[dst].path_len = 0;
        d.game[dst].root_kept = d.game[src].root_kept;
        d.game[dst].root_dead = 0;
        d.path_node[nbd] = 0;
    }
}

}  // namespace crl
