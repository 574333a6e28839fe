// search_wave.hpp -- `threads` > 1: virtual-loss WAVES of simulations per game on the device.
//
// The reference runs `threads` explore_tree workers on one tree, kept apart by a virtual loss
// (mctree.py:12,173-176,226-227,289-293).  One legal schedule of those workers is deterministic, the wave
// schedule: up to T workers select one after the other on frozen statistics (only vloss and the tree's structure
// change), then all simulate, then all back up in thread order.  A worker whose descent would step onto a node that
// an earlier worker of the same wave created (its S2 does not exist before the reply was evaluated) stays idle: the
// wave ends short.  tests/golden/wave_cases.json pins this schedule to the reference's own select / simulate /
// backprop; tests/wave_util.py restates it.
//
//   k_wave_begin     budgets and counters of a search                (after k_search_begin + k_root_priors)
//   k_wave_select    backprop of the previous wave in thread order + up to min(T, budget) descents, one expansion each
//   k_wave_reply     the opponent's reply of every new node, in thread order (edge runs are allocated in that order)
//   k_wave_backup    backprop of the last wave                        (the counterpart of k_backup)
//   k_wave_remaining the largest remaining budget of the window in one int
//
// One wavefront per game, as in search.hpp, and the same pieces of a simulation (best_child, descent_step,
// expand_child, reply_child, backup_leaf), each leaf with its own path plane and evaluator row: row = r * T + t.
// The float contract is search.hpp's, with the two differences best_child<true> makes (mctree.py:71-87):
//   the score is (Q + U) - vloss, one more float64 operation; vloss = how many of this wave's leaves ARE that child
//   (it sits on the reached node alone, mctree.py:226-227), so it lives in LDS as the list of the wave's leaf edges and
//   never reaches HBM.  Subtracting 0.0 is exact: T = 1 is the arithmetic of k_select_expand.
//   sum of the child's children's visits is 0 for a child with visits == 0 -- a sibling created earlier in this wave,
//   scored once its parent became fully expanded mid-wave.
#pragma once
#include "search.hpp"

namespace crl {

constexpr int WAVE_MAX_THREADS = 64;
enum WaveStat { WST_WAVES = 0, WST_SHORT, WST_LEAVES, WST_N };

__device__ inline Dev thread_view(const Dev &d, const WaveArrs &w, int t)
{
    Dev dt = d;                                        // past_ref / count_prior / encode_position index path_node[g*N + k]:
    const size_t plane = (size_t)t * d.G * d.N;        // a view whose path arrays are thread t's [G][N] plane reuses them
    dt.path_edge = w.path_edge + plane;
    dt.path_node = w.path_node + plane;                // (kept over handing the two pointers through: docs/history/experiments.md)
    return dt;
}

__global__ __launch_bounds__(64) void k_wave_begin(Dev d, int n_sims)
{
    const WaveArrs w = *d.wave;
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    if (lane < w.T) w.kind[(size_t)g * w.T + lane] = LEAF_NONE;
    if (lane < WST_N) w.stats[(size_t)g * WST_N + lane] = 0;
    if (lane == 0) {
        if (d.game[g].leaf_kind != LEAF_NONE || w.n_leaves[g] > 0) dev_error(d, DERR_STATE);   // a simulation is pending
        w.budget[g] = d.game[g].root_dead ? 0 : n_sims;
        w.n_leaves[g] = 0;
    }
}

// simulate + backprop (+ priors of each new node's future children) for every leaf of the pending wave, thread order
__device__ inline void wave_backup_pending(const Dev &d, const WaveArrs &w, int g, int r, int lane, const float *pol2,
                                           const float *val2)
{
    const int nl = uni(w.n_leaves[g]);
    if (nl <= 0) return;
    SimCounts n;
    for (int t = 0; t < nl; t++) {
        const size_t gt = (size_t)g * w.T + t;
        const int kind = uni(w.kind[gt]);
        if (kind == LEAF_NONE || kind == LEAF_NEW_REPLY) { dev_error(d, DERR_STATE); return; }
        backup_leaf(d, g, r * w.T + t, lane, kind, uni(w.leaf[gt]), uni(w.plen[gt]),
                    w.path_edge + ((size_t)t * d.G + g) * d.N, pol2, val2, FMT_FULL, nullptr, n);
        __threadfence_block();
        __syncthreads();                                               // the next leaf adds into the same sums
    }
    if (lane == 0) {
        w.n_leaves[g] = 0;
        add_counts(d, g, n);
    }
    if (lane < nl) w.kind[(size_t)g * w.T + lane] = LEAF_NONE;
    __threadfence_block();
    __syncthreads();
}

__global__ __launch_bounds__(64) void k_wave_backup(Dev d, const float *pol2, const float *val2)
{
    const WaveArrs w = *d.wave;
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    if (d.game[g].root_dead) return;
    wave_backup_pending(d, w, g, r, lane, pol2, val2);
}

__global__ __launch_bounds__(64) void k_wave_select(Dev d, const float *pol2, const float *val2, void *planes1)
{
    __shared__ WaveLds s;
    __shared__ int s_ledge[WAVE_MAX_THREADS];                          // the wave's leaf edges = its virtual losses
    const WaveArrs w = *d.wave;
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    if (d.game[g].root_dead) return;
    if (uni(d.game[g].leaf_kind) != LEAF_NONE) { dev_error(d, DERR_STATE); return; }   // a one-leaf simulation is pending
    wave_backup_pending(d, w, g, r, lane, pol2, val2);

    const int budget = uni(w.budget[g]);
    if (budget <= 0) return;                                           // this game's search is complete: it idles
    const int W = budget < w.T ? budget : w.T;
    const size_t nb = (size_t)g * d.N;
    const int p = uni(d.game[g].ply);
    if (d.ECAP >= HINT_EDGE_CAP) { dev_error(d, DERR_EDGE_POOL); return; }
    int nn = uni(d.game[g].n_nodes);
    u64 fresh = 0;                                                     // bit t: leaf t was created by this wave
    int cnt = 0;
    bool stop = false;
    for (int t = 0; t < W && !stop; t++) {
        const Dev dt = thread_view(d, w, t);
        const size_t gt = (size_t)g * w.T + t;
        Descent x;
        int last_edge = -1;
        bool made = false;
        if (lane == 0) dt.path_node[nb] = 0;
        for (;;) {
            descent_load_meta(d, g, x);
            if (x.result != RESULT_NONE) {                             // is_terminal_state: the leaf is this node again
                if (x.level == 0) { dev_error(d, DERR_STATE); stop = true; break; }
                if (lane == 0) { w.kind[gt] = LEAF_TERMINAL_HIT; w.leaf[gt] = (u16)x.node; s_ledge[t] = last_edge; }
                made = true;
                break;
            }
            if (x.nexp < x.nmoves) {                                   // not fully expanded: expand ONE child
                const NewLeaf lf = expand_child(dt, g, r * w.T + t, lane, s, x, nn, p, planes1, true);
                if (lf.kind == LEAF_NONE) { stop = true; break; }
                if (lf.kind == LEAF_NEW_REPLY) {
                    for (int i = lane; i < lf.n; i += 64) w.s1_moves[gt * MAX_MOVES + i] = s.mv[i];
                    if (lane == 0) w.s1_n[gt] = lf.n;
                }
                if (lane == 0) { w.leaf[gt] = (u16)nn; w.kind[gt] = (uint8_t)lf.kind; s_ledge[t] = lf.edge; }
                nn++;
                fresh |= 1ull << t;
                made = true;
                break;
            }
            const BestChild bc = best_child<true>(d, g, x.edge0, x.nmoves, lane, s_ledge, cnt);
            const int edge = x.edge0 + bc.j;
            // stepping onto a node this wave created: its S2 does not exist yet -- the wave ends here
            const bool on_fresh = lane < cnt && ((fresh >> lane) & 1) && s_ledge[lane] == edge;
            if (__ballot(on_fresh) != 0) { stop = true; break; }
            if (!descent_step(dt, g, lane, x, bc)) { stop = true; break; }
            last_edge = edge;
        }
        if (made) {
            if (lane == 0) w.plen[gt] = x.level;
            cnt++;
        }
        __threadfence_block();
        __syncthreads();                                               // s_ledge, nexp, hints, child ids: the next descent reads them
    }
    if (lane >= cnt && lane < w.T) w.kind[(size_t)g * w.T + lane] = LEAF_NONE;
    if (lane == 0) {
        d.game[g].n_nodes = nn;
        w.n_leaves[g] = cnt;
        w.budget[g] = budget - cnt;
        int32_t *st = w.stats + (size_t)g * WST_N;
        st[WST_WAVES] += 1;
        st[WST_SHORT] += cnt < W ? 1 : 0;
        st[WST_LEAVES] += cnt;
    }
}

__global__ __launch_bounds__(64) void k_wave_reply(Dev d, const float *pol1, void *planes2)
{
    __shared__ WaveLds s;
    const WaveArrs w = *d.wave;
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    if (d.game[g].root_dead) return;
    const int nl = uni(w.n_leaves[g]);
    const int p = uni(d.game[g].ply);
    int top = uni(d.game[g].edge_top);
    for (int t = 0; t < nl; t++) {
        const size_t gt = (size_t)g * w.T + t;
        if (uni(w.kind[gt]) != LEAF_NEW_REPLY) continue;
        const Dev dt = thread_view(d, w, t);
        // edge runs in thread order: the same tree every run
        const int n = reply_child(dt, g, r * w.T + t, lane, s, uni(w.leaf[gt]), uni(w.plen[gt]), p,
                                  w.s1_moves + gt * MAX_MOVES, uni(w.s1_n[gt]), top, pol1, FMT_FULL, nullptr,
                                  w.kind + gt, planes2);
        if (n < 0) return;
        top += n;
    }
}

// the largest remaining budget of the window: 0 = every game has selected its last wave
__global__ __launch_bounds__(64) void k_wave_remaining(Dev d, int n, int32_t *out)
{
    const WaveArrs w = *d.wave;
    int m = 0;
    for (int r = threadIdx.x; r < n; r += 64) {
        const int b = w.budget[r + d.g0];
        m = b > m ? b : m;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int x = __shfl_xor(m, o);
        m = x > m ? x : m;
    }
    if (threadIdx.x == 0) *out = m;
}

__global__ __launch_bounds__(64) void k_wave_stats(Dev d, int n, int32_t *out)
{
    const WaveArrs w = *d.wave;
    for (int i = threadIdx.x + blockIdx.x * 64; i < n * WST_N; i += 64 * gridDim.x)
        out[i] = w.stats[(size_t)d.g0 * WST_N + i];
}

}  // namespace crl
