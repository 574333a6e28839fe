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
// One wavefront per game, as in search.hpp.  Evaluator rows are game-major: row = r * T + t.
// Score of a child (mctree.py:71-87): (Q + U) - vloss, the subtraction one more float64 operation after the float
// contract of search.hpp; vloss = how many of this wave's leaves ARE that child (it sits on the reached node alone,
// mctree.py:226-227), so it lives in LDS as the list of the wave's leaf edges and never reaches HBM.  Subtracting 0.0
// is exact: T = 1 is the arithmetic of k_select_expand.
// sum of the child's children's visits: visits - 1 as in search.hpp, but 0 for a child with visits == 0 -- a sibling
// created earlier in this wave, scored once its parent became fully expanded mid-wave.
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
    dt.path_node = w.path_node + plane;
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
    const size_t nb = (size_t)g * d.N, eb = (size_t)g * d.ECAP;
    unsigned long long evals = 0, depth = 0, term = 0, nodes = 0, branch = 0;
    for (int t = 0; t < nl; t++) {
        const size_t gt = (size_t)g * w.T + t;
        const int row = r * w.T + t;
        const int kind = uni(w.kind[gt]);
        if (kind == LEAF_NONE || kind == LEAF_NEW_REPLY) { dev_error(d, DERR_STATE); return; }
        const int leaf = uni(w.leaf[gt]);
        const NodeMeta m = d.node[nb + leaf].meta;
        double v;
        if (m.result != RESULT_NONE) {
            v = (double)m.result;                                      // state.get_result() (mctree.py:268)
        } else {
            v = (double)val2[row];
            gather_priors(d, row, eb, m.edge0, m.nmoves, pol2, lane, FMT_FULL);
            evals += 1;
        }
        if (kind == LEAF_NEW_S2) evals += 1;                           // policy(S1) chose the reply
        const int plen = uni(w.plen[gt]);
        const int32_t *pe = w.path_edge + (size_t)t * d.G * d.N + nb;
        for (int l = lane; l < plen; l += 64) {
            Edge *e = d.edge + eb + pe[l];
            e->visits += 1;
            e->value = __dadd_rn(e->value, v);
        }
        depth += plen;
        if (kind == LEAF_TERMINAL_HIT) term += 1;
        else { nodes += 1; branch += m.nmoves; }
        __threadfence_block();
        __syncthreads();                                               // the next leaf adds into the same sums
    }
    if (lane == 0) {
        d.game[g].root_visits += nl;
        w.n_leaves[g] = 0;
        unsigned long long *c = d.counters + (size_t)g * CNT_N;
        c[CNT_SIMS] += nl; c[CNT_DEPTH] += depth; c[CNT_EVALS] += evals;
        c[CNT_TERMINAL] += term; c[CNT_NODES] += nodes; c[CNT_BRANCH] += branch;
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
    const size_t nb = (size_t)g * d.N, eb = (size_t)g * d.ECAP;
    const bool legacy = (d.flags & 1u) != 0;
    const int p = uni(d.game[g].ply);
    if (d.ECAP >= (1 << HINT_EDGE_BITS)) { dev_error(d, DERR_EDGE_POOL); return; }
    int nn = uni(d.game[g].n_nodes);
    u64 fresh = 0;                                                     // bit t: leaf t was created by this wave
    int cnt = 0;
    bool stop = false;
    for (int t = 0; t < W && !stop; t++) {
        const Dev dt = thread_view(d, w, t);
        const size_t gt = (size_t)g * w.T + t;
        const int row = r * w.T + t;
        int node = 0, level = 0, last_edge = -1;
        int edge0 = 0, nmoves = 0, nexp = 0, result = RESULT_NONE, parent_edge = -1;
        bool need_meta = true, made = false;
        if (lane == 0) dt.path_node[nb] = 0;
        for (;;) {
            if (need_meta) {
                NodeMeta m = d.node[nb + node].meta;
                edge0 = uni(m.edge0); nmoves = uni(m.nmoves); nexp = uni(m.nexp);
                result = uni(m.result); parent_edge = uni(m.parent_edge);
            }
            if (result != RESULT_NONE) {                               // is_terminal_state: the leaf is this node again
                if (level == 0) { dev_error(d, DERR_STATE); stop = true; break; }
                if (lane == 0) { w.kind[gt] = LEAF_TERMINAL_HIT; w.leaf[gt] = (u16)node; s_ledge[t] = last_edge; }
                made = true;
                break;
            }
            if (nexp < nmoves) {                                       // not fully expanded: expand ONE child
                const int j = nmoves - 1 - nexp;
                const int edge = edge0 + j;
                const u32 mv = d.edge[eb + edge].move;
                const int c = nn;
                if (c >= d.N || level + 1 >= d.N) { dev_error(d, DERR_NODE_POOL); stop = true; break; }
                if (lane == 0) {
                    d.node[nb + node].meta.nexp = (u16)(nexp + 1);
                    if (nexp + 1 == nmoves && parent_edge >= 0)
                        d.edge[eb + parent_edge].pad = hint_pack(edge0, nmoves);
                    dt.path_edge[nb + level] = edge;
                    dt.path_node[nb + level + 1] = (u16)c;
                    s_ledge[t] = edge;
                }
                nn = c + 1;
                level++;
                Board parent = d.node[nb + node].s2;
                Board s1 = apply_move(parent, mv);
                __threadfence_block();
                __syncthreads();                                       // path_node visible
                PosEval e = eval_position(dt, g, s1, 2 * level - 1, p, p, lane, s);
                NodeMeta cm;
                cm.edge0 = 0; cm.nmoves = (u16)e.n; cm.nexp = 0; cm.result = (int8_t)e.result;
                cm.has_s2 = 0; cm.parent = (u16)node; cm.parent_edge = edge;
                if (lane == 0) {
                    d.node[nb + c].s1 = e.b;
                    d.node[nb + c].h1 = e.hash;
                    d.node[nb + c].meta = cm;
                    w.leaf[gt] = (u16)c;
                }
                if (e.result != RESULT_NONE) {                         // game ended on our move
                    if (lane == 0) {
                        d.node[nb + c].s2 = e.b;
                        d.node[nb + c].h2 = e.hash;
                        d.edge[eb + edge].child = (u16)(c | CHILD_TERMINAL);
                        w.kind[gt] = LEAF_NEW_S1_OVER;
                    }
                } else {
                    for (int i = lane; i < e.n; i += 64) w.s1_moves[gt * MAX_MOVES + i] = s.mv[i];
                    if (lane == 0) {
                        d.edge[eb + edge].child = (u16)c;
                        w.s1_n[gt] = e.n;
                        w.kind[gt] = LEAF_NEW_REPLY;
                    }
                    __syncthreads();
                    encode_position(dt, g, e.b, 2 * level - 1, p, p, lane, s, planes1, row);
                }
                fresh |= 1ull << t;
                made = true;
                break;
            }
            // ---- get_best_child on (Q + U) - vloss, first max in children order = the LARGEST legal index among equals
            double best = -__builtin_inf();
            int bj = -1, bchild = 0;
            u32 bhint = 0;
            for (int base = 0; base < nmoves; base += 64) {
                const int j = base + lane;
                if (j < nmoves) {
                    const Edge e = d.edge[eb + edge0 + j];
                    const int n = e.visits;
                    const bool term = (e.child & CHILD_TERMINAL) != 0;
                    const double den = (double)(1 + n);
                    const double q = __ddiv_rn(e.value, den);
                    const double sumv = (term || n == 0) ? 0.0 : (double)(n - 1);
                    const double cp = legacy ? __dmul_rn(10.0, (double)e.prior)
                                             : (double)__fmul_rn(10.0f, e.prior);
                    const double u = __dmul_rn(cp, __ddiv_rn(__dsqrt_rn(sumv), den));
                    int vl = 0;
                    for (int k = 0; k < cnt; k++) vl += s_ledge[k] == edge0 + j ? 1 : 0;
                    const double sc = __dsub_rn(__dadd_rn(q, u), (double)vl);
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
            bj = uni(bj);
            const int edge = edge0 + bj;
            // stepping onto a node this wave created: its S2 does not exist yet -- the wave ends here
            const bool on_fresh = lane < cnt && ((fresh >> lane) & 1) && s_ledge[lane] == edge;
            if (__ballot(on_fresh) != 0) { stop = true; break; }
            const int child = uni(bchild) & CHILD_NONE;
            if (level + 1 >= d.N) { dev_error(d, DERR_NODE_POOL); stop = true; break; }
            if (lane == 0) {
                dt.path_edge[nb + level] = edge;
                dt.path_node[nb + level + 1] = (u16)child;
            }
            level++;
            node = child;
            last_edge = edge;
            const u32 hint = uni(bhint);
            if (uni(bchild) & CHILD_TERMINAL) {
                need_meta = false;
                result = 0;
            } else if (hint & HINT_FULL) {
                need_meta = false;
                edge0 = (int)(hint & ((1u << HINT_EDGE_BITS) - 1)); nmoves = (int)((hint >> HINT_EDGE_BITS) & 0xFFu); nexp = nmoves;
                result = RESULT_NONE;
            } else {
                need_meta = true;
            }
        }
        if (made) {
            if (lane == 0) w.plen[gt] = level;
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
    const size_t nb = (size_t)g * d.N, eb = (size_t)g * d.ECAP;
    const int p = uni(d.game[g].ply);
    int top = uni(d.game[g].edge_top);
    for (int t = 0; t < nl; t++) {
        const size_t gt = (size_t)g * w.T + t;
        if (uni(w.kind[gt]) != LEAF_NEW_REPLY) continue;
        const Dev dt = thread_view(d, w, t);
        const int row = r * w.T + t;
        const int c = uni(w.leaf[gt]), level = uni(w.plen[gt]), n1 = uni(w.s1_n[gt]);
        Board s1 = d.node[nb + c].s1;
        // agent.best_move(S1, real_game=True): legal[argmax(policy masked to legal)]
        const u16 *mv1 = w.s1_moves + gt * MAX_MOVES;
        const int bi = argmax_policy(d, row, mv1, n1, pol1, lane, FMT_FULL);
        const u32 reply = mv1[bi];
        Board s2 = apply_move(s1, reply);
        PosEval e = eval_position(dt, g, s2, 2 * level, p, p, lane, s);
        const int edge0 = top;                                         // edge runs in thread order: the same tree every run
        if (edge0 + e.n > d.ECAP) { dev_error(d, DERR_EDGE_POOL); return; }
        init_edges(d, eb, edge0, e.n, s.mv, lane);
        top = edge0 + e.n;
        if (lane == 0) {
            NodeMeta m = d.node[nb + c].meta;
            m.edge0 = edge0; m.nmoves = (u16)e.n; m.nexp = 0; m.result = (int8_t)e.result; m.has_s2 = 1;
            d.node[nb + c].meta = m;
            d.node[nb + c].s2 = e.b;
            d.node[nb + c].h2 = e.hash;
            d.node[nb + c].reply = (u16)reply;
            d.game[g].edge_top = top;
            if (e.result != RESULT_NONE) d.edge[eb + m.parent_edge].child = (u16)(c | CHILD_TERMINAL);
            w.kind[gt] = LEAF_NEW_S2;
        }
        __syncthreads();
        encode_position(dt, g, e.b, 2 * level, p, p, lane, s, planes2, row);
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
