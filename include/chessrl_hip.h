/*
 * chessrl_hip.h -- C-ABI of libchessrl_hip.so, the MI355X (gfx950) drop-in for
 * the self-play MCTS simulation loop of AIRLegend/ChessRL.
 *
 * The reference is pure Python and defines no FFI; its seams for this path are
 * duck-typed Python methods.  Each entry point below
 * names the reference method(s) it replaces (paths relative to
 * /root/reference/src/chessrl/).  The Python host mirror (chessrl_amd/game.py,
 * agent.py, mctree.py, selfplay.py) binds these with ctypes; INTEGRATION.md
 * shows the stub a reference maintainer would add.
 *
 * Conventions: plain pointers and sizes, no torch types; every call returns 0
 * on success or a negative crl_status and records a message retrievable with
 * crl_last_error(); one context per GPU, not thread-safe per context; "dev_"
 * pointers are device memory (e.g. torch.Tensor.data_ptr()), all others are
 * caller-owned host memory; kernels are enqueued on the stream given to
 * crl_set_stream() (torch's current stream) so they order with the tower and
 * can be captured into a hipGraph; calls that fill host buffers synchronise
 * that stream themselves.  G = max_games given to crl_create.
 */
#ifndef CHESSRL_HIP_H
#define CHESSRL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One chess position, 64 bytes.  Squares a1 = 0 ... h8 = 63 (python-chess). */
typedef struct crl_board {
    uint64_t bb[6];   /* pawns, knights, bishops, rooks, queens, kings (both colours) */
    uint64_t white;   /* squares occupied by white pieces                              */
    uint32_t state;   /* bit 0      side to move (1 = white)
                         bits 1-4   castling rights: WK(h1) WQ(a1) BK(h8) BQ(a8)
                         bits 5-11  en-passant square, 64 = none (set on EVERY double push)
                         bits 12-19 halfmove clock (saturates at 255)
                         bit 20     a legal en-passant capture exists (derived; recomputed
                                    by the library, ignored on input)                   */
    uint32_t pad;
} crl_board;

/* A move is a uint16: from | to << 6 | promo << 12, promo in {0, 2=N, 3=B, 4=R, 5=Q};
 * castling is the king move (e1g1), as python-chess prints it.  0xFFFF = "no move". */
#define CRL_NO_MOVE 0xFFFFu
#define CRL_MAX_MOVES 256      /* row stride of every per-position move list           */
#define CRL_N_LABELS 1968      /* netencoder.get_uci_labels(), netencoder.py:94-134     */
#define CRL_PLANES 128         /* 127 reference planes + 1 zero pad, fp16 NHWC          */
#define CRL_RESULT_NONE 2      /* Game.get_result() is None                             */

typedef enum crl_status {
    CRL_OK = 0,
    CRL_ERR_ARG = -1,          /* bad argument                                          */
    CRL_ERR_HIP = -2,          /* HIP runtime failure (message has the hipError string) */
    CRL_ERR_CAPACITY = -3,     /* a device pool overflowed (nodes / edges / plies)      */
    CRL_ERR_STATE = -4         /* call not valid in the current search state            */
} crl_status;

/* crl_create flags */
#define CRL_FLAG_NUMPY_LEGACY 1u  /* PUCT: 10*prior evaluated in float64 (numpy 1.x scalar
                                     promotion, the reference's pinned numpy==1.17.2);
                                     default is numpy>=2 (product rounded to float32).  */

typedef struct crl_ctx crl_ctx;

/* ---- identity of the library ------------------------------------------------------------- */
/* Bumped whenever a signature or the meaning of an argument below changes.  A binding calls
 * crl_abi_version() first and refuses a library of another version (a ctypes call through a stale
 * signature hands the GPU garbage pointers).  crl_source_hash(): sha256 over the sources (csrc/ + this
 * header + compiler flags) the library was built from, as chessrl_amd/_lib.py computes it; the string
 * is also findable in the file itself behind the marker "CRL_SRC_HASH=".  No reference counterpart.
 * (The _ord, _rep, _ev, _sel and _exc entries of the built-in opponent, crl_opponent_evaluate and
 * crl_opponent_exchange are additions that change no existing signature or meaning: still 9.) */
#define CRL_ABI_VERSION 9
int  crl_abi_version(void);
const char *crl_source_hash(void);

/* ---- lifetime ------------------------------------------------------------------- */
int  crl_create(crl_ctx **out, int device, int max_games, int max_sims, int max_plies,
                uint32_t flags);
void crl_destroy(crl_ctx *ctx);
int  crl_set_stream(crl_ctx *ctx, void *hip_stream);
int  crl_sync(crl_ctx *ctx);                 /* wait for the stream; report device errors */
const char *crl_last_error(crl_ctx *ctx);    /* ctx may be NULL for crl_create failures   */
/* Restrict every later call to slots [first, first+count): host arrays and dev_ rows are then
 * indexed relative to `first` and sized by `count` instead of G (default window = all G). */
int  crl_set_window(crl_ctx *ctx, int first, int count);
/* What the encoding entry points (crl_encode, crl_search_begin, crl_sim_select_expand,
 * crl_sim_reply: netencoder.get_game_state, netencoder.py:72-91) write per position:
 * CRL_PLANES_F16 (default) = the fp16 NHWC planes [8][8][128] (16 KiB);
 * CRL_PLANES_BITS = the same information as 128 plane bitboards, uint64 [128] (1 KiB; bit s of
 * plane c = channel c on square s, a1 = 0): the input of crl_trunk_forward_bitplanes, which expands
 * it on chip, so that the planes never exist in HBM. */
#define CRL_PLANES_F16  0
#define CRL_PLANES_BITS 1
int  crl_set_plane_format(crl_ctx *ctx, int format);
/* What the evaluator hands back to crl_sim_select_expand / crl_sim_reply / crl_sim_backup as
 * "policy" (mctree.py:298-303 _update_prior and agentdistributed.py:80-82 read the 1968-vector only
 * at the labels of the position's legal moves):
 * CRL_POLICY_FULL (default) = dev_policy rows are float32 [1968], the kernels gather at the labels;
 * CRL_POLICY_LEGAL = dev_policy rows are float32 [CRL_MAX_MOVES]: entry j is the probability of the
 * position's legal move j (crl_legal_moves order).  The search kernels then publish, for the position
 * each tower call evaluates, the labels of its legal moves: crl_eval_labels(ctx, 0, ...) after
 * crl_sim_select_expand (S1), crl_eval_labels(ctx, 1, ...) after crl_sim_reply (S2): device pointers
 * to uint16 [count][CRL_MAX_MOVES] and int32 [count] (0 = this row needs no policy in this step),
 * rows window-relative, valid for the life of the context.  crl_heads_forward_legal consumes them.
 * crl_search_root_priors and crl_greedy_moves always take full policies.
 * CRL_POLICY_LEGAL_RAW = rows as CRL_POLICY_LEGAL, but holding the LOGITS of the legal moves, with the
 * softmax statistics of the board (8 label slices x (max, sum exp), float [rows][16]) at the address given
 * to crl_set_policy_stats(ctx, which, ...) (which = 0: the evaluation of S1, read by crl_sim_reply; 1: of
 * S2, read by crl_sim_select_expand / crl_sim_backup): the kernels form exp(l - M) / S on read -- the
 * arithmetic of the heads' normalising pass, same bits -- so small batches need no such pass
 * (crl_heads_forward_legal_raw).  Both addresses must be set before the format is selected. */
#define CRL_POLICY_FULL  0
#define CRL_POLICY_LEGAL 1
#define CRL_POLICY_LEGAL_RAW 2
int  crl_set_policy_format(crl_ctx *ctx, int format);
int  crl_set_policy_stats(crl_ctx *ctx, int which, const void *dev_stats_f32);
int  crl_eval_labels(crl_ctx *ctx, int which, const uint16_t **dev_labels, const int32_t **dev_counts);
int  crl_max_games(crl_ctx *ctx);
int  crl_max_sims(crl_ctx *ctx);

/* netencoder.get_uci_labels (netencoder.py:94-134): move id of each of the 1968 labels */
int  crl_uci_label_moves(uint16_t *moves_out /*1968*/);

/* ---- Game seam (game.py) ------------------------------------------------------------ */
/* Game.__init__/reset (game.py:17-26,82-83): slots with mask[g] != 0 (NULL = all)
 * restart from the standard position with an empty move stack. */
int  crl_reset_games(crl_ctx *ctx, const uint8_t *mask);
/* Game(board=...) / set_fen (game.py:17-21,71-72): slots 0..n-1 take `boards` with an
 * EMPTY move stack (tests: arbitrary positions). */
int  crl_set_positions(crl_ctx *ctx, const crl_board *boards, int n);
int  crl_get_positions(crl_ctx *ctx, crl_board *boards_out, int n);
/* Game.get_copy (game.py:79-80): slot dst becomes a deep copy (board AND move stack) of
 * slot src; absolute slot numbers, independent of the window. */
int  crl_copy_game(crl_ctx *ctx, int dst, int src);
/* Tree.__init__ (mctree.py:105-109, ``Node(root.get_copy())``) and Game(board=other.board) when the
 * two games live in different contexts of one GPU (the Game arena and a search engine): slot dst
 * of ctx becomes a deep copy of slot src of src_ctx -- position, move stack and the history the
 * encoder and the repetition rule read -- whatever position the source game started from.
 * The record must fit ctx's max_plies (CRL_ERR_CAPACITY otherwise).  Absolute slot numbers. */
int  crl_copy_game_from(crl_ctx *ctx, int dst, crl_ctx *src_ctx, int src);
/* Game.get_legal_moves (game.py:43-57): python-chess generation order.  moves may be NULL when
 * only len(get_legal_moves()) is wanted (the 512-byte rows are then not copied back). */
int  crl_legal_moves(crl_ctx *ctx, uint16_t *moves /*G x 256*/, int32_t *counts /*G*/);
/* Game.move (game.py:28-41): applied iff in the legal list; ok[g] = 1/0; CRL_NO_MOVE skips. */
int  crl_push_moves(crl_ctx *ctx, const uint16_t *moves /*G*/, uint8_t *ok /*G*/);
/* DatasetGame.loads / augment_game (dataset.py:21-57): every game replays its own recorded move
 * list moves[g*stride .. g*stride+counts[g]) in ONE launch, each move through Game.move's legality
 * test; pushed[g] = number of moves applied (stops at the first illegal move or CRL_NO_MOVE). */
int  crl_push_sequences(crl_ctx *ctx, const uint16_t *moves /*G x stride*/, const int32_t *counts /*G*/,
                        int stride, int32_t *pushed /*G*/);
/* Game.get_result (game.py:92-109): 1 / -1 / 0, CRL_RESULT_NONE while running. */
int  crl_results(crl_ctx *ctx, int8_t *result /*G*/);
/* len(Game) and Game.get_history()['moves'] (game.py:59-66,111-112). */
int  crl_records(crl_ctx *ctx, uint16_t *moves /*G x max_plies or NULL*/, int32_t *plies /*G*/,
                 int8_t *result /*G or NULL*/);

/* ---- encoder seam (netencoder.py) ------------------------------------------------------ */
/* netencoder.get_game_state (netencoder.py:72-91) for every slot: fp16 NHWC
 * [G][8][8][128] (row 0 = rank 8, col 0 = file a; channel 127 is a zero pad). */
int  crl_encode(crl_ctx *ctx, void *dev_planes_f16);

/* ---- Agent seam (agentdistributed.py) ----------------------------------------------- */
/* AgentDistributed.best_move(real_game=True) (agentdistributed.py:56-58): per slot with
 * mask[g] != 0 (NULL = all): legal[argmax(policy[label(m)] for m in legal)], first max.
 * dev_policy_f32 is [G][1968].  If push != 0 the move is also played (selfplay.py:68-70).
 * moves_out (host, may be NULL) receives the chosen move ids (CRL_NO_MOVE if game over). */
int  crl_greedy_moves(crl_ctx *ctx, const void *dev_policy_f32, const uint8_t *mask, int push,
                      uint16_t *moves_out);

/* ---- SelfPlayTree seam (mctree.py), lockstep over all slots, threads=1 semantics -------- */
/* Tree.__init__ (mctree.py:105-111): fresh tree per slot, root = current game, visits 1.
 * Finished games get an inert root.  Also encodes every root into dev_planes_f16 (the
 * reference evaluates the root's policy in _update_prior, mctree.py:298-303). */
int  crl_search_begin(crl_ctx *ctx, void *dev_planes_f16);
/* Root part of _update_prior: priors of the root's children from the tower's policy. */
int  crl_search_root_priors(crl_ctx *ctx, const void *dev_policy_f32);
/* First half of explore_tree (mctree.py:200-257): [backprop of the previous simulation
 * (mctree.py:278-296) if one is pending, using the S2 outputs], then select to a leaf,
 * pop the last unexpanded move, play it (S1) and encode S1 where the opponent must reply.
 * dev_policy_s2/dev_value_s2 may be NULL only when no simulation is pending. */
int  crl_sim_select_expand(crl_ctx *ctx, const void *dev_policy_s2_f32,
                           const void *dev_value_s2_f32, void *dev_planes_s1_f16);
/* Second half of expand (mctree.py:244-250): opponent's greedy reply from policy(S1),
 * S2 = S1 + reply, Node(S2) with its legal moves, encode S2. */
int  crl_sim_reply(crl_ctx *ctx, const void *dev_policy_s1_f32, void *dev_planes_s2_f16);
/* simulate + backprop + child priors (mctree.py:259-303) for the pending simulation. */
int  crl_sim_backup(crl_ctx *ctx, const void *dev_policy_s2_f32, const void *dev_value_s2_f32);
/* [c.visits for c in root.children] etc., CHILDREN order (= reverse legal order);
 * rows of 256; any output may be NULL. */
int  crl_root_children(crl_ctx *ctx, int32_t *nchild /*G*/, int32_t *visits, double *values,
                       float *priors, uint16_t *moves, uint16_t *replies, int32_t *root_visits);
/* selfplay.play_game's two pushes (selfplay.py:77-78) for the chosen root child per slot
 * (children-order index, -1 = leave the slot alone).  bm/am (host, may be NULL) get our
 * move and the stored reply (CRL_NO_MOVE when the game ended on our move). */
int  crl_advance(crl_ctx *ctx, const int32_t *chosen /*G*/, uint16_t *bm, uint16_t *am);
/* gam.move(bm) alone: Agent.best_move in a game whose other side moves for itself (gameagent.py,
 * benchmark.py:100-118).  crl_advance's checks and its bm; the game goes on by ONE ply, to the position after
 * our move, and the stored reply is not played: the other side's move comes from its own search and
 * arrives through crl_push_moves.  The tree is consumed.  A child on which the game ended is played
 * exactly as by crl_advance.  Window-relative like crl_advance; bm (host, may be NULL).
 * (An addition that changes no existing signature: still 9.) */
int  crl_advance_one(crl_ctx *ctx, const int32_t *chosen /*G*/, uint16_t *bm /*G*/);
/* The noise-free one-ply boundary without the host (gameagent.py; the choice is compute_policy followed by
 * np.argmax, mctree.py:305-322): crl_root_children, the choice and crl_advance_one in one kernel.  A slot moves iff its
 * tree is alive, its game has no result, its ply count is below dev_ply_limit[g], the side to move is mover_white
 * (1 white, 0 black) and its root has an expanded child.  The chosen child is the first maximum of the root
 * children's visits in CHILDREN order -- what the policy visits**(1/tau) / root_visits**(1/tau) and np.argmax choose
 * for every tau, since the policy is strictly increasing in visits.  The slot is advanced as by crl_advance_one.
 * dev_bm[g] / dev_chosen[g] (DEVICE memory): the move and the child, CRL_NO_MOVE / -1 for a slot that does not move
 * and whose state is untouched.  Asynchronous on the context's stream; window-relative; a device error shows at the
 * next synchronising call.  (An addition that changes no existing signature: still 9.) */
int  crl_advance_one_argmax(crl_ctx *ctx, int mover_white, const int32_t *dev_ply_limit /*G*/,
                            uint16_t *dev_bm /*G*/, int32_t *dev_chosen /*G*/);
/* crl_push_moves with the moves already in DEVICE memory (crl_advance_one_argmax's dev_bm of the mirror context, on
 * the same stream) and no synchronisation: Game.move (game.py:28-41) per slot, CRL_NO_MOVE skips.  dev_ok (device,
 * may be NULL) gets 1/0.  A refused move is a device error (CRL_ERR_STATE) at the next synchronising call.
 * (An addition that changes no existing signature: still 9.) */
int  crl_push_moves_dev(crl_ctx *ctx, const uint16_t *dev_moves /*G*/, uint8_t *dev_ok /*G, may be NULL*/);
/* The move boundary of the lockstep runner in TWO synchronising calls instead of five (a synchronisation costs
 * ~70 us; at C2 a move is 13 ms).  crl_end_move_fetch = crl_sim_backup + crl_root_children(nchild, visits,
 * root_visits) + len(Game) of every slot; the host then computes the policies (compute_policy, mctree.py:305-322)
 * and crl_advance_fetch = crl_advance + crl_results + the number of legal moves of every NEXT root
 * (len(get_legal_moves()): how many children the next search can have -- the runner draws its Dirichlet
 * noise ahead with it).  Same kernels, same values as the single calls. */
int  crl_end_move_fetch(crl_ctx *ctx, const void *dev_policy_s2_f32, const void *dev_value_s2_f32,
                        int32_t *nchild /*G*/, int32_t *visits /*G x 256*/, int32_t *root_visits /*G*/,
                        int32_t *plies /*G*/);
int  crl_advance_fetch(crl_ctx *ctx, const int32_t *chosen /*G*/, uint16_t *bm, uint16_t *am,
                       int8_t *results /*G*/, int32_t *legal_counts /*G*/);
/* Tree(Node) (mctree.py:98-111: "You can pass a Node object with a Game as state or directly the game"):
 * crl_advance's two pushes, and the chosen child KEEPS its subtree and becomes the root of the next search
 * (visits 1, mctree.py:111).  Decided per slot on the device: kept iff the child's state is S2 and the game
 * goes on and kept nodes + next_sims <= max_sims + 1 (the node pool of crl_create; one simulation creates at
 * most one node, so the pool cannot overflow during the next move).  Every other slot ends exactly as after
 * crl_advance: no live tree, fresh tree at the next begin.  The kept tree is compacted in place (ids dense
 * from 0, edge runs contiguous); value sums, visits and priors move as bit patterns.
 * crl_search_begin_kept is crl_search_begin that leaves kept roots alone (only the pending-simulation
 * state is reset; the following crl_search_root_priors skips them and counts no evaluation for them), so a
 * batch mixes kept and fresh roots; plain crl_search_begin starts a fresh tree in every slot.
 * crl_reroot_fetch is the fused boundary form, crl_advance_fetch + kept_nodes (0 = fresh tree next) and
 * kept_children (children the kept root already has: the next search ends with
 * min(legal moves, kept_children + simulations) of them). */
int  crl_reroot(crl_ctx *ctx, const int32_t *chosen /*G*/, int next_sims, uint16_t *bm, uint16_t *am);
int  crl_reroot_fetch(crl_ctx *ctx, const int32_t *chosen /*G*/, int next_sims, uint16_t *bm, uint16_t *am,
                      int8_t *results /*G*/, int32_t *legal_counts /*G*/, int32_t *kept_nodes /*G*/,
                      int32_t *kept_children /*G*/);
int  crl_search_begin_kept(crl_ctx *ctx, void *dev_planes_f16);
/* crl_copy_game that carries a live tree along (nodes, edges, root visits, the kept mark): the lockstep
 * runner moves games between slots at a move boundary.  crl_copy_game itself leaves no tree in dst. */
int  crl_copy_game_tree(crl_ctx *ctx, int dst, int src);
/* Debug read-back of one slot's tree: 176-byte node records and 24-byte edge records as the kernels keep
 * them (csrc/state.hpp), info = {nodes, edges, root visits, kept mark}; nodes / edges may be NULL. */
int  crl_fetch_tree(crl_ctx *ctx, int slot, void *nodes, int node_cap, void *edges, int edge_cap,
                    int32_t *info /*4*/);
/* Device-side counters since crl_create: [0] simulations run, [1] nodes created,
 * [2] sum of selection depth (edges), [3] sum of legal moves over created nodes,
 * [4] tower evaluations consumed, [5] terminal leaves hit. */
int  crl_counters(crl_ctx *ctx, uint64_t *out6);

/* ---- random playouts: RandomSimulation.run (simulation.py:19-34), the leaf evaluator SelfPlayTree.simulate
 * names beside predict_outcome (mctree.py:272-274).  csrc/rollout.hpp states the ply, the choice rule
 * (CPython's random.choice, word for word) and the counter generator of the private form. ------------------- */
#define CRL_ROLLOUT_GAMES  0   /* roots = the current position of every slot of the window                 */
#define CRL_ROLLOUT_LEAVES 1   /* roots = S2 of the pending leaf of every slot of a running search           */
#define CRL_ROLLOUT_SKIPPED 0xFFFFu   /* dev_plies_u16 of a slot that had no playout to run                */
/* The in-slot form (simulation.py:19-34 as written; mctree.py:272-274 calls it on the leaf's own game): every
 * slot of the window plays ITS game on by random moves -- history, move record, ply count and result change as
 * by crl_push_moves -- taking 32-bit words from words[g*stride .. g*stride+counts[g]) (host; random.choice
 * consumes one MT19937 output per word).  A slot stops when its game has a result, when chunks * max_moves plies
 * have been played since the run began, or when its words run out: played[g] (host, in/out; 0 at the start of a
 * run) counts the plies of the run, and a caller whose slot stopped for want of words calls again with the
 * following words and the played[] it got back.  used[g] = words this call consumed; chunk_results[g*chunks + c] =
 * Game.get_result() after chunk c of max_moves plies (CRL_RESULT_NONE where the game went on), final once the
 * slot's run is over.  CRL_ERR_ARG: chunks < 1, max_moves < 0, stride < 1, a NULL array. */
int  crl_rollout_games(crl_ctx *ctx, const uint32_t *words /*G x stride*/, const int32_t *counts /*G*/, int stride,
                       int chunks, int max_moves, int32_t *played /*G*/, int32_t *used /*G*/,
                       int8_t *chunk_results /*G x chunks*/);
/* The private form (simulation.py:19-34 with independent repetitions, mctree.py:272-274): `repetitions` playouts
 * of at most max_moves plies from every root, nothing of the game state written; a playout still running after
 * max_moves plies counts 0.  Everything is device memory and the call only enqueues (it captures into a hipGraph):
 * dev_keys uint64 [G] = the stream key of every slot (read at run time), dev_value_f32 [G] =
 * (float)((double)sum of results / repetitions), dev_results_i8 / dev_plies_u16 [G][repetitions] = result and
 * plies of every playout (either may be NULL: the library then keeps them in a buffer of its own, grown by a
 * device allocation when a call needs more than any before -- pass both inside a graph capture).
 * root_source CRL_ROLLOUT_LEAVES: a slot with no pending simulation, a terminal leaf or a leaf that ended on our
 * move gets value 0 and CRL_ROLLOUT_SKIPPED plies (the backup does not read the value there); the simulation
 * index of the generator is the number of simulations the current search has backed up.
 * CRL_ERR_ARG: repetitions < 1, max_moves < 0 or > 65534, a NULL key or value array, an unknown root source;
 * CRL_ERR_STATE: CRL_ROLLOUT_LEAVES on a context where no search was ever begun.  No state changes on an error. */
int  crl_rollout(crl_ctx *ctx, int root_source, int repetitions, int max_moves, const uint64_t *dev_keys,
                 void *dev_value_f32, int8_t *dev_results_i8, uint16_t *dev_plies_u16);

/* ---- the built-in opponent: a fixed-depth alpha-beta player per slot (csrc/opponent.hpp states the search, the
 * node value, the move order, the static evaluation and the node limit).  It stands where the reference calls its
 * engine: Stockfish.best_move (stockfish.py:23-31, engine.play(board, Limit(depth))) and the reply inside
 * GameStockfish.move (gamestockfish.py:27-41).  It is not that engine: repetition below the root only on request (the _rep calls), quiescence
 * only through the _q calls below, no time control, no Elo.  Host arrays, synchronous, window-relative like crl_greedy_moves.
 * depths[g] (host int32): 0 leaves slot g alone, 1 .. CRL_OPP_MAX_DEPTH searches it to that depth -- the array is
 * both the mask and the per-game depth.  node_limit >= 1 bounds the nodes (move generations) of every slot: a slot
 * that reaches it returns the best root move among those completely searched, or its first legal move, and the flag
 * CRL_OPP_CUT.  A slot whose game already has a result returns CRL_NO_MOVE and CRL_OPP_SKIPPED.  If push != 0 the
 * chosen move is played: history, record, ply and result change as by crl_push_moves.
 * moves[g] = the move (CRL_NO_MOVE for depth 0 and skipped slots); scores[g] = its score from the side to move
 * (mate in k plies = 30000 - k); nodes[g] = nodes generated; flags[g]; the last three may be NULL.
 * CRL_ERR_ARG: NULL depths or moves, a depth outside 0 .. CRL_OPP_MAX_DEPTH, node_limit < 1.  No state changes on
 * an error. */
#define CRL_OPP_MAX_DEPTH 5
#define CRL_OPP_CUT 1
#define CRL_OPP_SKIPPED 2
int  crl_opponent_moves(crl_ctx *ctx, const int32_t *depths /*G*/, int push, int64_t node_limit,
                        uint16_t *moves /*G*/, int32_t *scores /*G*/, int64_t *nodes /*G*/, uint8_t *flags /*G*/);
/* crl_sim_reply with the built-in opponent as the mover: the second half of expand (mctree.py:244-246), where the
 * reply to S1 comes from a game that answers every move of ours with its engine (gamestockfish.py:27-41) instead of
 * from policy(S1).  The search above runs from the pending node's S1 to depth dev_depths_i32[row] under node_limit;
 * its move -- a function of the board alone, hence the move crl_opponent_moves plays from S1 -- is stored as the
 * node's reply, then S2, Node(S2) and the planes of S2 exactly as by crl_sim_reply (labels of S2 in the legal-label
 * policy formats included).  A cut reply (node limit) is still a move and is stored like any other.  No tower call
 * on S1 is needed in such a step.  All pointers are DEVICE pointers, rows window-relative, so the call captures
 * into a hipGraph: dev_depths_i32 int32 [count]; dev_nodes_u64 / dev_cuts_u32 [count] accumulate the nodes searched
 * and the number of cut replies per row (the caller clears them).  Rows without a pending reply read no depth.
 * CRL_ERR_ARG: a NULL pointer, node_limit < 1.  A depth outside 1 .. CRL_OPP_MAX_DEPTH on a row that needs a reply
 * is a device error (reported as CRL_ERR_STATE by the next synchronising call). */
int  crl_sim_reply_opponent(crl_ctx *ctx, const int32_t *dev_depths_i32, int64_t node_limit, void *dev_planes_s2,
                            uint64_t *dev_nodes_u64, uint32_t *dev_cuts_u32);
/* The two calls above with `quiescence` plies of quiescence search past the fixed depth, one value per call:
 * 0 .. CRL_OPP_MAX_QUIESCENCE (csrc/opponent.hpp, QUIESCENCE: stand-pat, the tactical moves by victim, every evasion
 * when in check, the static evaluation after the last ply).  quiescence = 0 is the call above: the same moves, scores,
 * node counts and flags, from the same kernel.  Node counts grow with quiescence; node_limit bounds them as before.
 * CRL_ERR_ARG: what the call above refuses, or a quiescence outside 0 .. CRL_OPP_MAX_QUIESCENCE.  No state changes
 * on an error. */
#define CRL_OPP_MAX_QUIESCENCE 6
int  crl_opponent_moves_q(crl_ctx *ctx, const int32_t *depths /*G*/, int quiescence, int push, int64_t node_limit,
                          uint16_t *moves /*G*/, int32_t *scores /*G*/, int64_t *nodes /*G*/, uint8_t *flags /*G*/);
int  crl_sim_reply_opponent_q(crl_ctx *ctx, const int32_t *dev_depths_i32, int quiescence, int64_t node_limit,
                              void *dev_planes_s2, uint64_t *dev_nodes_u64, uint32_t *dev_cuts_u32);
/* The two _q calls with ITERATIVE DEEPENING under a node budget (csrc/opponent.hpp states the rule), the deterministic
 * counterpart of the reference's Limit(time=...) (stockfish.py:14-21).  depths[g] is now the MAXIMUM depth of slot g:
 * the slot searches depth 1, 2, ... with one node counter, the best move of an iteration first at the root of the
 * next, and stops when the counter reaches node_budget >= 1, so no slot costs more than node_budget nodes.  It plays
 * the result of the deepest iteration it finished, or the best completely searched root move of the iteration the
 * budget stopped; depths_done[g] (host int32 / dev_depth_sum_u64[row] accumulates it) is the last finished iteration,
 * and CRL_OPP_CUT means depths_done[g] < depths[g].  Everything else -- depth 0, finished games, push, quiescence,
 * the node and cut accumulators, the stored reply -- is as in the calls above; depths_done may be NULL.  The calls
 * above do not change: they launch the kernels they launched.
 * CRL_ERR_ARG: what the calls above refuse (NULL dev_depth_sum_u64 included), with node_budget in node_limit's place.
 * No state changes on an error. */
int  crl_opponent_moves_id(crl_ctx *ctx, const int32_t *depths /*G*/, int quiescence, int push, int64_t node_budget,
                           uint16_t *moves /*G*/, int32_t *scores /*G*/, int64_t *nodes /*G*/, uint8_t *flags /*G*/,
                           int32_t *depths_done /*G*/);
int  crl_sim_reply_opponent_id(crl_ctx *ctx, const int32_t *dev_depths_i32, int quiescence, int64_t node_budget,
                               void *dev_planes_s2, uint64_t *dev_nodes_u64, uint32_t *dev_cuts_u32,
                               uint64_t *dev_depth_sum_u64);
/* The two _id calls with an opt-in move ORDERING (csrc/opponent.hpp states the rule) for the budgeted search that
 * stands for the reference's Limit(time=...) (stockfish.py:14-21).  ordering = 0 launches the kernels of the _id call
 * and nothing else.  ordering = 1: below the root the moves are searched by victim (Q R B N P, promotions), then the two
 * killer moves of the ply, then the other quiet moves; a quiet move that cuts a node below the root becomes the
 * first killer of its ply, for this slot and this search only.  With a budget that no slot reaches, moves, scores,
 * flags and depths_done are those of ordering = 0 and only the node counts differ; under a budget that cuts, all may
 * differ.  The answer stays a function of the board and the arguments alone.
 * CRL_ERR_ARG: an ordering other than 0 or 1, and what the _id calls refuse.  No state changes on an error. */
int  crl_opponent_moves_ord(crl_ctx *ctx, const int32_t *depths /*G*/, int quiescence, int push, int64_t node_budget,
                            int ordering, uint16_t *moves /*G*/, int32_t *scores /*G*/, int64_t *nodes /*G*/,
                            uint8_t *flags /*G*/, int32_t *depths_done /*G*/);   /* stockfish.py:14-21 */
int  crl_sim_reply_opponent_ord(crl_ctx *ctx, const int32_t *dev_depths_i32, int quiescence, int64_t node_budget,
                                int ordering, void *dev_planes_s2, uint64_t *dev_nodes_u64, uint32_t *dev_cuts_u32,
                                uint64_t *dev_depth_sum_u64);                     /* stockfish.py:14-21 */
/* The two _ord calls with an opt-in REPETITION rule (csrc/opponent.hpp states it).  repetition = 0 is the _ord call,
 * array for array, from the same kernels.  repetition = 1: a node below the root whose position -- the same
 * _transposition_key, the same side to move -- occurred before, on the search path or among the reversible plies
 * that led to the root (the game's history ring; for the reply call the tree path of the pending node and then the
 * ring), is worth 0 and is searched no further.  One earlier occurrence is enough and the decision is exact; the root
 * is never tested, a result takes precedence, and the game itself still ends on the fifth occurrence.  The answer is
 * a function of the root, its reversible history and the arguments.
 * CRL_ERR_ARG: a repetition other than 0 or 1, and what the _ord calls refuse.  No state changes on an error. */
int  crl_opponent_moves_rep(crl_ctx *ctx, const int32_t *depths /*G*/, int quiescence, int push, int64_t node_budget,
                            int ordering, int repetition, uint16_t *moves /*G*/, int32_t *scores /*G*/,
                            int64_t *nodes /*G*/, uint8_t *flags /*G*/, int32_t *depths_done /*G*/);
int  crl_sim_reply_opponent_rep(crl_ctx *ctx, const int32_t *dev_depths_i32, int quiescence, int64_t node_budget,
                                int ordering, int repetition, void *dev_planes_s2, uint64_t *dev_nodes_u64,
                                uint32_t *dev_cuts_u32, uint64_t *dev_depth_sum_u64);
/* The two _rep calls with an opt-in positional EVALUATION (csrc/opponent.hpp states it, term by term, with its
 * bound).  evaluation = CRL_OPP_EVAL_MATERIAL is the _rep call, array for array, from the same kernels.
 * evaluation = CRL_OPP_EVAL_POSITIONAL: the static evaluation of the search -- at the horizon and as the stand-pat of
 * a quiescence node -- is the tapered sum of material, advancement, passed / doubled / isolated pawns, mobility, open
 * files, the seventh rank, the bishop pair, king shelter and king attack, plus a tempo; nothing else of the search
 * changes.  Conventional untuned weights, no Elo claim.  |score| <= 14528 unless it is a mate score.
 * CRL_ERR_ARG: an evaluation outside {0, 1}, and what the _rep calls refuse.  No state changes on an error. */
#define CRL_OPP_EVAL_MATERIAL 0
#define CRL_OPP_EVAL_POSITIONAL 1
int  crl_opponent_moves_ev(crl_ctx *ctx, const int32_t *depths /*G*/, int quiescence, int push, int64_t node_budget,
                           int ordering, int repetition, int evaluation, uint16_t *moves /*G*/, int32_t *scores /*G*/,
                           int64_t *nodes /*G*/, uint8_t *flags /*G*/, int32_t *depths_done /*G*/);
int  crl_sim_reply_opponent_ev(crl_ctx *ctx, const int32_t *dev_depths_i32, int quiescence, int64_t node_budget,
                               int ordering, int repetition, int evaluation, void *dev_planes_s2,
                               uint64_t *dev_nodes_u64, uint32_t *dev_cuts_u32, uint64_t *dev_depth_sum_u64);
/* The two _ev calls with opt-in SELECTIVE search (csrc/opponent.hpp states it): null-move pruning and late-move
 * reductions on top of ORDERING.  selective = 0 is the _ev call, array for array, from the same kernels.
 * selective = 1 needs ordering = 1 and launches the SEL instantiation of k_opponent_moves_id / k_reply_opponent_id of the
 * same shape (quiescence, repetition, evaluation): a node with remaining depth >= 2 whose static evaluation reaches beta
 * first tries a null move searched 3 plies shallower, and a quiet late move (position >= 3, remaining depth >= 3) is
 * first searched one ply shallower on a null window and again at full depth only if it beats alpha.  The search is
 * no longer minimax over the full tree; with a maximum depth <= 2 every output equals the _ev call's.
 * CRL_ERR_ARG: a selective other than 0 or 1, selective = 1 with ordering = 0, and what the _ev calls refuse.  No
 * state changes on an error. */
int  crl_opponent_moves_sel(crl_ctx *ctx, const int32_t *depths /*G*/, int quiescence, int push, int64_t node_budget,
                            int ordering, int repetition, int evaluation, int selective, uint16_t *moves /*G*/,
                            int32_t *scores /*G*/, int64_t *nodes /*G*/, uint8_t *flags /*G*/,
                            int32_t *depths_done /*G*/);
int  crl_sim_reply_opponent_sel(crl_ctx *ctx, const int32_t *dev_depths_i32, int quiescence, int64_t node_budget,
                                int ordering, int repetition, int evaluation, int selective, void *dev_planes_s2,
                                uint64_t *dev_nodes_u64, uint32_t *dev_cuts_u32, uint64_t *dev_depth_sum_u64);
/* The two _sel calls with opt-in EXCHANGE (csrc/opponent.hpp states it): delta and exchange pruning at the quiescence
 * nodes that stand pat.  exchange = 0 is the _sel call, array for array, from the same kernels.  exchange = 1 needs
 * ordering = 1 and quiescence >= 1 and launches the EXC instantiation of k_opponent_moves_id / k_reply_opponent_id of the
 * same shape (repetition, evaluation, selective): at such a node a tactical move that is no promotion is dropped when
 * stand + value(victim) + 200 <= alpha, and any tactical move when its static exchange value on the destination
 * square is negative.  The filter generates no moves: node counts count what they counted.  From a root whose search
 * meets no such move every output equals the _sel call's.
 * CRL_ERR_ARG: an exchange other than 0 or 1, exchange = 1 with ordering = 0 or quiescence = 0, and what the _sel calls
 * refuse.  No state changes on an error. */
int  crl_opponent_moves_exc(crl_ctx *ctx, const int32_t *depths /*G*/, int quiescence, int push, int64_t node_budget,
                            int ordering, int repetition, int evaluation, int selective, int exchange,
                            uint16_t *moves /*G*/, int32_t *scores /*G*/, int64_t *nodes /*G*/, uint8_t *flags /*G*/,
                            int32_t *depths_done /*G*/);
int  crl_sim_reply_opponent_exc(crl_ctx *ctx, const int32_t *dev_depths_i32, int quiescence, int64_t node_budget,
                                int ordering, int repetition, int evaluation, int selective, int exchange,
                                void *dev_planes_s2, uint64_t *dev_nodes_u64, uint32_t *dev_cuts_u32,
                                uint64_t *dev_depth_sum_u64);
/* The exchange test alone, without a search, for every legal move of every window slot's current position, whatever
 * the game's result: bits[g * CRL_MAX_MOVES + i] for move i of crl_legal_moves' order (host uint8, synchronous,
 * window-relative) has bit 0 set if the move is tactical and bit 1 if the test keeps it (static exchange value >= 0;
 * always set for a move that is not tactical); bytes from counts[g] on are 0.  counts[g]: the slot's legal
 * moves.  No state change.  CRL_ERR_ARG: a NULL array. */
int  crl_opponent_exchange(crl_ctx *ctx, uint8_t *bits /*G*CRL_MAX_MOVES*/, int32_t *counts /*G*/);
/* The static evaluation of every window slot's current position, from the side to move, whatever the game's result:
 * scores[g] (host int32, synchronous, window-relative).  evaluation as above: 0 is STATIC EVALUATION of
 * csrc/opponent.hpp, 1 its EVALUATION.  No search, no state change.
 * CRL_ERR_ARG: NULL scores, an evaluation outside {0, 1}. */
int  crl_opponent_evaluate(crl_ctx *ctx, int evaluation, int32_t *scores /*G*/);

/* ---- threads > 1: virtual-loss waves of simulations per game (csrc/search_wave.hpp) --------------------------
 * The reference runs `threads` explore_tree workers on one tree, kept apart by a virtual loss (mctree.py:12,173-176,
 * 226-227,289-293).  The wave schedule is the deterministic one among its legal schedules: per game, up to `threads`
 * workers select one after the other on frozen statistics, all simulate, all back up in thread order; a worker whose
 * descent would step onto a node created in the same wave stays idle (the wave ends short).  Evaluator rows are
 * game-major: leaf t of window slot r is row r * threads + t, so every evaluator buffer has slots * threads rows.
 * CRL_POLICY_FULL only (CRL_ERR_STATE otherwise).  The step is
 *     crl_wave_select -> policy(S1 rows) -> crl_wave_reply -> policy/value(S2 rows)
 * and enqueues only (it captures into a hipGraph); a game whose budget is spent idles.
 * crl_wave_config: 1 <= threads <= CRL_WAVE_MAX_THREADS; allocates the wave arrays (about 6 bytes x threads x
 * max_games x (max_sims + 1)); synchronises and reads the pending state from the device: CRL_ERR_STATE while a
 * simulation or a wave is pending (also one enqueued by a replayed hipGraph).  crl_wave_begin / crl_wave_select on a
 * slot with a pending one-leaf simulation raise the sticky device error (CRL_ERR_STATE at the next synchronising call).
 * crl_wave_begin: after crl_search_begin + crl_search_root_priors; every live slot gets a budget of n_sims
 * (1 <= n_sims <= max_sims) simulations and the wave statistics restart.
 * crl_wave_backup: the backprop of the last wave (the counterpart of crl_sim_backup).
 * crl_wave_remaining (synchronises): the largest budget not yet selected over the window; 0 = only crl_wave_backup
 * is left.  crl_wave_stats (synchronises): per window slot, since crl_wave_begin: waves, short waves, leaves. */
#define CRL_WAVE_MAX_THREADS 64
int  crl_wave_config(crl_ctx *ctx, int threads);
int  crl_wave_begin(crl_ctx *ctx, int n_sims);
int  crl_wave_select(crl_ctx *ctx, const void *dev_policy_s2_f32, const void *dev_value_s2_f32, void *dev_planes_s1);
int  crl_wave_reply(crl_ctx *ctx, const void *dev_policy_s1_f32, void *dev_planes_s2);
int  crl_wave_backup(crl_ctx *ctx, const void *dev_policy_s2_f32, const void *dev_value_s2_f32);
int  crl_wave_remaining(crl_ctx *ctx, int32_t *max_remaining);
int  crl_wave_stats(crl_ctx *ctx, int32_t *waves /*G*/, int32_t *short_waves /*G*/, int32_t *leaves /*G*/);

/* ---- tower seam (model.py) -------------------------------------------------------------- */
/* Residual trunk of ChessModel (model.py:33-37,111-122: stem conv + n_blocks residual blocks,
 * BatchNorm folded) for `filters` in {64, 128, 256} (BASELINE configs C2, C3/C4, C5; 256 is the
 * reference's own width, model.py:33) as ONE fused MFMA kernel, plus the three 1x1 head
 * convolutions with their BN + ReLU (model.py:40-42,51-55).  fp16 NHWC planes
 * [n_boards][8][8][128] in.  dev_wtiles_f16 holds the folded fp16 kernels as 64-byte-row planes in
 * consumption order [conv][tap = ky*3+kx][in-ch/32][filters rows][4 chunks][8 in] -- byte for byte the
 * image the kernel keeps in LDS, so that its weight DMA copies contiguous blocks: row r of a
 * plane holds output channel (r & ~31) + 8*((r & 15) >> 2) + 4*((r >> 4) & 1) + (r & 3), and the
 * 16-byte chunk with input channels 8c .. 8c+7 of that row sits at position c ^ ((-(r >> 2)) & 3)
 * (chessrl_amd/packing.py:pack_trunk is the reference packer); the stem has 128 input channels, every
 * other conv `filters`; dev_bias_f32 is [1+2*n_blocks][filters].
 * Outputs (either may be NULL): dev_out_f32 = fp32 trunk activations [n_boards][8][8][filters];
 * dev_head_out_f32 = [n_boards][192] floats after ReLU: [0,128) the policy head in Keras Flatten
 * order (position*2 + channel), [128,192) the value head; from dev_head_w_f32 [3][filters] and
 * dev_head_b_f32 [3].  n_boards % 4 == 0.
 * Stateless: needs no crl_ctx. */
int  crl_trunk_forward(void *hip_stream, int filters, const void *dev_planes_f16,
                       const void *dev_wtiles_f16, const void *dev_bias_f32, void *dev_out_f32,
                       int n_boards, int n_blocks, const void *dev_head_w_f32,
                       const void *dev_head_b_f32, void *dev_head_out_f32);

/* The general form.  flags: CRL_TRUNK_BITPLANES = dev_planes holds plane bitboards (as
 * crl_trunk_forward_bitplanes); CRL_TRUNK_SPLIT = precision mode "f16x3": every operand is carried
 * as two fp16 numbers (hi + lo) and every product is three MFMAs (hi.Whi + hi.Wlo + lo.Whi, fp32
 * accumulation), which puts the outputs within ~1e-5 of an fp32 evaluation of the same weights
 * whatever the weights are (one fp16 MFMA per product is within 1e-3 of fp32 for Keras-initialised
 * and lightly trained towers but not for sharp ones; model.py:31-63 runs fp32).  The weight image
 * then lists, per conv and spatial tap, the planes of Whi and then the planes of Wlo = fp16(W - Whi),
 * each in the plane order above (twice the size of the plain image; a Whi plane serves hi.Whi and
 * lo.Whi while it sits in LDS).
 * CRL_TRUNK_BALANCE = where the kernel of this filter count, batch and precision tiles the board by ranks (128 filters,
 * four boards per workgroup, one MFMA per product), its partner-balance instantiation runs (csrc/tower_x16.hpp, ALT = 1:
 * the wave of each SIMD that reaches a tap's sync first requests the weight tiles for both); everywhere else the flag
 * changes nothing.  Same outputs bit for bit; crl_trunk_kernel_name reports which kernel a flag combination gets. */
#define CRL_TRUNK_BITPLANES 1
#define CRL_TRUNK_SPLIT 2
#define CRL_TRUNK_BALANCE 4
int  crl_trunk_forward_x(void *hip_stream, int filters, int flags, const void *dev_planes,
                         const void *dev_wtiles_f16, const void *dev_bias_f32, void *dev_out_f32,
                         int n_boards, int n_blocks, const void *dev_head_w_f32,
                         const void *dev_head_b_f32, void *dev_head_out_f32, void *dev_workspace,
                         size_t workspace_bytes);

/* 256 filters with CRL_TRUNK_SPLIT run LAYER-WISE (csrc/tower_layer.hpp: one launch per convolution, a workgroup owns 4
 * boards x all 256 output channels and streams activations and weights; the fused kernel could keep ONE such board resident
 * and streamed the whole weight set for it).  The caller lends the activation images: crl_trunk_workspace_bytes() bytes of
 * device memory (two images of 256 KiB per 4 boards; 0 for every other (filters, flags): dev_workspace may then be NULL),
 * contents undefined before and after a call; workspace_bytes says how much the caller really lent and a call whose batch
 * needs more fails with CRL_ERR_ARG instead of overrunning it (ignored where no workspace is wanted).  n_blocks >= 1 and
 * dev_head_out_f32 are required there (a trunk-only call has no consumer in the product; the other filter counts, whose
 * fused kernels write the fp32 trunk on the way, accept both).  The weight image of
 * that path lists, per convolution, the planes K-CHUNK-major: [conv][in-ch/32][tap][Whi, Wlo][256 rows][4 chunks][8 in]
 * (rows / chunks as above; the stem has 4 chunks of input planes, every other convolution 8). */
size_t crl_trunk_workspace_bytes(int filters, int n_boards, int flags);

/* Hybrid precision (ChessModel(precision="hybrid")).  An evaluation of S1 only chooses the opponent's reply
 * -- argmax of the policy over the legal labels (agentdistributed.py:57-58 -> mctree.py:244-250) -- so S1 runs
 * the single-MFMA trunk first and only the boards whose choice is not safe against that arithmetic's error are
 * evaluated again with CRL_TRUNK_SPLIT; S2 (priors and value: the 1e-3 outputs) always runs CRL_TRUNK_SPLIT.
 * crl_reply_margin lists the unsafe boards from the legal priors (or logits) of the first pass: board b is
 * listed when it has at least two legal moves and log p1 - log p2 of its two best ones (the difference of
 * their logits) is below *dev_log_margin_f32 -- one float in DEVICE memory (not by value: the margin belongs to
 * the weight set, and weights are rewritten in place under captured hipGraphs; a NaN there lists every board).
 * dev_list: int32 [CRL_LIST_HEADER + n_boards]: [0] boards listed by this call, [1] unused, [2..3] one uint64
 * running total over all calls on this buffer (statistics; zero it once), [CRL_LIST_HEADER + k] the boards
 * (unordered).
 * crl_trunk_forward_indexed evaluates exactly the listed boards (rows of dev_bitplanes_u64 / dev_head_out_f32;
 * other rows of dev_head_out_f32 are left as they are): the CRL_TRUNK_BITPLANES | CRL_TRUNK_SPLIT kernels with a
 * grid for n_boards whose surplus workgroups exit at once -- the list never leaves the device, the launch sequence
 * is fixed and captures into a hipGraph.  dev_workspace: as for crl_trunk_forward_x (crl_trunk_workspace_bytes(filters,
 * n_boards, CRL_TRUNK_BITPLANES | CRL_TRUNK_SPLIT); may be the buffer of the full-batch launches).  Stateless. */
#define CRL_LIST_HEADER 4
int  crl_reply_margin(void *hip_stream, const void *dev_priors_f32, const int32_t *dev_counts, int n_boards,
                      const float *dev_log_margin_f32, int rows_are_logits, int32_t *dev_list);
int  crl_trunk_forward_indexed(void *hip_stream, int filters, const void *dev_bitplanes_u64,
                               const void *dev_wtiles_f16x3, const void *dev_bias_f32, int n_boards, int n_blocks,
                               const void *dev_head_w_f32, const void *dev_head_b_f32, void *dev_head_out_f32,
                               const int32_t *dev_list, void *dev_workspace, size_t workspace_bytes);

/* crl_trunk_forward with the input given as plane bitboards (CRL_PLANES_BITS), uint64
 * [n_boards][128]; everything else as above. */
int  crl_trunk_forward_bitplanes(void *hip_stream, int filters, const void *dev_bitplanes_u64,
                                 const void *dev_wtiles_f16, const void *dev_bias_f32, void *dev_out_f32,
                                 int n_boards, int n_blocks, const void *dev_head_w_f32,
                                 const void *dev_head_b_f32, void *dev_head_out_f32);

/* The dense layers behind the head convolutions (model.py:44-48: Dense(1968, softmax); model.py:56-61:
 * Dense(256, relu) -> Dense(1, tanh)) on the [n_boards][192] head activations crl_trunk_forward
 * leaves: one launch per head, fp32-accurate through fp16 MFMAs on (hi, lo)-split operands.
 * dev_policy_wp_f16: the policy kernel W[128 in][1968 out] packed in fragment order
 * [label tile 128][k-step 4][hi|lo][lane 64][8 halves], lane 16 q + r holding
 * W[32 s + 8 q + e][16 tile + r] (labels >= 1968 zero): 1 MiB; dev_policy_bias_f32: [2048], entries
 * >= 1968 set to -1e30.  dev_value_w1p_f16: W1[64 in][256 out] packed the same way
 * [tile 16][k-step 2][hi|lo][lane][8]: 64 KiB; b1 [256]; dev_value_w2b2_f32 [257] = w2 then b2 (in
 * memory, not by value: weights may be rewritten in place under a captured hipGraph).
 * dev_policy_out_f32: [n_boards][1968] probabilities; dev_value_out_f32: [n_boards] or NULL (the
 * value head is skipped: evaluations of S1 only choose the reply).  Stateless (dev_scratch_f32: below). */
int  crl_heads_forward(void *hip_stream, const void *dev_head_act_f32, int n_boards,
                       const void *dev_policy_wp_f16, const void *dev_policy_bias_f32,
                       const void *dev_value_w1p_f16, const void *dev_value_b1_f32,
                       const void *dev_value_w2b2_f32, void *dev_policy_out_f32, void *dev_value_out_f32,
                       void *dev_scratch_f32);

/* crl_heads_forward writing only what the search reads: dev_priors_out_f32 [n_boards][CRL_MAX_MOVES],
 * entry j of row b = softmax(...)[dev_labels[b][j]] for j < dev_counts[b] (the rest of the row is left
 * untouched) -- 4 x count bytes per board instead of 7 872, bit-identical values.  dev_labels uint16
 * [n_boards][CRL_MAX_MOVES], dev_counts int32 [n_boards] (crl_eval_labels).  Stateless. */
int  crl_heads_forward_legal(void *hip_stream, const void *dev_head_act_f32, int n_boards,
                             const void *dev_policy_wp_f16, const void *dev_policy_bias_f32,
                             const void *dev_value_w1p_f16, const void *dev_value_b1_f32,
                             const void *dev_value_w2b2_f32, const uint16_t *dev_labels,
                             const int32_t *dev_counts, void *dev_priors_out_f32, void *dev_value_out_f32,
                             void *dev_scratch_f32);

/* crl_heads_forward_legal without its normalising pass, for batches the sliced form serves
 * (crl_heads_raw_supported(n_boards) == 1; CRL_ERR_ARG otherwise): dev_logits_out_f32 rows receive the
 * LOGITS of the legal moves and dev_stats_out_f32 (float [n_boards][16], required) the slice statistics;
 * the search kernels normalise on read (CRL_POLICY_LEGAL_RAW, crl_set_policy_stats) -- one launch per
 * tower call instead of two, identical priors. */
int  crl_heads_forward_legal_raw(void *hip_stream, const void *dev_head_act_f32, int n_boards,
                                 const void *dev_policy_wp_f16, const void *dev_policy_bias_f32,
                                 const void *dev_value_w1p_f16, const void *dev_value_b1_f32,
                                 const void *dev_value_w2b2_f32, const uint16_t *dev_labels,
                                 const int32_t *dev_counts, void *dev_logits_out_f32, void *dev_value_out_f32,
                                 void *dev_stats_out_f32);
int  crl_heads_raw_supported(int n_boards);

/* dev_scratch_f32 of the two calls above: float [n_boards][16] or NULL.  With it, batches of at most
 * crl_heads_set_sliced_max boards (default 2048: measured 16 vs 17 us there, 9 vs 17 us at 512) run as label slices x board blocks (8 slices of 256
 * labels, the value head as a ninth "slice": 9 x n_boards/16 workgroups instead of n_boards/16)
 * followed by a normalising pass that reads the slice statistics left in the scratch -- a batch of
 * 512 boards otherwise pulls the whole 1-MiB policy kernel through each of 32 CUs.  Same results for
 * the two calls (bit for bit); the last bits differ from the one-pass form (summation order).  Larger batches run ONE launch: the
 * policy head's workgroups and, behind them, the value head's.
 * PROCESS-GLOBAL tuning state (like crl_trunk_set_small_batch below): it applies to every context and
 * stream of the process; meant to be set once at start-up, not per context. */
int  crl_heads_set_sliced_max(int boards);

/* Batches of at most 512 boards (256 at 256 filters) give at most half of the 256 CUs a
 * workgroup; they run the same kernels with half the boards per workgroup and twice the
 * workgroups (identical trunk bits).  enabled = 0 turns that off process-wide (default 1). */
int  crl_trunk_set_small_batch(int enabled);

/* Which kernel crl_trunk_forward_x launches for this filter count, batch and flags, written as
 * rocprofv3 prints it without namespace and argument list ("k_trunk_x16<128, 4, 1, 0, 1, 0, 0, 0>"):
 * measurement tools look their profiles up by it instead of restating the dispatch rule.  No
 * reference counterpart (model.py:31-63 builds one Keras graph). */
int  crl_trunk_kernel_name(int filters, int n_boards, int flags, char *buf, int buf_len);

/* ---- measurement -------------------------------------------------------------------------------
 * crl_stamp enqueues a one-thread kernel that appends (id, wall clock of the device) to a ring in device memory:
 * dev_ring is uint64 [2 + 2 * capacity], [0] = stamps written so far (zero it once), [1] unused, then pairs
 * (id, clock) at entry (count % capacity).  It captures into a hipGraph like any kernel, so bench.py gets the time of
 * every phase of a step and of every trunk launch from the REPLAYED graph (consecutive stamps telescope to the step)
 * instead of from eager launches beside it.  crl_stamp_clock_khz: the rate of that clock
 * (hipDeviceAttributeWallClockRate; 100 000 on MI355X), or a negative crl_status.  No reference counterpart. */
int  crl_stamp(void *hip_stream, uint64_t *dev_ring, uint32_t capacity, uint32_t id);
int  crl_stamp_clock_khz(int device);

/* ---- training step (model.py:83-99 fit_generator) --------------------
 * The reference's Conv2D layers (model.py:33-34,113-118) train through TensorFlow; here a 3x3 'same'
 * convolution on the 8x8 board is the GEMM [B*64, 9*C] x [9*C, Cout] over NHWC activations, and these
 * two kernels build its patch matrix and the adjoint (gradient w.r.t. the activations).  fp32, NHWC
 * x [n_boards][8][8][C], cols [n_boards*64][9][C] with tap = ky*3+kx; C % 4 == 0.  Stateless. */
int  crl_im2col3x3_f32(void *hip_stream, const void *dev_x_f32, void *dev_cols_f32, int n_boards,
                       int channels);
int  crl_col2im3x3_f32(void *hip_stream, const void *dev_gcols_f32, void *dev_gx_f32, int n_boards,
                       int channels);

#ifdef __cplusplus
}
#endif
#endif /* CHESSRL_HIP_H */
