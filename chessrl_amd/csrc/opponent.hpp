// opponent.hpp -- the built-in opponent: a fixed-depth alpha-beta player on the device.  It stands where the
// reference puts its engine (stockfish.py:23-31 Stockfish.best_move, gamestockfish.py:27-41 the reply inside
// GameStockfish.move); it is NOT that engine and claims no Elo: results read "against the built-in depth-d opponent".
//
// One wavefront (one workgroup) searches one window slot (lane = square, as everywhere in search.hpp); the root is
// d.cur[g].  Integer work only.  This comment is the specification; tests/opponent_util.py restates it.
//
// SEARCH.  Negamax with alpha-beta, depth d = depths[slot] plies, fail-soft (a node returns its best score):
//     the root window is (-INF, +INF), INF = 32000;
//     a child is searched with (-beta, -alpha) and scores the negation of what it returns;
//     a move replaces the best only on a STRICTLY greater score; alpha = max(alpha, score);
//     the remaining moves of a node are cut when alpha >= beta.
// The returned move is therefore the FIRST root move, in the root's order, that attains the minimax value, and the
// returned score is that value: plain minimax with a first-maximum rule gives the same pair.
//
// NODE VALUE, in this order, for the node at search ply k (root = 0):
//     1. generate the legal moves.  This is ONE NODE: the node counter counts wave_movegen calls, the root's included;
//     2. r = position_result(b, n, in_check, 1): no legal move (mate or stalemate), insufficient material, the
//        fifty-move claim at clock >= 100, the 75-move rule.  The repetition count handed in is 1: repetition is NOT
//        looked at below the root (nor at it: a slot whose game has a result, fivefold included, is skipped before);
//     3. r = mate (the side to move is mated): the value is -(30000 - k).  Any other result (a draw): 0;
//     4. no result and k = d (no depth remains): the static evaluation;
//     5. otherwise the search of the moves.
// Horizon nodes are generated too, so depth d sees a mate delivered by ply d.
//
// QUIESCENCE.  Q = quiescence plies of the call, 0 .. CRL_OPP_MAX_QUIESCENCE (6), the same for every slot.  Q = 0 is
// the search above and nothing else.  For Q > 0 the node at ply k >= d is a quiescence node, j = k - d; nodes at k < d
// are unchanged.  Steps 1-3 hold for it as they stand (its moves are generated: one node, counted and tested against
// the node limit like any other; a result is -(30000 - k) or 0).  Without a result:
//     4a. j = Q (no quiescence ply remains): the static evaluation, in check or not;
//     4b. the side to move is in check: ALL legal moves are searched in the below-root order; no stand-pat, best
//         starts at -INF;
//     4c. otherwise stand = the static evaluation and best = stand.  If stand >= beta the node returns stand and
//         searches nothing; otherwise alpha = max(alpha, stand) and only the TACTICAL moves (the predicate below) are
//         searched, in a stable partition by victim: queen, rook, bishop, knight, pawn (en passant counts as pawn),
//         then the promotions that capture nothing; generation order inside a class; a capturing promotion sorts by
//         its victim.  Without a tactical move the value is stand.
// Children, the strictly-greater rule, alpha and the cut are those of SEARCH.  The root (k = 0 < d) is never a
// quiescence node, so the root rule holds.  The evaluation is bounded by material, so a score that is not a mate stays
// inside (-30000 + k, 30000 - k).  Not done: checks other than the evasions of 4b; delta and exchange pruning only on
// request (EXCHANGE below).
// (tests/quiescence_util.py restates this section.)
//
// ORDER OF THE MOVES.  At the root: python-chess generation order, as wave_movegen emits it.  Below the root: a stable
// partition, tactical moves first, generation order inside each class.  A move is tactical if
//     its destination holds an enemy piece, or
//     it is an en-passant capture (a pawn that changes file onto an empty square), or
//     it is a promotion.
// (The partition is two ballots per 64 moves and prefix popcounts, like the suffix scan of movegen.hpp.)
//
// STATIC EVALUATION, int32, from the side to move: one term per lane, one wave reduction.
//     material           P 100, N 320, B 330, R 500, Q 900, K 0
//     ring(sq)           min(file, 7 - file, rank, 7 - rank) = 0 .. 3
//     position bonus     N 10 * ring, B 5 * ring, R 0, Q 2 * ring, K -10 * ring,
//                        P 5 * ring + 6 * (ranks advanced from its start rank: rank - 1 for white, 6 - rank for black)
//     score              (sum over white pieces) - (sum over black pieces), negated when black is to move
//
// STRUCTURE.  No device recursion: an explicit stack of per-ply frames in LDS.  A frame holds the node's board, its
// 256-entry u16 move list, the cursor, the count, alpha, beta and the best score: 608 B, d + 1 <= 6 of them = 3.6 KiB
// (game_push's scratch shares the bytes: the frames are dead when the move is pushed).  The main loop is
// `while (nodes < limit)` and every turn generates exactly one node; the unwinding inside a turn strictly
// decreases the ply.  So the loop is bounded by the node limit by construction: a logic error ends as a flagged cut.
// With Q > 0 a node that searches moves lies at ply <= d + Q - 1: 5 + 6 = 11 frames, 6.5 KiB, in kernels of their own
// (k_opponent_moves_q, k_reply_opponent_q; one search body, a template parameter apart), so a Q = 0 launch runs the
// code and keeps the LDS it had.  A quiescence node that stands pat at or above beta, or lies at j = Q, is generated
// without a list and takes no frame; whether it is in check is read from the board before its moves are generated.
//
// NODE LIMIT, per slot.  The limit is tested before every node.  When the count has reached it and the search is not
// finished, the search ends: the slot returns the best root move among those COMPLETELY searched (and its score), or
// the first legal move (and the score -INF) if none was, with the flag CRL_OPP_CUT.  A search that finishes with its
// last permitted node is not cut.  Node counts are deterministic, so the cut is.
//
// PER SLOT.  depths[slot] = 0 leaves the slot alone (NO_MOVE, score 0, 0 nodes, flag 0); 1 .. CRL_OPP_MAX_DEPTH
// searches it.  A slot whose game already has a result returns NO_MOVE, score 0, 0 nodes and CRL_OPP_SKIPPED.  With
// `push`, the chosen move is pushed through game_push: history, record, ply and result change exactly as by
// crl_push_moves, repetition included.
//
// ITERATIVE DEEPENING (the _id kernel templates only; every other launch is the text above and nothing else).  Per slot:
// D = depths[slot], now the MAXIMUM depth, 1 .. CRL_OPP_MAX_DEPTH; B >= 1, the node budget of the call; Q as above.
//     One node counter runs across all iterations of the slot.  It counts wave_movegen calls as above; the root is
//     generated again at the start of every iteration and counted each time.  The counter is tested before every node:
//     when it has reached B and the search is not finished, the search stops.
//     Iteration i = 1 .. D is SEARCH (and QUIESCENCE) to depth i with ONE difference: at the root the best move of
//     iteration i - 1 is moved to the front of the list, the other root moves keeping generation order (a stable
//     move-to-front; iteration 1 uses generation order).  Below the root nothing changes: the tactical-first
//     partition, the victim partition, the strictly-greater rule, fail-soft, the windows.
//     An iteration that finishes sets (move, score) to its result and depth_done = i.  Iteration D finishing ends the
//     search; a search that finishes with its last permitted node is not cut.
//     If the budget stops iteration i: with at least one root move of iteration i searched completely, (move, score)
//     is the best completely searched root move of iteration i and its score -- the first such move is the previous
//     iteration's best, so the partial answer is never worse at depth i than the move already held; otherwise (move,
//     score) of iteration i - 1 stands, and in iteration 1 that is the first legal move with the score -INF, as under
//     NODE LIMIT.  depth_done stays i - 1.
//     CRL_OPP_CUT means depth_done < D.  depths[slot] = 0, finished games (CRL_OPP_SKIPPED; depth_done 0) and `push`
//     are unchanged.
// The answer is still a function of the board and the settings alone.  Structure: the same frames (an iteration to depth
// i uses i + 1 of them, or i + Q) and the same main loop, `while (nodes < B)` with one wave_movegen per turn; starting
// iteration i + 1 is a change of state inside the turn that finished iteration i (ply 0, the full window, the remembered
// best move), not a loop of its own, so a logic error still ends as a flagged cut.  The move-to-front is one ballot per
// 64 moves and a shift by one lane.  (tests/iterdeep_util.py restates this section.)
//
// ORDERING (the ORD shapes of the _id kernels only; it requires ITERATIVE DEEPENING, and everything in that section holds, the root's
// order included: generation order with the previous iteration's best moved to the front).
//     Move order below the root.  At every node at ply k >= 1 that searches moves the order is a stable partition into
//     NINE classes, generation order inside each class:
//         0 .. 5   the victim classes of QUIESCENCE 4c: victim Q, R, B, N, P (en passant counts as P), then the
//                  promotions that capture nothing;
//         6        killer A of ply k;      7   killer B of ply k;      8   every other quiet move.
//     A tactical move is classed by its victim whatever the killers are.  A node that stands pat (4c) searches the
//     classes 0 .. 5 only, exactly as without ORDERING; a quiescence node in check (4b) and every node at k < D search
//     all nine.
//     Killers.  Each ply 1 .. D + Q - 1 has ONE pair of 16-bit moves (A, B).  Both are NO_MOVE when the slot's search
//     starts; they are kept across the iterations of that search and never shared between slots or between two
//     searches.  A killer that is not in the node's list has no effect.
//     Setting a killer.  When a node at ply k >= 1 has searched its move m and then alpha >= beta (the cut of SEARCH,
//     whether or not a move remained), and m is not tactical in that node's position, and m != A: B = A, then A = m.
//     A node that stands pat searches tactical moves only, so it never sets a killer; the root never sets one.
//     Nothing else changes: fail-soft, the strictly-greater rule, the windows, one wave_movegen per turn, the budget
//     tested before every node, the cut rules, depth_done and CRL_OPP_CUT.
// Consequence.  With a budget nothing reaches, move, score, flag and depth_done are those of the search without ORD (each
// iteration returns the minimax pair of its root order, and the root order does not depend on what lies below it); only
// `nodes` differs.  Under a budget that cuts, all five may differ.  Both searches stay a function of the board and the
// settings alone.  Structure: the killers of ply k and the number of tactical moves of the node live in the pad words
// of frame k (frames exist exactly for the plies that search moves, and a frame is written field by field, never as a
// whole), so the LDS is what it was; a cursor at or past the stored number is a quiet move, so the turn that hands a
// value up needs no board to decide whether a cut sets a killer, and lane 0 stores the pair with the frame's own
// cursor, best and alpha.  The partition is the seven ballots of 4c per 64 moves and two more that find the killers: a
// killer class holds at most one move.  (tests/ordering_util.py restates this section.)
//
// REPETITION (the REP shapes of the _id kernels only; it requires ITERATIVE DEEPENING, so a node budget, and everything in
// ITERATIVE DEEPENING, QUIESCENCE and ORDERING holds; it combines freely with quiescence and with ordering).
//     One step is added to NODE VALUE for the node at search ply k >= 1, after steps 1-3 (the moves are generated
//     first: one node, counted and tested against the budget like any other; a result -- mate, stalemate,
//     insufficient material, the fifty-move claim, the 75-move rule -- takes precedence with the value it has):
//         3b. no result, and the position of this node has occurred before: the value is 0.
//     Such a node searches no move, takes no stand-pat, no evaluation and no frame, and sets no killer.  3b comes
//     before 4 / 4a / 4b / 4c: a quiescence node that would have stood pat at or above beta is a draw first.
//     Occurred before: an earlier position with the same side to move has the same _transposition_key -- piece
//     placement, turn, castling rights, and the en-passant square only where a capture there is legal (bit 20 as
//     wave_movegen derives it).  The earlier position is looked for
//         among the positions of the search path at plies k - 4, k - 6, .. >= 0, the root included, and
//         beyond the root among the positions that led to it: for crl_opponent_moves* the game's history ring; for
//         the reply kernels the tree path of the pending node (S1 / S2 of its ancestors) and then the game's ring,
//         which is what past_ref resolves.
//     Only the node's reversible plies can hold it: distances 4, 6, .. up to its halfmove clock (a running node has
//     clock < 100, so the 256-ply ring always suffices).  ONE earlier occurrence is enough; the game itself still ends
//     on the fifth, as the reference's does.  The root is never tested.  The value is 0 at every ply and for either
//     side: no contempt.  The decision is exact: the 64-bit hash is a filter, same_key on the boards decides, as in
//     count_prior.
// Consequences.  (a) The search is still minimax over its tree; a node's value now also depends on its path, and there
// is no transposition table, so nothing is shared between paths: with a budget nothing reaches, move, score, flag and
// depth_done with ordering on and off are equal, only `nodes` differs.  (b) From a root with halfmove clock 0 and
// D + Q <= 3 no node can be a repetition (the shortest distance is 4 and only reversible plies count): every output,
// `nodes` included, equals the search without REPETITION.  (c) The answer is a function of the root, its reversible
// history and the arguments; for the games form that is still a function of the slot's state alone.
// Structure.  No dependent HBM read per node: once per search the hashes of the root's reversible history, min(root
// clock, 99) positions as far as they exist, are copied into LDS through past_ref (at most 99 x 8 B; the copy survives
// the iterations), and beside them live, per ply that has a frame, the hash of the node's key-normalised board and its
// state word with the derived en-passant bit (the frame's board has it clear: apply_move builds it so).  The node's own
// bit comes from the MoveGenInfo of the movegen it runs anyway.  Per node the lanes compare the node's hash at the
// distances 4, 6, .. in parallel, against the path's plies where the distance stays inside the search and against the
// history copy beyond; a board is read (a frame's from LDS, a history one from the ring or the tree) only on a hash
// hit.  These arrays lie outside the union game_push reuses.  LDS: 3.6 KiB + 864 B = 4 512 B (REP without QS) and
// 6.5 KiB + 928 B = 7 616 B (REP with QS).  (tests/repetition_util.py restates this section.)
//
// EVALUATION (the POS shapes of the _id kernels only: evaluation = "positional", an opt-in on top of ITERATIVE DEEPENING, so of a node
// budget; it combines freely with QUIESCENCE, ORDERING and REPETITION.  Every other launch uses STATIC EVALUATION above
// and nothing else).  It replaces the static evaluation and nothing else: NODE VALUE 1-3 and 3b, the stand-pat (4c
// still reads the evaluation before the moves are generated), the orders, the windows, the budget and the cut stay.
//     Notation.  c is the colour of the piece on square sq and own the pieces of c; rel(sq, c) is the rank for white
//     and 7 - rank for black; ring(sq) as above; occ is all pieces; PA(c') the squares attacked by the pawns of c';
//     ksq(c') the king square of c'; zone(c') = king_attacks(ksq(c')) | bit(ksq(c')) (empty for a side without a
//     king); "ahead" means towards promotion.
//     Per-piece terms.  Two int32 sums, MG and EG, run over all pieces; a white piece adds, a black piece subtracts;
//     a term given once goes to both sums.
//         Pawn    material 100
//                 advancement, adv = rel - 1 (0 .. 5):                      MG 5 * ring + 6 * adv     EG 12 * adv
//                 passed -- no enemy pawn ahead on its own or an adjacent file:
//                                                      MG {0,5,10,20,40,70}[adv]     EG {0,10,20,40,80,140}[adv]
//                 doubled -- a friendly pawn ahead on its file:             MG -10                    EG -20
//                 isolated -- no friendly pawn on an adjacent file, any rank:  MG -10                 EG -15
//         Knight  material 320; position 10 * ring;
//                 mobility, m = popc(knight_attacks & ~own & ~PA(enemy)):   4 * m
//         Bishop  material 330; position 5 * ring;
//                 mobility, m = popc(bishop_attacks(sq, occ) & ~own & ~PA(enemy)):   4 * m
//         Rook    material 500;
//                 mobility, m = popc(rook_attacks(sq, occ) & ~own):         MG 2 * m                  EG 4 * m
//                 its file holds no pawn of either colour:                  MG +20                    EG +10
//                 its file holds no own pawn but an enemy pawn:             MG +10                    EG +5
//                 rel = 6:                                                  MG +10                    EG +20
//         Queen   material 900; position 2 * ring;
//                 mobility, m = popc((rook_attacks | bishop_attacks) & ~own & ~PA(enemy)):   MG m     EG 2 * m
//         King    position                                                  MG -10 * ring             EG +10 * ring
//                 shelter, only when rel(ksq) <= 1: the friendly pawns on the king's file and the adjacent files, on
//                 the next two ranks ahead of the king:                     MG +8 per pawn            EG 0
//         N, B, R, Q   king attack -- the piece's attack set (as computed for its mobility, before the ~own and ~PA
//                 masks) meets zone(enemy):                                 MG N 8, B 8, R 12, Q 20   EG 0
//     Per side.  Bishop pair: a side with two or more bishops gets MG +30 and EG +40, once.
//     Phase.  ph = min(24, N + B + 2 * R + 4 * Q), counted over both colours.
//     Taper.  white = (MG * ph + EG * (24 - ph)) / 24, the division truncating toward zero, so a colour flip (ranks
//     mirrored, colours and the side to move exchanged) negates it exactly.
//     Score.  (white to move ? white : -white) + 10; the 10 is the tempo.
//     Decisions where the table leaves room.  Attack sets stop at the first piece of either colour and include it
//     (x-rays count nothing); a pinned piece moves as if it were free; en-passant and castling rights are not read;
//     PA includes squares a pawn attacks whatever stands there; a rook's "file" terms read pawns of every rank, behind
//     it included; "isolated" and "doubled" are per pawn, so both pawns of an isolated doubled pair are isolated and
//     the rear one is doubled; with several kings of a colour (no legal game has them) zone is the union.
//     Bound.  A piece's terms are at most P 100 + 60 + 140 = 300, N 320 + 30 + 32 + 8 = 390, B 330 + 15 + 52 + 8 = 405,
//     R 500 + 56 + 10 + 20 = 586 (EG; MG 500 + 28 + 20 + 10 + 12 = 570), Q 900 + 6 + 54 = 960 (EG; MG 953), K 48 (MG:
//     six shelter pawns; EG 30), and never below -30 (the king, MG).  A side has a king and at most 15 other pieces,
//     each at most a queen: a side's sum lies in [-30, 15 * 960 + 48 + 40] = [-30, 14488], so |MG|, |EG| <= 14518, the
//     taper lies between them, and |score| <= 14528: well inside (-30000 + k, 30000 - k) for every ply k <= 11, so a
//     score that is not a mate still cannot be taken for one.
//     Structure.  Uniform quantities come from the scalar board: PA of both colours, the fills behind passed and
//     doubled, the eight-bit sets of files that hold a pawn of a colour (isolated, the rook's files), both zones, the
//     phase and the bishop counts.  Lane-local: the one piece of the lane; the diagonal line_attacks are computed
//     under predication for B and Q, the orthogonal ones for R and Q, so a wave pays for each once and not once per
//     piece type; the lane tests its attack set against the masks of both colours and selects the counts, not the
//     masks.  What depends on the lane number alone is kept from being hoisted out of the search loop (an empty asm
//     on the lane number): hoisted, it cost the kernels a wave of occupancy and reserved scratch.  |MG|, |EG| < 2^15 (also for every partial sum: a
//     subset of the pieces obeys the same bound), so MG * 65536 + EG travels through ONE wave reduction as an int32
//     and is taken apart exactly afterwards.  No LDS, no scratch.  (tests/evaluation_util.py restates this section.)
//
// SELECTIVE (the SEL shapes of the _id kernels only: selective = 1, an opt-in on top of ORDERING, so of ITERATIVE DEEPENING and a node
// budget; it combines freely with QUIESCENCE, REPETITION and EVALUATION, and everything in those sections holds unless
// this one says otherwise.  Every other launch searches every line to full width, as above).  Null-move pruning and
// late-move reductions; the three constants (the null move's 3 plies, c >= 3, r >= 3) are fixed.
//     Remaining depth.  A node carries a remaining depth r: the root of iteration i has r = i, a child has r - 1
//     unless a rule below says less.  A node with r <= 0 is a horizon node -- the static evaluation at Q = 0, otherwise
//     a quiescence node whose quiescence ply j counts from the FIRST node on its path with r <= 0 (that node has
//     j = 0, whatever its r; its children j = 1, ..).  This replaces "k = d" of NODE VALUE 4 and "j = k - d" of
//     QUIESCENCE; without this section's rules the definitions coincide.  r falls by at least 1 per ply, so a node
//     that searches moves still lies at ply <= D + Q - 1: the frames, the killers per ply and the REPETITION arrays
//     keep their sizes.
//     Null move.  Tried at a node at ply k >= 1, after NODE VALUE 1-3 and 3b, when ALL of these hold: the node has no
//     result and is no repetition; r >= 2; the side to move is not in check; it owns at least one knight, bishop,
//     rook or queen; the node's own position was not reached by a null move; |beta| < 29000; the static evaluation
//     of the node (the call's evaluation kind) is >= beta.  Then the null child is searched before any move.  Its
//     board is the node's with the side to move exchanged, the en-passant square cleared and the halfmove clock 0, so
//     neither the fifty-move rule nor REPETITION looks across a null move (a fullmove number would change as after a
//     move; the device board keeps none).  It is searched with r_child = r - 3 and the window (-beta, -beta + 1); its
//     move generation is one node, counted and tested against the budget like any other.  If its negated score is
//     s >= beta the node returns s, or beta when s >= 29000; it searches nothing more and sets no killer.  Otherwise
//     the node searches its moves as if nothing had happened.
//     Late-move reduction.  At a node at ply k >= 0, the root included, the move at 0-based position c of the node's
//     order is FIRST searched with r_child = r - 2 and the window (-alpha - 1, -alpha) when ALL of these hold: r >= 3;
//     the node is not in check; c >= 3; the move is not tactical (the predicate of ORDER OF THE MOVES in the node's
//     position; at the root too, whose order stays that of ITERATIVE DEEPENING); it is neither killer A nor B of ply
//     k; the child's position is not in check (read from the child's board before its moves are generated, as
//     quiescence does).  If the negated score of the reduced search is > alpha, the move is searched again with
//     r_child = r - 1 and the window (-beta, -alpha), and that result is the move's score; otherwise the reduced score
//     is.  The strictly-greater rule, fail-soft, the killer rule and the cut then apply to the move's score as before.
//     A root move counts as COMPLETELY searched when its last search has finished.
//     Nothing else changes: the orders, one wave_movegen per turn, the budget tested before every node (a null child,
//     a reduced search and a re-search included), the cut rules, depth_done and CRL_OPP_CUT.
// Consequences.  (a) With D <= 2 no node has r >= 3 and none below the root has r >= 2: every output, `nodes`
// included, equals the search without this section.  (b) The search is no longer minimax over the full tree: move and
// score may differ from the ORD search even under a budget nothing reaches.  It stays a function of the root, its
// reversible history and the arguments.  (c) A null-move cut is never a mate score, and no null move is tried against
// a mate window, so a mate score still counts plies of real moves and null moves alike from the root.  (d) A null child
// has r - 3, and a node below the root has r <= 4 at the depths this opponent runs (D <= 5), so a null child has r <= 1:
// "not reached by a null move" never refuses a null move that the depth guard would have let through.  The guard is
// stated and kept for the rule's sake; at D <= 5 no output depends on it.
// Structure.  The main loop stays `while (nodes < budget)` with one wave_movegen per turn: the null child, a reduced
// search and a re-search are changes of state inside turns (which child the descent builds, and what the turn that
// hands its value up does with it), not loops of their own, so a logic error still ends as a flagged cut.  The
// entering node carries r (as -j for a quiescence node) beside its window in a scalar register; a frame keeps its r,
// whether its node is in check and what its current child is (a move, the null child, a reduced search, the
// re-search) in its spare pad word, written by lane 0 with the frame's other fields, and a node reads "reached by a
// null move" from its parent's frame: the parent's current child is the null child.
// sizeof(OppFrame) stays 608 and the LDS of a kernel is that of its non-selective sibling.  A node at k >= 1 has its
// tactical moves in front (ORDERING), so "not tactical" is the cursor against the stored number; the root asks the
// predicate (a promotion, or a piece has left the board: the same moves).  ONE call site of the evaluation per
// kernel: with quiescence ahead of the move generation (the stand-pat and the null move's last guard), without it
// behind the move generation (the horizon and that guard).  (tests/selective_util.py restates this section.)
//
// EXCHANGE (the EXC shapes of the _id kernels only: exchange = 1, an opt-in on top of ORDERING, so of ITERATIVE DEEPENING and a node
// budget, with Q >= 1; it combines freely with REPETITION, EVALUATION and SELECTIVE, and everything in those sections
// holds.  Every other launch tries every tactical move of a stand-pat node, as QUIESCENCE 4c says).  Delta and exchange
// pruning in quiescence; the margin 200 is conventional, untuned and fixed.
//     Where.  Only at a quiescence node that stands pat and searches moves -- QUIESCENCE 4c: not in check,
//     stand < beta, after alpha = max(alpha, stand); under SELECTIVE the quiescence node of that section.  Never at a
//     node in check (4b), at a node above the horizon, or at the root.
//     What.  After the victim partition the tactical moves mv[0 .. nt) pass two tests in this order; a move that fails
//     either is removed from the node's list and the others keep their order (a stable compaction).  The node then
//     searches what is left exactly as before; a removed move touches neither best nor alpha.  If nothing is left the
//     value is stand, as for a node without a tactical move (no frame).
//     value(.)  is the material of STATIC EVALUATION whichever evaluation the call uses: P 100, N 320, B 330, R 500,
//     Q 900 (a king's value is never read).  The victim of a move is the piece on its destination; an en-passant
//     capture has the victim P; a promotion onto an empty square has none, value 0.
//     1. Delta.  The move is removed if it is not a promotion and stand + value(victim) + 200 <= alpha.
//     2. Exchange.  The move is removed if SEE(m) < 0, the static exchange value on its destination square t:
//         the occupancy starts as the node's without the mover's origin square (and, en passant, without the captured
//         pawn) and with t;  gain[0] = value(victim), and a promotion adds value(promoted) - 100;  the piece on t is
//         the mover, or the promoted piece;
//         the sides then alternate, beginning with the opponent of the mover.  The side to capture takes with its
//         least valuable attacker of t: the pieces of that side which stand in the occupancy and attack t in it
//         (sliders stop at the first piece of the occupancy, so a slider behind a piece that has captured joins in: an
//         x-ray), in the order P, N, B, R, Q, K and inside a type the lowest square index first.  Without an attacker
//         the sequence ends.  A king captures only if the other side has no attacker of t in the occupancy as it is
//         before the king's capture; otherwise the sequence ends before it.  A king's capture ends the sequence;
//         capture d = 1, 2, .. has gain[d] = value(piece on t) - gain[d - 1]; the capturing piece then leaves the
//         occupancy and is the piece on t;
//         pins are ignored, and a pawn that captures on the last rank stays a pawn;
//         either side may stop before any of its captures: from the last capture back, gain[d - 1] =
//         -max(-gain[d - 1], gain[d]), and SEE(m) = gain[0].  Only its sign is read.
// Consequences.  (a) Off, nothing changes: the same entries are called and the same kernels launched.  (b) On, from a
// root whose search meets no removable move, every output equals the search without this section, `nodes` included.
// (c) The search is no longer minimax over the full quiescence tree; it stays a function of the root, its reversible
// history and the arguments.  (d) The filter generates no moves, so it costs no node: a node becomes dearer in time,
// not in count.  (e) gain[0] >= 0, so a capture of a piece worth at least the mover is never removed by test 2.
// Structure.  One site, behind opp_partition_victim in the 4c branch.  Lane i judges mv[i], 64 moves per pass and as
// many passes as nt needs; each lane runs its own exchange loop on the wave-uniform board (the attack sets of
// attackers_to with the lane's destination and occupancy, both colours in one set per capture: only the sliders'
// share changes with the occupancy), so the loop is divergent and a pass lasts as long as its longest exchange.  The
// SIGN of SEE needs no list of gains: the lane keeps one balance and one answer bit -- balance = value(piece on t) - gain[0],
// answer "not negative"; if balance <= 0 the answer stands; every capture flips the answer and sets balance =
// value(capturer) - balance, and the sequence is left as soon as balance < answer; a king flips the answer only if it
// may capture.  Nothing is indexed per lane, so nothing goes to scratch.  One ballot per pass and prefix popcounts
// compact the list, the scheme of opp_partition.  Frames, LDS and sizeof(OppFrame) stay; F->nt of such a node is the
// filtered count.  k_opponent_exchange judges, without a search, every legal move of a slot's current position with
// test 2 alone.  (tests/exchange_util.py restates this section and checks the sign form against the definition.)
#pragma once
#include "search.hpp"

namespace crl {

constexpr int OPP_MAX_DEPTH = 5;
constexpr int OPP_MAX_QUIESCENCE = 6;
constexpr int OPP_INF = 32000;
constexpr int OPP_MATE = 30000;
constexpr uint8_t OPP_CUT = 1, OPP_SKIPPED = 2;
// SELECTIVE: scores from here on are mates (no null move against such a beta; a null-move cut is capped to beta)
constexpr int OPP_NULL_MATE = 29000;
// SELECTIVE, the frame's pad word.  Bits 0-1: what the child being searched is -- a move at full depth (the first
// search of one), the null child, a reduced search, the re-search after a reduced one.  Bit 2: the node is in check.
// Bits 8-15, signed: the node's remaining depth r where r > 0, otherwise -j, its quiescence ply.
constexpr uint32_t OPP_CHILD_MOVE = 0, OPP_CHILD_NULL = 1, OPP_CHILD_REDUCED = 2, OPP_CHILD_AGAIN = 3;
constexpr uint32_t OPP_NODE_IN_CHECK = 4;

struct __attribute__((aligned(16))) OppFrame {
    Board b;
    u16 mv[MAX_MOVES];
    int32_t cur, n, alpha, beta, best;
    int32_t nt;                                // ORDERING: the tactical moves of the node are mv[0 .. nt)
    uint32_t killers;                          // ORDERING: killer A (low half) and B of this ply
    int32_t pad;                               // SELECTIVE: the OPP_CHILD_* / OPP_NODE_* bits and the remaining depth
};
static_assert(sizeof(OppFrame) == 608, "OppFrame must be 608 bytes");

template <bool QS>                         // QS: a search with quiescence plies
union OppLds {
    OppFrame f[QS ? OPP_MAX_DEPTH + OPP_MAX_QUIESCENCE : OPP_MAX_DEPTH + 1];
    WaveLds w;                             // game_push, after the search
};

// REPETITION: what lives beside the frames.  hh[i - 1] is the hash of the position i plies before the root (i = 1 ..
// the root's reversible history, at most OPP_REP_WINDOW); ph[k] / ps[k] are the hash of the key-normalised board of
// the node that holds frame k and its state word with the derived en-passant bit.
constexpr int OPP_REP_WINDOW = 99;
template <bool QS>
struct OppRepLds {
    u64 hh[OPP_REP_WINDOW];
    u64 ph[QS ? OPP_MAX_DEPTH + OPP_MAX_QUIESCENCE : OPP_MAX_DEPTH + 1];
    u32 ps[QS ? OPP_MAX_DEPTH + OPP_MAX_QUIESCENCE : OPP_MAX_DEPTH + 1];
};
// ... and where the root stands: at tree ply `tp` of slot g (0: the game's current position), whose game ply is `ply`
struct OppRepRoot { const Dev *d; int g, tp, ply; };

// a wave-uniform board read from LDS, moved to scalar registers
__device__ inline Board uni_board(const Board &x)
{
    Board b;
#pragma unroll
    for (int i = 0; i < 6; i++)
        b.bb[i] = (u64)(u32)uni((int)(u32)x.bb[i]) | ((u64)(u32)uni((int)(u32)(x.bb[i] >> 32)) << 32);
    b.white = (u64)(u32)uni((int)(u32)x.white) | ((u64)(u32)uni((int)(u32)(x.white >> 32)) << 32);
    b.state = (u32)uni((int)x.state);
    b.pad = 0;
    return b;
}

__device__ inline int opp_evaluate(const Board &b, int lane)
{
    const int pt = piece_at(b, lane);
    const int f = lane & 7, r = lane >> 3;
    const int rf = f < 7 - f ? f : 7 - f, rr = r < 7 - r ? r : 7 - r;
    const int ring = rf < rr ? rf : rr;
    const bool white = (b.white >> lane) & 1;
    int v = 0;
    if (pt == PAWN) v = 100 + 5 * ring + 6 * (white ? r - 1 : 6 - r);
    else if (pt == KNIGHT) v = 320 + 10 * ring;
    else if (pt == BISHOP) v = 330 + 5 * ring;
    else if (pt == ROOK) v = 500;
    else if (pt == QUEEN) v = 900 + 2 * ring;
    else if (pt == KING) v = -10 * ring;
    if (!white) v = -v;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return st_turn(b.state) ? v : -v;
}

// EVALUATION of the header comment: the positional static evaluation, from the side to move.  `b` is wave-uniform.
__device__ inline u64 opp_nfill(u64 x) { x |= x << 8; x |= x << 16; return x | (x << 32); }
__device__ inline u64 opp_sfill(u64 x) { x |= x >> 8; x |= x >> 16; return x | (x >> 32); }
__device__ inline u64 opp_widen(u64 x) { return x | ((x << 1) & ~FILE_A) | ((x >> 1) & ~FILE_H); }

__device__ inline int opp_evaluate_positional(const Board &b, int lane)
{
    // Inside the search loop everything below that depends on the lane alone (the ring, the line masks, the shelter
    // squares ..) is loop-invariant, and hoisted out it would hold some twenty VGPRs for the whole search.  The empty
    // asm makes the lane number opaque, so these values are computed where they are used and die there.
    asm volatile("" : "+v"(lane));
    const u64 occ = occupied(b);
    const u64 wh = b.white & occ, bl = occ & ~b.white;
    // ---- the lane's piece and its attack set: the slider lines under predication, each once for the wave
    const int pt = piece_at(b, lane);
    const bool white = (wh >> lane) & 1;
    const int f = lane & 7, r = lane >> 3;
    const int rf = f < 7 - f ? f : 7 - f, rr = r < 7 - r ? r : 7 - r;
    const int ring = rf < rr ? rf : rr;
    const int rel = white ? r : 7 - r;
    u64 at = 0;
    if (pt == KNIGHT) at = knight_attacks(lane);
    if (pt == BISHOP || pt == QUEEN) at = bishop_attacks(lane, occ);
    if (pt == ROOK || pt == QUEEN) at |= rook_attacks(lane, occ);
    // ---- uniform masks from the scalar board, each read by the lanes at once: bit sq = the pawn on sq has the
    // property, whichever its colour; the files that hold a pawn of a colour are eight bits
    const u64 wp = b.bb[PAWN] & wh, bp = b.bb[PAWN] & bl;
    const u64 stopped = (opp_sfill(opp_widen(bp) >> 8) & wp) | (opp_nfill(opp_widen(wp) << 8) & bp);    // not passed
    const u64 doubled = (opp_sfill(wp >> 8) & wp) | (opp_nfill(bp << 8) & bp);
    const bool is_stopped = (stopped >> lane) & 1, is_doubled = (doubled >> lane) & 1;
    const u32 wf8 = (u32)opp_sfill(wp) & 0xFFu, bf8 = (u32)opp_sfill(bp) & 0xFFu;
    const u32 ownf = white ? wf8 : bf8, enf = white ? bf8 : wf8;
    const bool is_lonely = !((((ownf << 1) | (ownf >> 1)) >> f) & 1);                  // (read by a pawn)
    const bool is_open = !(((ownf | enf) >> f) & 1), is_half = !((ownf >> f) & 1);     // (by a rook; half: not open)
    // ---- per colour, against uniform masks (no 64-bit select per lane): the squares of the attack set not held by
    // an own piece, those of them an enemy pawn attacks, and whether the set meets the enemy king's zone
    const u64 pa_w = ((wp << 9) & ~FILE_A) | ((wp << 7) & ~FILE_H), pa_b = ((bp >> 7) & ~FILE_A) | ((bp >> 9) & ~FILE_H);
    const u64 wrow = opp_widen(b.bb[KING] & wh), brow = opp_widen(b.bb[KING] & bl);
    const u64 zone_w = wrow | (wrow << 8) | (wrow >> 8), zone_b = brow | (brow << 8) | (brow >> 8);
    const int free_sq = white ? popc(at & ~wh) : popc(at & ~bl);
    const int guarded = white ? popc(at & ~wh & pa_b) : popc(at & ~bl & pa_w);
    const int m = pt == ROOK ? free_sq : free_sq - guarded;
    const bool hit = ((white ? zone_b : zone_w) & at) != 0;
    int mg = 0, eg = 0;
    if (pt == PAWN) {
        const int adv = rel - 1;
        mg = 100 + 5 * ring + 6 * adv;
        eg = 100 + 12 * adv;
        if (!is_stopped) {                                 // {0,5,10,20,40,70} and twice that
            const int pm = adv <= 0 ? 0 : (5 << (adv - 1)) - (adv == 5 ? 10 : 0);      // adv = 5: 80 - 10
            mg += pm; eg += 2 * pm;
        }
        if (is_doubled) { mg -= 10; eg -= 20; }
        if (is_lonely) { mg -= 10; eg -= 15; }
    } else if (pt == KNIGHT) {
        mg = eg = 320 + 10 * ring + 4 * m;
        if (hit) mg += 8;
    } else if (pt == BISHOP) {
        mg = eg = 330 + 5 * ring + 4 * m;
        if (hit) mg += 8;
    } else if (pt == ROOK) {
        mg = 500 + 2 * m;
        eg = 500 + 4 * m;
        if (is_open) { mg += 20; eg += 10; }
        else if (is_half) { mg += 10; eg += 5; }
        if (rel == 6) { mg += 10; eg += 20; }
        if (hit) mg += 12;
    } else if (pt == QUEEN) {
        mg = 900 + 2 * ring + m;
        eg = 900 + 2 * ring + 2 * m;
        if (hit) mg += 20;
    } else if (pt == KING) {
        mg = -10 * ring;
        eg = 10 * ring;
        if (rel <= 1) {                                    // the shelter: own pawns on the next two ranks ahead
            const u64 row = opp_widen(bit(lane));
            mg += 8 * (white ? popc(((row << 8) | (row << 16)) & wp) : popc(((row >> 8) | (row >> 16)) & bp));
        }
    }
    int v = mg * 65536 + eg;                               // |mg|, |eg| < 2^15: one reduction carries both
    if (!white) v = -v;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    // ---- uniform again: the bishop pairs, the phase, the taper
    int EG = (int)(short)(v & 0xFFFF);
    int MG = (v - EG) >> 16;                               // (v - EG is a multiple of 65536)
    const int pair = (popc(b.bb[BISHOP] & wh) >= 2 ? 1 : 0) - (popc(b.bb[BISHOP] & bl) >= 2 ? 1 : 0);
    MG += 30 * pair;
    EG += 40 * pair;
    int ph = popc(b.bb[KNIGHT]) + popc(b.bb[BISHOP]) + 2 * popc(b.bb[ROOK]) + 4 * popc(b.bb[QUEEN]);
    if (ph > 24) ph = 24;
    const int w = (MG * ph + EG * (24 - ph)) / 24;
    return (st_turn(b.state) ? w : -w) + 10;
}

// the static evaluation of a search: POS selects EVALUATION, otherwise STATIC EVALUATION
template <bool POS>
__device__ inline int opp_static(const Board &b, int lane)
{
    if (POS) return opp_evaluate_positional(b, lane);
    return opp_evaluate(b, lane);
}

__device__ inline bool opp_tactical(const Board &b, u64 occ, u64 own, u32 mv)
{
    const int from = mv & 63, to = (mv >> 6) & 63;
    const u64 tb = bit(to);
    if ((mv >> 12) & 7) return true;
    if (occ & ~own & tb) return true;
    return (b.bb[PAWN] & bit(from)) && (from & 7) != (to & 7) && !(occ & tb);
}

// stable partition of mv[0 .. n): tactical moves first.  mv is visible on entry and on return.
__device__ inline void opp_partition(const Board &b, u16 *mv, int n, int lane)
{
    const u64 occ = occupied(b);
    const u64 own = st_turn(b.state) ? b.white : (occ & ~b.white);
    const u64 below = bit(lane) - 1;
    u32 m[4];
    u64 T[4], V[4];
    int nt = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int i = c * 64 + lane;
        const bool valid = i < n;
        m[c] = valid ? mv[i] : 0u;
        V[c] = __ballot(valid);
        T[c] = __ballot(valid && opp_tactical(b, occ, own, m[c]));
        nt += popc(T[c]);
    }
    __syncthreads();                                   // every move read before any is rewritten
    int bt = 0, bq = nt;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const u64 Q = V[c] & ~T[c];
        if (V[c] & bit(lane)) {
            const int pos = (T[c] & bit(lane)) ? bt + popc(T[c] & below) : bq + popc(Q & below);
            mv[pos] = (u16)m[c];
        }
        bt += popc(T[c]);
        bq += popc(Q);
    }
    __syncthreads();
}

// whether the side to move is in check (what wave_movegen reports as in_check), wave-uniform
__device__ inline bool opp_in_check(const Board &b)
{
    const bool white = st_turn(b.state);
    const u64 occ = occupied(b);
    const u64 kbb = b.bb[KING] & (white ? b.white : (occ & ~b.white));
    return kbb && attackers_to(b, msb(kbb), occ, !white) != 0;
}

// the class of a move in a quiescence node that stands pat: 0 .. 4 = its victim Q R B N P (en passant: P), 5 = a
// promotion that captures nothing, 6 = not tactical
__device__ inline int opp_victim_class(const Board &b, u64 occ, u64 own, u32 mv)
{
    const int to = (mv >> 6) & 63;
    if (occ & ~own & bit(to)) {
        const int pt = piece_at(b, to);
        return pt >= QUEEN ? 0 : QUEEN - pt;               // (a legal move never takes a king)
    }
    if (!opp_tactical(b, occ, own, mv)) return 6;
    return ((mv >> 12) & 7) ? 5 : 4;
}

// stable partition of mv[0 .. n) by opp_victim_class, the scheme of opp_partition with seven ballots per 64 moves.
// Returns the number of tactical moves: they are mv[0 .. that).  mv is visible on entry and on return.
// KL: ORDERING -- inside class 6, the quiet moves, killer `ka` comes first, then killer `kb`, then the others in
// generation order: the nine classes of the header.  A killer is ONE move, so its class needs no ballot row of its own:
// one ballot per 64 moves finds its rank among the quiet moves, and every other quiet move steps back by the killers
// that stood behind it.  (A tactical move equal to a killer is no hit.)  Every line marked KL folds away without it.
template <bool KL = false>
__device__ inline int opp_partition_victim(const Board &b, u16 *mv, int n, int lane, u32 ka = NO_MOVE, u32 kb = NO_MOVE)
{
    constexpr int NC = 7;
    const u64 occ = occupied(b);
    const u64 own = st_turn(b.state) ? b.white : (occ & ~b.white);
    const u64 below = bit(lane) - 1;
    u32 m[4];
    int cl[4], tot[NC];
    u64 C[4][NC];
    int ra = -1, rb = -1;                              // KL: the ranks of the killers among the quiet moves, -1: absent
#pragma unroll
    for (int q = 0; q < NC; q++) tot[q] = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int i = c * 64 + lane;
        const bool valid = i < n;
        m[c] = valid ? mv[i] : 0u;
        cl[c] = valid ? opp_victim_class(b, occ, own, m[c]) : -1;
#pragma unroll
        for (int q = 0; q < NC; q++) {
            C[c][q] = __ballot(cl[c] == q);
            if (KL && q == NC - 1) {                   // (tot[6] still counts the quiet moves of the chunks before)
                const u64 ha = __ballot(cl[c] == q && m[c] == ka), hb = __ballot(cl[c] == q && m[c] == kb);
                if (ha) ra = tot[q] + popc(C[c][q] & (ha - 1));        // (a legal move stands in the list once)
                if (hb) rb = tot[q] + popc(C[c][q] & (hb - 1));
            }
            tot[q] += popc(C[c][q]);
        }
    }
    __syncthreads();                                   // every move read before any is rewritten
    int base[NC];
    base[0] = 0;
#pragma unroll
    for (int q = 1; q < NC; q++) base[q] = base[q - 1] + tot[q - 1];
    const int quiet0 = base[NC - 1];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        int pos = -1;
#pragma unroll
        for (int q = 0; q < NC; q++) {
            if (cl[c] == q) pos = base[q] + popc(C[c][q] & below);
            base[q] += popc(C[c][q]);
        }
        if (KL && cl[c] == NC - 1) {                   // a permutation of the quiet ranks: ka, kb, the others in order
            const int r = pos - quiet0;
            pos = quiet0 + (r == ra ? 0 : r == rb ? (ra >= 0) : r + (ra > r) + (rb > r));
        }
        if (pos >= 0) mv[pos] = (u16)m[c];             // pos < n: the classes partition the n valid moves
    }
    __syncthreads();
    return n - tot[NC - 1];
}

// ITERATIVE DEEPENING, the root's order: the stable move-to-front of `pm` in mv[0 .. n), where it stands at some p --
// mv[1 .. p] take mv[0 .. p - 1] (each lane its left neighbour's move, lane 0 the last lane's of the 64 moves before)
// and mv[0] = pm.  A move that is not in the list, or stands in front already, changes nothing.  mv is visible on entry
// and on return.
__device__ inline void opp_move_to_front(u16 *mv, int n, u32 pm, int lane)
{
    u32 m[4];
    int p = -1;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int i = c * 64 + lane;
        m[c] = i < n ? mv[i] : (u32)NO_MOVE;
        const u64 hit = __ballot(i < n && m[c] == pm);
        if (hit && p < 0) p = c * 64 + lsb(hit);
    }
    if (p <= 0) return;                                // (wave-uniform: p comes from ballots)
    __syncthreads();                                   // every move read before any is rewritten
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int i = c * 64 + lane;
        u32 left = __shfl_up(m[c], 1);
        const u32 carry = c > 0 ? __shfl(m[c > 0 ? c - 1 : 0], 63) : pm;
        if (lane == 0) left = carry;
        if (i <= p) mv[i] = (u16)left;                 // i <= p < n
    }
    __syncthreads();
}

// EXCHANGE of the header comment.  The material of a piece type (selects, no table: nothing is indexed per lane)
__device__ inline int opp_value(int pt)
{
    return pt == PAWN ? 100 : pt == KNIGHT ? 320 : pt == BISHOP ? 330 : pt == ROOK ? 500 : pt == QUEEN ? 900 : 0;
}

// the value of the victim of the tactical move mv of `b` (occ: its occupancy): en passant P, a quiet promotion 0
__device__ inline int opp_victim_value(const Board &b, u64 occ, u32 mv)
{
    const int to = (mv >> 6) & 63;
    if (occ & bit(to)) return opp_value(piece_at(b, to));
    return ((mv >> 12) & 7) ? 0 : 100;
}

// whether SEE(mv) >= 0 for the TACTICAL move mv of `b`: the alternating-bound form of the header.  `b` is wave-uniform,
// mv is the lane's; every lane that enters runs its own loop, at most once per piece on the board.
__device__ inline bool opp_see_not_negative(const Board &b, u64 occ0, u32 mv)
{
    const int from = mv & 63, to = (mv >> 6) & 63, promo = (mv >> 12) & 7;
    const bool white = st_turn(b.state);
    const u64 tb = bit(to);
    u64 occ = occ0 & ~bit(from);
    int first;
    if (occ0 & tb) first = opp_value(piece_at(b, to));
    else if (promo) first = 0;
    else {                                                 // tactical, nothing on t, no promotion: en passant
        first = 100;
        occ &= ~bit(white ? to - 8 : to + 8);              // (t is on rank 6 or 3)
    }
    occ |= tb;
    int on_t = opp_value(piece_at(b, from));
    if (promo) { on_t = opp_value(promo - 1); first += on_t - 100; }
    int balance = on_t - first;
    if (balance <= 0) return true;                         // not negative even if the piece on t is lost for nothing
    // the attackers of t of BOTH colours in one set per capture: only the sliders' share changes with the occupancy
    const u64 rq = b.bb[ROOK] | b.bb[QUEEN], bq = b.bb[BISHOP] | b.bb[QUEEN];
    const u64 fixed = (knight_attacks(to) & b.bb[KNIGHT]) | (king_attacks(to) & b.bb[KING]) |
                      (b.bb[PAWN] & ((pawn_attacks(to, false) & b.white) | (pawn_attacks(to, true) & ~b.white)));
    bool answer = true, side = white;
    for (;;) {
        side = !side;
        const u64 all = (fixed | (rook_attacks(to, occ) & rq) | (bishop_attacks(to, occ) & bq)) & occ;
        const u64 att = all & (side ? b.white : ~b.white);
        if (!att) break;
        int t = KING;
        u64 s = att;
#pragma unroll
        for (int q = QUEEN; q >= PAWN; q--)
            if (att & b.bb[q]) { t = q; s = att & b.bb[q]; }
        if (t == KING) {                                   // it captures only where nothing could take it back
            if (!(all & ~att)) answer = !answer;
            break;
        }
        answer = !answer;
        occ &= ~(s & (0ull - s));                          // the lowest square of the type
        balance = opp_value(t) - balance;
        if (balance < (answer ? 1 : 0)) break;
    }
    return answer;
}

// the two tests on the tactical moves mv[0 .. nt) of the stand-pat node `b`, and the stable compaction of those that
// pass.  Returns how many are left: they are mv[0 .. that).  mv is visible on entry and on return; nt, stand and alpha
// are wave-uniform.  A pass writes at or below what it read, and later passes read above it.
__device__ inline int opp_exchange_filter(const Board &b, u16 *mv, int nt, int stand, int alpha, int lane)
{
    const u64 occ = occupied(b);
    const u64 below = bit(lane) - 1;
    int kept = 0;
    for (int base = 0; base < nt; base += 64) {
        const int i = base + lane;
        const u32 m = i < nt ? mv[i] : 0u;
        bool keep = false;
        if (i < nt) {
            keep = ((m >> 12) & 7) != 0 || stand + opp_victim_value(b, occ, m) + 200 > alpha;      // 1. delta
            if (keep) keep = opp_see_not_negative(b, occ, m);                                      // 2. exchange
        }
        const u64 K = __ballot(keep);
        __syncthreads();                                   // every move of the pass read before any is rewritten
        if (keep) mv[kept + popc(K & below)] = (u16)m;     // kept + rank <= i < nt
        kept += popc(K);
    }
    __syncthreads();
    return kept;
}

// The search of the header comment, stated once for both kernels: from `root` to depth Dmax (1 .. OPP_MAX_DEPTH, checked by
// the caller) with Q quiescence plies (QS: 1 .. OPP_MAX_QUIESCENCE, checked by the caller; otherwise not read) under the
// node limit, in the frames f[0 .. Dmax] or, QS, f[0 .. Dmax + Q - 1].  mv: the move (NO_MOVE only for a root without a legal
// move or with a result, which no caller hands in); score, nodes; done = false is the cut.  Every value is
// wave-uniform.  The frames are dead on return, but not yet fenced: a barrier comes before their bytes are reused.
// ID: ITERATIVE DEEPENING of the header comment -- Dmax is the maximum depth and `limit` the node budget; the loop below
// then searches to D = 1, 2, .. Dmax, and depth_done is the last iteration that finished (done: it was Dmax).  Without
// ID, D = Dmax throughout, depth_done is not set and every line marked ID folds away.
// ORD: ORDERING of the header comment, on top of ID; NF is the number of frames behind f (their killers are cleared
// here).  Every line marked ORD folds away without it.
// REP: REPETITION of the header comment, on top of ID; rs and rr are read only then.  Every line marked REP folds away
// without it.
// POS: EVALUATION of the header comment in place of STATIC EVALUATION, on top of ID; nothing else reads it.
// SEL: SELECTIVE of the header comment, on top of ORD.  The entering node carries `e` (its remaining depth r where
// r > 0, otherwise -j) beside its window; a frame keeps e, whether its node is in check and what its current child is
// in its pad word, so a node reads there whether a null move led to it.  Every line marked SEL folds away without it.
// EXC: EXCHANGE of the header comment, on top of ORD and QS: one site, the filter behind the victim partition of 4c.
struct OppResult { u32 mv; int score; long long nodes; bool done; int depth_done; };

// SEL: the board after a null move -- the side to move exchanged, no en-passant square, the halfmove clock 0
__device__ inline Board opp_null_board(const Board &b)
{
    Board n = b;
    n.state = mk_state(st_turn(b.state) ^ 1u, st_castle(b.state), (u32)NO_EP, 0u, 0u);
    n.pad = 0;
    return n;
}

// SEL: the null move's guards that need neither the moves nor the evaluation, for the node `b` at ply k of the frames
// f with the remaining depth e, and beta.  (Whether the node was reached by a null move stands in its parent's frame.)
__device__ inline bool opp_null_guards(const Board &b, int k, int e, int beta, const OppFrame *f)
{
    const u64 occ = occupied(b);
    const u64 own = st_turn(b.state) ? b.white & occ : occ & ~b.white;
    if (!(k >= 1 && e >= 2 && beta > -OPP_NULL_MATE && beta < OPP_NULL_MATE &&
          (own & (b.bb[KNIGHT] | b.bb[BISHOP] | b.bb[ROOK] | b.bb[QUEEN])) != 0))
        return false;
    return ((u32)uni(f[k - 1].pad) & 3u) != OPP_CHILD_NULL;
}

// THE SHAPES of the budgeted search: six flags, one bit each in this order (the index of the host's kernel tables).
// SELECTIVE requires ORDERING; EXCHANGE requires ORDERING and quiescence plies.
enum : unsigned { OPP_SHAPE_QS = 1, OPP_SHAPE_ORD = 2, OPP_SHAPE_REP = 4, OPP_SHAPE_POS = 8, OPP_SHAPE_SEL = 16,
                  OPP_SHAPE_EXC = 32, OPP_SHAPES = 64 };
constexpr bool opp_shape_legal(bool QS, bool ORD, bool /*REP*/, bool /*POS*/, bool SEL, bool EXC)
{
    return (ORD || !SEL) && ((ORD && QS) || !EXC);
}
constexpr bool opp_shape_legal(unsigned i)
{
    return opp_shape_legal(i & OPP_SHAPE_QS, i & OPP_SHAPE_ORD, i & OPP_SHAPE_REP, i & OPP_SHAPE_POS,
                           i & OPP_SHAPE_SEL, i & OPP_SHAPE_EXC);
}
constexpr int opp_legal_shapes()
{
    int n = 0;
    for (unsigned i = 0; i < OPP_SHAPES; i++) n += opp_shape_legal(i) ? 1 : 0;
    return n;
}
static_assert(opp_legal_shapes() == 32, "the budgeted search has 32 legal shapes");

template <bool QS, bool ID = false, bool ORD = false, bool REP = false, bool POS = false, bool SEL = false,
          bool EXC = false>
__device__ inline OppResult opp_search(const Board &root, int Dmax, int Q, long long limit, OppFrame *f, int lane,
                                       OppRepLds<QS> *rs = nullptr, OppRepRoot rr = OppRepRoot())
{
    static_assert(ID || !ORD, "ORDERING requires ITERATIVE DEEPENING");
    static_assert(ID || !REP, "REPETITION requires ITERATIVE DEEPENING");
    static_assert(ID || !POS, "EVALUATION requires ITERATIVE DEEPENING");
    static_assert(opp_shape_legal(QS, ORD, REP, POS, SEL, EXC), "not a shape of the search (opp_shape_legal)");
    int K = 0;                                             // REP: the positions behind the root that hh holds
    if (ORD) {                                             // both killers of every ply: NO_MOVE
        constexpr int NF = QS ? OPP_MAX_DEPTH + OPP_MAX_QUIESCENCE : OPP_MAX_DEPTH + 1;
        if (lane < NF) f[lane].killers = ((u32)NO_MOVE << 16) | (u32)NO_MOVE;
    }
    if (REP) {                                             // the root's reversible history, as far as it exists
        const int c0 = (int)st_clock(root.state);
        K = c0 < OPP_REP_WINDOW ? c0 : OPP_REP_WINDOW;
        const int have = rr.tp + (rr.ply < HIST_RING - 1 ? rr.ply : HIST_RING - 1);
        if (K > have) K = have;
        for (int i = lane + 1; i <= K; i += 64) rs->hh[i - 1] = *past_ref(*rr.d, rr.g, rr.tp - i, rr.ply, rr.ply).h;
    }
    if (ORD || REP) __syncthreads();
    Board b = root;
    int k = 0, a = -OPP_INF, be = OPP_INF, v = 0, root_best = -OPP_INF;
    u32 best_mv = NO_MOVE, first_mv = NO_MOVE;
    bool done = false;
    long long nodes = 0;
    int D = ID ? 1 : Dmax, depth_done = 0, held_score = -OPP_INF;      // ID: the iteration; what the last whole one gave
    u32 held_mv = NO_MOVE;
    int e = D;                                             // SEL: of the entering node, as a, be
    while (nodes < limit) {
        // ---- enter the node `b` at ply k, window (a, be)
        OppFrame *const F = f + k;                         // (read only where the node searches moves: k < D + Q)
        if (SEL && k >= (QS ? D + Q : D)) e = QS ? -Q : 0; // (r falls by at least 1 per ply: never taken.  The frames end here)
        const bool quiet = QS && (SEL ? e <= 0 : k >= D);  // a quiescence node, j = k - D; SEL: j = -e
        int stand = 0;
        bool chk = false;
        bool nullc = false;                                // SEL: the null move's guards that need no move generation
        // (SEL: ONE place evaluates per kernel.  With quiescence, ahead of the move generation: the stand-pat and the
        // null move's last guard; without, behind it: the horizon and that guard)
        if (SEL) {
            if (QS) {
                nullc = opp_null_guards(b, k, e, be, f);
                if (quiet || nullc) stand = uni(opp_static<POS>(b, lane));
            }
            if (quiet) chk = opp_in_check(b);
        } else if (quiet) { stand = uni(opp_static<POS>(b, lane)); chk = opp_in_check(b); }
        // a node that searches no move: the horizon; with quiescence 4a, and the stand-pat at or above beta of 4c
        const bool horizon = QS ? quiet && ((SEL ? -e >= Q : k >= D + Q) || (!chk && stand >= be)) : (SEL ? e <= 0 : k == D);
        MoveGenInfo mi = wave_movegen(b, lane, horizon ? nullptr : F->mv);
        nodes++;
        const int n = uni(mi.n);
        const int res = uni(position_result(b, n, mi.in_check, 1));
        bool have_v = true;
        bool rep_hit = false;                              // REP: step 3b
        u64 nh = 0;                                        // REP: the hash and the state of the key-normalised node
        u32 ns = 0;
        if (REP && res == RESULT_NONE) {
            const int clock = (int)st_clock(b.state);      // (< 100: no result)
            if (!horizon || (k >= 1 && clock >= 4)) {
                Board nb = b;
                nb.state = ns = (b.state & ~(1u << 20)) | ((uni((int)mi.ep_legal) ? 1u : 0u) << 20);
                nh = board_hash(nb);
                if (k >= 1 && clock >= 4) {
                    const int dist = 2 * (lane + 2);       // 4, 6, .. 130 >= clock: one pass
                    bool hit = false;
                    if (dist <= clock && dist <= k) {      // on the path: ply k - dist, its frame's board
                        const int j = k - dist;
                        if (rs->ph[j] == nh) {
                            Board o = f[j].b;
                            o.state = rs->ps[j];
                            hit = same_key(o, nb);
                        }
                    } else if (dist <= clock && dist - k <= K) {           // behind the root
                        const int hd = dist - k;
                        if (rs->hh[hd - 1] == nh)
                            hit = same_key(*past_ref(*rr.d, rr.g, rr.tp - hd, rr.ply, rr.ply).b, nb);
                    }
                    rep_hit = __ballot(hit) != 0;
                }
            }
        }
        if (SEL && !QS && res == RESULT_NONE && !(REP && rep_hit)) {
            nullc = !horizon && opp_null_guards(b, k, e, be, f);   // (in check or not: that guard comes below)
            if (horizon || nullc) stand = uni(opp_static<POS>(b, lane));
        }
        if (res != RESULT_NONE) v = res == 0 ? 0 : -(OPP_MATE - k);
        else if (REP && rep_hit) v = 0;
        else if (horizon) v = QS || SEL ? stand : uni(opp_static<POS>(b, lane));
        else {
            __syncthreads();                               // F->mv visible
            int cnt = n, best0 = -OPP_INF, nt = 0;         // ORD: nt, the node's tactical moves
            if (quiet && !chk) {                           // 4c: stand pat, then the tactical moves by victim
                cnt = opp_partition_victim(b, F->mv, n, lane);
                best0 = stand;
                if (stand > a) a = stand;
                if (EXC) cnt = opp_exchange_filter(b, F->mv, cnt, stand, a, lane);
                nt = cnt;                                  // (never below the cursor: no killer from this frame)
            } else if (k > 0) {
                if (ORD) {
                    const u32 kl = (u32)uni((int)F->killers);
                    nt = opp_partition_victim<true>(b, F->mv, n, lane, kl & 0xFFFFu, kl >> 16);
                } else opp_partition(b, F->mv, n, lane);
            } else {
                first_mv = (u32)uni((int)F->mv[0]);
                if (ID && held_mv != NO_MOVE) opp_move_to_front(F->mv, n, held_mv, lane);
            }
            if (QS && cnt == 0) v = stand;                 // 4c without a tactical move (cnt = n > 0 everywhere else)
            else {
                // SEL: the null child is searched before any move (nullc: k >= 1, r >= 2, so no quiescence node)
                const bool in_chk = SEL && (quiet ? chk : uni((int)mi.in_check) != 0);
                const bool null_first = SEL && nullc && !in_chk && stand >= be;
                if (lane == 0) {
                    F->b = b; F->cur = 0; F->n = cnt; F->alpha = a; F->beta = be; F->best = best0;
                    if (ORD) F->nt = nt;
                    if (SEL) F->pad = (int32_t)((null_first ? OPP_CHILD_NULL : OPP_CHILD_MOVE) |
                                                (in_chk ? OPP_NODE_IN_CHECK : 0u) | (((u32)e & 0xFFu) << 8));
                    if (REP) { rs->ph[k] = nh; rs->ps[k] = ns; }
                }
                __syncthreads();
                have_v = false;
            }
        }
        // ---- hand v up: every turn lowers k, so at most d + Q + 1 of them
        bool again = false;                                // ID: this turn finished an iteration below Dmax
        while (have_v) {
            if (k == 0) {
                if (ID) {
                    held_mv = best_mv; held_score = v; depth_done = D;
                    // the next iteration: ply 0, the full window, no best yet.  (A root that searched a move wrote its
                    // frame, so the root's board is read back from there; one with a result -- no caller hands one in
                    // -- searched none and ends here as it does without ID.)
                    if (D < Dmax && best_mv != NO_MOVE) {
                        D++;
                        b = uni_board(f[0].b); a = -OPP_INF; be = OPP_INF;
                        best_mv = NO_MOVE; root_best = -OPP_INF;
                        e = D;
                        again = true;
                        break;
                    }
                }
                done = true;
                break;
            }
            k--;
            OppFrame &P = f[k];
            const int sc = -v, pn = uni(P.n), pb = uni(P.beta);
            int cur = uni(P.cur), best = uni(P.best), al = uni(P.alpha);
            u32 pad = 0;
            if (SEL) {
                pad = (u32)uni(P.pad);
                const u32 child = pad & 3u;
                if (child == OPP_CHILD_NULL && sc >= pb) {     // the null-move cut: frame k returns, no killer
                    v = sc >= OPP_NULL_MATE ? pb : sc;
                    continue;
                }
                // the null move failed: the moves, from the first; a reduced search above alpha: the move again
                if (child == OPP_CHILD_NULL || (child == OPP_CHILD_REDUCED && sc > al)) {
                    __syncthreads();                           // the frame was read
                    if (lane == 0)
                        P.pad = (int32_t)((pad & ~3u) | (child == OPP_CHILD_NULL ? OPP_CHILD_MOVE : OPP_CHILD_AGAIN));
                    __syncthreads();
                    have_v = false;
                    continue;
                }
            }
            if (sc > best) {
                best = sc;
                if (k == 0) { best_mv = (u32)uni((int)P.mv[cur]); root_best = sc; }
            }
            if (sc > al) al = sc;
            u32 kl = 0;
            bool set_killer = false;                       // ORD: a cut below the root by a quiet move other than A
            if (ORD && k > 0 && al >= pb && cur >= uni(P.nt)) {
                const u32 m = (u32)uni((int)P.mv[cur]);
                kl = (u32)uni((int)P.killers);
                set_killer = m != (kl & 0xFFFFu);
                kl = (kl << 16) | m;                       // B = A, A = m
            }
            cur++;
            __syncthreads();                               // the frame was read
            if (lane == 0) {
                P.cur = cur; P.best = best; P.alpha = al;
                if (ORD && set_killer) P.killers = kl;
                if (SEL) P.pad = (int32_t)(pad & ~3u);     // the next child: a move, not yet searched
            }
            __syncthreads();
            if (cur < pn && al < pb) have_v = false;       // frame k has a next move to search
            else v = best;                                 // exhausted or cut: it returns its best
        }
        if (done) break;
        if (ID && again) continue;                         // (the budget is tested before the new root like any node)
        // ---- descend: the next move of frame k  (k < D + Q: a frame with moves to search is above the last ply)
        OppFrame &P = f[k];
        if (SEL) {
            const u32 pad = (u32)uni(P.pad), child = pad & 3u;
            const int pe = (int)(signed char)(pad >> 8), pal = uni(P.alpha), pbe = uni(P.beta);
            const Board pb = uni_board(P.b);
            if (child == OPP_CHILD_NULL) {                     // r - 3 and the window (-beta, -beta + 1)
                b = opp_null_board(pb);
                a = -pbe; be = -pbe + 1;
                e = pe > 3 ? pe - 3 : 0;
            } else {
                const int cur = uni(P.cur);
                const u32 mv = (u32)uni((int)P.mv[cur]);
                const int pieces = popc(occupied(pb));
                b = apply_move(pb, mv);
                a = -pbe; be = -pal;
                e = pe - 1;                                // (a quiescence node: j + 1)
                // late-move reduction: the guards in the order of their price
                bool red = child != OPP_CHILD_AGAIN && pe >= 3 && !(pad & OPP_NODE_IN_CHECK) && cur >= 3;
                if (red) {
                    const u32 kl = (u32)uni((int)P.killers);   // (the root's pair stays NO_MOVE)
                    // tactical: below the root the tactical moves stand in front; at the root a legal move is tactical
                    // exactly if it promotes or a piece has left the board (en passant included), so no parent board
                    const bool tact = k > 0 ? cur < uni(P.nt) : ((mv >> 12) & 7u) != 0 || popc(occupied(b)) != pieces;
                    red = !tact && mv != (kl & 0xFFFFu) && mv != (kl >> 16) && !opp_in_check(b);
                }
                if (red) {                                     // r - 2 and the window (-alpha - 1, -alpha)
                    e = pe - 2;
                    a = -pal - 1; be = -pal;
                    __syncthreads();                           // the frame was read
                    if (lane == 0) P.pad = (int32_t)((pad & ~3u) | OPP_CHILD_REDUCED);
                    __syncthreads();
                }
            }
        } else {
            const u32 mv = (u32)uni((int)P.mv[uni(P.cur)]);
            b = apply_move(uni_board(P.b), mv);
            a = -uni(P.beta);
            be = -uni(P.alpha);
        }
        k++;
    }
    OppResult o;
    if (ID && !done && best_mv == NO_MOVE && depth_done > 0) {             // a cut iteration without a whole root move
        o.mv = held_mv;
        o.score = held_score;
    } else {
        o.mv = done || best_mv != NO_MOVE ? best_mv : first_mv;
        o.score = done ? v : root_best;
    }
    o.nodes = nodes;
    o.done = done;
    o.depth_done = depth_done;
    return o;
}

// One slot of k_opponent_moves / k_opponent_moves_q and, ID, of their _id forms.  Window-relative rows: depths / moves /
// scores / nodes_out / flags [count] and, ID only, depths_done [count]
template <bool QS, bool ID = false, bool ORD = false, bool REP = false, bool POS = false, bool SEL = false,
          bool EXC = false>
__device__ inline void opponent_moves_slot(Dev d, const int32_t *depths, int Q, int push, long long limit, u16 *moves,
                                           int32_t *scores, long long *nodes_out, uint8_t *flags, OppLds<QS> &s,
                                           int32_t *depths_done = nullptr, OppRepLds<QS> *rs = nullptr)
{
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    int D = uni(depths[r]);
    if (D > OPP_MAX_DEPTH) D = OPP_MAX_DEPTH;              // (the host refuses such a depth before the launch,
    if (Q > OPP_MAX_QUIESCENCE) Q = OPP_MAX_QUIESCENCE;    //  and such a Q)
    const bool skipped = D > 0 && uni(d.game[g].game_result) != RESULT_NONE;
    if (D <= 0 || skipped) {
        if (lane == 0) {
            moves[r] = NO_MOVE; scores[r] = 0; nodes_out[r] = 0; flags[r] = skipped ? OPP_SKIPPED : 0;
            if (ID) depths_done[r] = 0;
        }
        return;
    }
    const Board root = uni_board(d.cur[g]);
    OppRepRoot rr;                                         // REP: the root is the game's current position
    rr.d = &d; rr.g = g; rr.tp = 0; rr.ply = REP ? uni(d.game[g].ply) : 0;
    const OppResult o = opp_search<QS, ID, ORD, REP, POS, SEL, EXC>(root, D, Q, limit, s.f, lane, rs, rr);
    if (lane == 0) {
        moves[r] = (u16)o.mv;
        scores[r] = o.score;
        nodes_out[r] = o.nodes;
        flags[r] = o.done ? 0 : OPP_CUT;                   // (ID: done = the iteration to depth D finished)
        if (ID) depths_done[r] = o.depth_done;
    }
    if (push && o.mv != NO_MOVE) {
        __syncthreads();                                   // the frames are dead: s.w takes their bytes
        game_push(d, g, ORD || REP ? uni_board(d.cur[g]) : root, o.mv, lane, s.w);   // (not held across the search)
    }
}

__global__ __launch_bounds__(64) void k_opponent_moves(Dev d, const int32_t *depths, int push, long long limit,
                                                       u16 *moves, int32_t *scores, long long *nodes_out,
                                                       uint8_t *flags)
{
    __shared__ OppLds<false> s;
    opponent_moves_slot<false>(d, depths, 0, push, limit, moves, scores, nodes_out, flags, s);
}

// the same with Q = 1 .. OPP_MAX_QUIESCENCE quiescence plies
__global__ __launch_bounds__(64) void k_opponent_moves_q(Dev d, const int32_t *depths, int Q, int push, long long limit,
                                                         u16 *moves, int32_t *scores, long long *nodes_out,
                                                         uint8_t *flags)
{
    __shared__ OppLds<true> s;
    opponent_moves_slot<true>(d, depths, Q, push, limit, moves, scores, nodes_out, flags, s);
}

// ITERATIVE DEEPENING under the node budget: depths[] are maximum depths, depths_done [count] the completed ones.  One
// kernel template of its own for the 32 legal shapes (opp_shape_legal), so a launch without a budget runs the code it
// ran.  One argument list for all: Q is not read without QS, and the REPETITION arrays exist in LDS only with REP.
template <bool QS, bool ORD, bool REP, bool POS, bool SEL, bool EXC>
__global__ __launch_bounds__(64) void k_opponent_moves_id(Dev d, const int32_t *depths, int Q, int push,
                                                          long long budget, u16 *moves, int32_t *scores,
                                                          long long *nodes_out, uint8_t *flags, int32_t *depths_done)
{
    __shared__ OppLds<QS> s;
    OppRepLds<QS> *rs = nullptr;
    if constexpr (REP) {
        __shared__ OppRepLds<QS> rep;
        rs = &rep;
    }
    opponent_moves_slot<QS, true, ORD, REP, POS, SEL, EXC>(d, depths, QS ? Q : 0, push, budget, moves, scores,
                                                           nodes_out, flags, s, depths_done, rs);
}

// expand, the opponent's half (mctree.py:244-246) with the built-in opponent as the mover (gamestockfish.py:27-41):
// the reply stored for S1 is the move k_opponent_moves plays from S1 -- it reads the board alone, so the tree holds the
// real opponent's reply.  Rows as k_reply: one whose pending leaf is not LEAF_NEW_REPLY only clears lab_n2.  The root
// order of the search is wave_movegen's (s1_moves is not read).  A cut reply is a move like any other.  nodes_acc /
// cuts_acc [count], window-relative: this wave owns its row, so lane 0 adds with a plain load and store.  ID: the
// search is ITERATIVE DEEPENING under the budget `limit`, and depth_acc [count] sums the completed depths.
// REP: REPETITION -- S1 stands at tree ply 2 * path_len - 1 of the one path d.path_node holds, so what led to it is the
// S1 / S2 of the pending node's ancestors and then the game's ring.
template <bool QS, bool ID = false, bool ORD = false, bool REP = false, bool POS = false, bool SEL = false,
          bool EXC = false>
__device__ inline void reply_opponent_row(Dev d, const int32_t *depths, int Q, long long limit, void *planes2,
                                          unsigned long long *nodes_acc, uint32_t *cuts_acc, OppLds<QS> &s,
                                          unsigned long long *depth_acc = nullptr, OppRepLds<QS> *rs = nullptr)
{
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    if (lane == 0) d.lab_n2[r] = 0;                     // no policy(S2) wanted unless a new node gets priors
    if (d.game[g].root_dead || d.game[g].leaf_kind != LEAF_NEW_REPLY) return;
    const int D = uni(depths[r]);
    if (D < 1 || D > OPP_MAX_DEPTH || (QS && (Q < 1 || Q > OPP_MAX_QUIESCENCE))) {
        dev_error(d, DERR_STATE);                       // (the host never sends one)
        return;
    }
    const int c = uni(d.game[g].leaf_node);
    const Board s1 = uni_board(d.node[(size_t)g * d.N + c].s1);
    OppRepRoot rr;
    rr.d = &d; rr.g = g; rr.tp = REP ? 2 * uni(d.game[g].path_len) - 1 : 0; rr.ply = REP ? uni(d.game[g].ply) : 0;
    const OppResult o = opp_search<QS, ID, ORD, REP, POS, SEL, EXC>(s1, D, Q, limit, s.f, lane, rs, rr);
    if (o.mv == NO_MOVE) { dev_error(d, DERR_STATE); return; }              // S1 is running: it has a legal move
    if (lane == 0) {
        nodes_acc[r] += (unsigned long long)o.nodes;
        if (!o.done) cuts_acc[r] += 1u;
        if (ID) depth_acc[r] += (unsigned long long)o.depth_done;
    }
    __syncthreads();                                       // the frames are dead: s.w takes their bytes
    reply_tail(d, g, r, lane, s.w, c, uni(d.game[g].path_len), uni(d.game[g].ply), s1, o.mv,
               uni(d.game[g].edge_top), d.policy_fmt, &d.game[g].leaf_kind, planes2);
}

__global__ __launch_bounds__(64) void k_reply_opponent(Dev d, const int32_t *depths, long long limit, void *planes2,
                                                       unsigned long long *nodes_acc, uint32_t *cuts_acc)
{
    __shared__ OppLds<false> s;
    reply_opponent_row<false>(d, depths, 0, limit, planes2, nodes_acc, cuts_acc, s);
}

__global__ __launch_bounds__(64) void k_reply_opponent_q(Dev d, const int32_t *depths, int Q, long long limit,
                                                         void *planes2, unsigned long long *nodes_acc,
                                                         uint32_t *cuts_acc)
{
    __shared__ OppLds<true> s;
    reply_opponent_row<true>(d, depths, Q, limit, planes2, nodes_acc, cuts_acc, s);
}

// the budgeted reply: the 32 legal shapes as one kernel template with the argument list of k_opponent_moves_id's kind
template <bool QS, bool ORD, bool REP, bool POS, bool SEL, bool EXC>
__global__ __launch_bounds__(64) void k_reply_opponent_id(Dev d, const int32_t *depths, int Q, long long budget,
                                                          void *planes2, unsigned long long *nodes_acc,
                                                          uint32_t *cuts_acc, unsigned long long *depth_acc)
{
    __shared__ OppLds<QS> s;
    OppRepLds<QS> *rs = nullptr;
    if constexpr (REP) {
        __shared__ OppRepLds<QS> rep;
        rs = &rep;
    }
    reply_opponent_row<QS, true, ORD, REP, POS, SEL, EXC>(d, depths, QS ? Q : 0, budget, planes2, nodes_acc, cuts_acc,
                                                          s, depth_acc, rs);
}

// EXCHANGE, test 2 alone and no search: every legal move of every window slot's current position, in generation
// order.  bits [count][MAX_MOVES], window-relative: bit 0 = the move is tactical, bit 1 = it is kept (SEE >= 0; always
// set for a move that is not tactical; 0 from the slot's move count on); counts [count]: the legal moves of the slot.  Lane i judges move i, 64 per pass.
__global__ __launch_bounds__(64) void k_opponent_exchange(Dev d, uint8_t *bits, int32_t *counts)
{
    __shared__ u16 mv[MAX_MOVES];
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    const Board b = uni_board(d.cur[g]);
    const MoveGenInfo mi = wave_movegen(b, lane, mv);
    __syncthreads();
    int n = uni(mi.n);
    if (n > MAX_MOVES) n = MAX_MOVES;                      // (no position has more than MAX_BRANCH)
    const u64 occ = occupied(b);
    const u64 own = st_turn(b.state) ? b.white : (occ & ~b.white);
    for (int base = 0; base < MAX_MOVES; base += 64) {     // (the entries from n on: 0)
        const int i = base + lane;
        uint8_t out = 0;
        if (i < n) {
            const u32 m = mv[i];
            const bool tact = opp_tactical(b, occ, own, m);
            const bool keep = !tact || opp_see_not_negative(b, occ, m);
            out = (uint8_t)((tact ? 1 : 0) | (keep ? 2 : 0));
        }
        bits[(size_t)r * MAX_MOVES + i] = out;
    }
    if (lane == 0) counts[r] = n;
}

// the static evaluation of every window slot's current position: scores [count], window-relative
__global__ __launch_bounds__(64) void k_opponent_evaluate(Dev d, int positional, int32_t *scores)
{
    const int r = blockIdx.x, g = r + d.g0, lane = threadIdx.x;
    const Board b = uni_board(d.cur[g]);
    const int v = positional ? opp_evaluate_positional(b, lane) : opp_evaluate(b, lane);
    if (lane == 0) scores[r] = v;
}

}  // namespace crl
