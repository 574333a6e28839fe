"""CPU restatement of the built-in opponent's selective search -- null-move pruning and late-move reductions on top of
ORDERING (chessrl_amd/csrc/opponent.hpp, SELECTIVE) -- over ``oracle.chess_oracle.OracleGame``.

TEST INFRASTRUCTURE, written from the header comment of opponent.hpp alone; the evaluations, the results, the tactical
predicate, the victim classes and the check test are imported from ``tests/opponent_util.py``,
``tests/quiescence_util.py`` and ``tests/evaluation_util.py``.  The search loop is that of ``ordering_util.ordered`` /
``repetition_util.repeated`` with a remaining depth per node in place of the ply test, the null move and the reduced
search.  A null child is a game of its own that starts from the null board (side to move exchanged, no en-passant
square, halfmove clock 0), so neither its results nor ``OracleGame.repetitions()`` look across the null move.  Pure
Python integers:

  search         the rule as specified -> (move id, score, nodes, flag, depth_done); ``selective=False`` is the ordered
                 search without the section; ``counts`` (a dict) collects how often each branch of the rule was taken
  play_ply       the move a side with these settings plays, pushed
  ReplyAgentSel  ``opponent_reply_util.ReplyAgent`` whose real-game reply is ``search``; logs (reply, None, nodes,
                 flag, depth_done)
  HAND_MADE / games / CASES / reference    the set the GPU test runs, computed once
"""
import functools

from oracle.chess_oracle import OcBoard, OracleGame, board_from_fen, move_to_uci
from tests import evaluation_util
from tests import opponent_reply_util
from tests import ordering_util
from tests import repetition_util
from tests.opponent_util import CUT, INF, MATE, MAX_DEPTH, NO_MOVE, NODE_LIMIT, SKIPPED, child, tactical, terminal
from tests.quiescence_util import MAX_QUIESCENCE, in_check, victim_class

NULL_REDUCTION = 3                               # the null child has r - 3
NULL_MATE = 29000                                # no null move against such a beta; a cut from there on is capped
LMR_FROM = 3                                     # the first reduced position c, and the least r that reduces
BRANCHES = ("null_cut", "null_failed", "null_refused_in_check", "null_refused_no_piece", "null_refused_after_null",
            "null_refused_evaluation", "null_refused_mate_beta", "null_refused_depth", "null_cut_capped",
            "reduction_holds", "reduction_researched", "reduction_refused_tactical", "reduction_refused_killer",
            "reduction_refused_gives_check", "reduction_refused_early", "reduction_refused_depth",
            "reduction_refused_in_check", "reduction_at_root", "repetition_stops_at_null",
            "budget_cut_in_null_child", "budget_cut_in_reduced_search", "budget_cut_in_research")
UNREACHED = repetition_util.UNREACHED


def new_counts():
    return dict.fromkeys(BRANCHES, 0)


def clock(game):
    return (int(game.board_at(0).state) >> 12) & 255


def has_piece(game):
    """The side to move owns a knight, a bishop, a rook or a queen."""
    b = game.board_at(0)
    occ = 0
    for pt in range(6):
        occ |= int(b.bb[pt])
    own = int(b.white) & occ if int(b.state) & 1 else occ & ~int(b.white)
    return bool(own & (int(b.bb[1]) | int(b.bb[2]) | int(b.bb[3]) | int(b.bb[4])))


def null_child(game):
    """A game whose only position is ``game``'s current one after a null move."""
    b, n = game.board_at(0), OcBoard()
    for pt in range(6):
        n.bb[pt] = b.bb[pt]
    n.white = b.white
    st = int(b.state)
    n.state = ((st & 1) ^ 1) | (st & 0x1E) | (64 << 5)                     # turn, castling kept, no ep, clock 0
    return OracleGame(board=n)


class _Cut(Exception):
    pass


def search(game, max_depth, budget, quiescence=0, repetition=False, evaluation="material", selective=True,
           counts=None):
    """(move id, score, nodes, flag, depth_done) of the search of ``game``'s current position: depths 1 ..
    ``max_depth`` under ``budget`` nodes with ORDERING, with REPETITION and the EVALUATION asked for and,
    ``selective``, with SELECTIVE, as opponent.hpp states them."""
    assert 1 <= max_depth <= MAX_DEPTH and 0 <= quiescence <= MAX_QUIESCENCE and budget >= 1
    evaluate = evaluation_util.EVALUATIONS[evaluation]
    if game.get_result() is not None:
        return NO_MOVE, 0, 0, SKIPPED, 0
    st = {"nodes": 0, "best": (NO_MOVE, -INF), "first": NO_MOVE, "front": NO_MOVE}
    killers = dict((k, [NO_MOVE, NO_MOVE]) for k in range(0, max_depth + quiescence))   # (ply 0: never set)

    def count(what):
        if counts is not None:
            counts[what] += 1

    def nine_classes(g, k, moves):
        a, b = killers[k]
        cls = []
        for m in moves:
            c = victim_class(g, m)
            if c == 6:
                c = 6 if m == a else 7 if m == b else 8
            cls.append(c)
        return [m for c in range(9) for m, x in zip(moves, cls) if x == c], sum(1 for x in cls if x < 6)

    def count_null_guards(g, r, checked, after_null, beta):
        """Which single guard refused the null move (only with ``counts``)."""
        guards = {"null_refused_depth": r >= 2, "null_refused_in_check": not checked,
                  "null_refused_no_piece": has_piece(g), "null_refused_after_null": not after_null,
                  "null_refused_mate_beta": abs(beta) < NULL_MATE}
        failed = [name for name, ok in guards.items() if not ok]
        # A null child has r - 3 <= 1 at every depth up to 5 (r <= 4 below the root), so "reached by a null move" can
        # never be the ONLY guard that fails: it is counted where it and the depth are the only two.
        if failed == ["null_refused_depth", "null_refused_after_null"]:
            failed = ["null_refused_after_null"]
        if len(failed) > 1:
            return
        if evaluate(g) < beta:
            failed.append("null_refused_evaluation")
        if len(failed) == 1:
            count(failed[0])

    def count_reduction_guards(k, r, checked, c, is_tactical, is_killer, gives_check):
        guards = {"reduction_refused_depth": r >= LMR_FROM, "reduction_refused_in_check": not checked,
                  "reduction_refused_early": c >= LMR_FROM, "reduction_refused_tactical": not is_tactical,
                  "reduction_refused_killer": not is_killer, "reduction_refused_gives_check": not gives_check}
        failed = [name for name, ok in guards.items() if not ok]
        if len(failed) == 1:
            count(failed[0])

    def node(g, k, alpha, beta, r, j, after_null, below_null, run):
        """``r``: the remaining depth; ``j``: the quiescence ply of a node with r <= 0; ``after_null``: a null move led
        here; ``below_null``: one lies on the path; ``run``: the reversible plies behind the node if no null move had
        reset the clock (read by ``counts`` alone)."""
        if st["nodes"] >= budget:                                          # tested before every node
            raise _Cut()
        moves = g.legal_move_ids()
        st["nodes"] += 1
        over, mated = terminal(g, len(moves))
        if over:
            return -(MATE - k) if mated else 0
        if repetition and k >= 1:                                          # 3b
            if g.repetitions() >= 2:
                return 0
            if counts is not None and below_null and run >= 4 and run // 2 > clock(g) // 2:
                count("repetition_stops_at_null")                          # the distances past the null move: not read
        best = -INF
        n_tactical = None                                                  # of a node that may set a killer
        checked = in_check(g)
        if r > 0:
            if k > 0:
                moves, n_tactical = nine_classes(g, k, moves)
            else:
                st["first"] = moves[0]
                front = st["front"]
                if front != NO_MOVE:                                       # the stable move-to-front
                    moves = [front] + [m for m in moves if m != front]
        elif quiescence == 0 or j == quiescence:                           # the horizon; 4a
            if counts is not None and selective and k >= 1:
                count_null_guards(g, r, checked, after_null, beta)
            return evaluate(g)
        elif checked:                                                      # 4b: all nine classes
            moves, n_tactical = nine_classes(g, k, moves)
        else:                                                              # 4c: classes 0 .. 5 only
            best = evaluate(g)
            if best >= beta:
                return best
            alpha = max(alpha, best)
            cls = [victim_class(g, m) for m in moves]
            moves = [m for c in range(6) for m, x in zip(moves, cls) if x == c]
        # ---- the null move
        if selective and k >= 1:
            if r >= 2 and not checked and has_piece(g) and not after_null and abs(beta) < NULL_MATE \
                    and evaluate(g) >= beta:
                rc = r - NULL_REDUCTION
                try:
                    s = -node(null_child(g), k + 1, -beta, -beta + 1, rc, 0, True, True, run + 1)
                except _Cut:
                    count("budget_cut_in_null_child")
                    raise
                if s >= beta:
                    count("null_cut")
                    if s >= NULL_MATE:
                        count("null_cut_capped")
                        return beta
                    return s
                count("null_failed")
            elif counts is not None:
                count_null_guards(g, r, checked, after_null, beta)
        # ---- the moves
        for c, m in enumerate(moves):
            kid = child(g, m)
            kid_run = 0 if clock(kid) == 0 else run + 1
            full = (r - 1, 0) if r > 0 else (r - 1, j + 1)
            sc, researched = None, False
            if selective and (counts is not None or (r >= LMR_FROM and not checked and c >= LMR_FROM)):
                is_tactical, is_killer = tactical(g, m), m in killers[k]
                gives_check = in_check(kid)
                if r >= LMR_FROM and not checked and c >= LMR_FROM and not is_tactical and not is_killer \
                        and not gives_check:
                    if k == 0:
                        count("reduction_at_root")
                    try:
                        sc = -node(kid, k + 1, -alpha - 1, -alpha, r - 2, 0, False, below_null, kid_run)
                    except _Cut:
                        count("budget_cut_in_reduced_search")
                        raise
                    if sc > alpha:
                        count("reduction_researched")
                        sc, researched = None, True
                    else:
                        count("reduction_holds")
                elif counts is not None:
                    count_reduction_guards(k, r, checked, c, is_tactical, is_killer, gives_check)
            if sc is None:
                try:
                    sc = -node(kid, k + 1, -beta, -alpha, full[0], full[1], False, below_null, kid_run)
                except _Cut:
                    if researched:
                        count("budget_cut_in_research")
                    raise
            if sc > best:
                best = sc
                if k == 0:
                    st["best"] = (m, sc)
            alpha = max(alpha, sc)
            if alpha >= beta:
                if n_tactical is not None and c >= n_tactical and m != killers[k][0]:
                    pair = killers[k]
                    pair[1], pair[0] = pair[0], m
                break
        return best

    held, depth_done = (NO_MOVE, -INF), 0
    for i in range(1, max_depth + 1):
        st["best"], st["front"] = (NO_MOVE, -INF), held[0]
        try:
            score = node(game, 0, -INF, INF, i, 0, False, False, clock(game))
        except _Cut:
            if st["best"][0] != NO_MOVE:                                   # a root move of iteration i was completed
                return st["best"] + (st["nodes"], CUT, depth_done)
            if depth_done > 0:
                return held + (st["nodes"], CUT, depth_done)
            return st["first"], -INF, st["nodes"], CUT, 0
        held, depth_done = (st["best"][0], score), i
    return held + (st["nodes"], 0, depth_done)


def play_ply(game, max_depth, budget, quiescence=0, repetition=False, evaluation="material", selective=True):
    """The built-in player with these settings moves in ``game``; returns the move id (NO_MOVE on a finished game)."""
    m = search(game, max_depth, budget, quiescence, repetition, evaluation, selective)[0]
    if m != NO_MOVE:
        assert game.move(move_to_uci(m))
    return m


class ReplyAgentSel(opponent_reply_util.ReplyAgent):
    """``best_move(S1, real_game=True)`` is the built-in opponent's ordered selective move of maximum depth ``depth``
    under ``budget`` nodes; logs (reply, None, nodes, flag, depth_done)."""

    def __init__(self, net, depth, budget, quiescence=0, repetition=False, evaluation="material", selective=True, **kw):
        kw.setdefault("log_greedy", False)
        super().__init__(net, depth, NODE_LIMIT, **kw)
        self.settings = (budget, quiescence, repetition, evaluation, selective)

    def best_move(self, game, real_game=False, **kw):
        if not real_game:
            return super().best_move(game, real_game=False, **kw)
        m, _, nodes, flag, done = search(game, self.depth, *self.settings)
        assert m != NO_MOVE
        self.log.append((move_to_uci(m), None, nodes, flag, done))
        return move_to_uci(m)


# ---- hand-made roots for the branches the 19 roots of ``ordering_util.games()`` do not reach: name -> FEN
HAND_MADE = (
    # after e3e2 and a null move black can only promote, and Rxe1 mates inside quiescence: the null child is worth a
    # mate.  The cut needs beta at ply 1 between the stand-pat after e1=N and the evaluation after e3e2; the other root
    # move, e3xf2, searched first, leaves such a beta at D = 5, Q = 2 with the material evaluation (the pawn on f5 is
    # what lifts the evaluation after e3e2 over it): a null-move cut worth a mate, capped to beta (CAPPED_CASE)
    ("capped_cut", "4R3/8/8/5P2/7P/4pNK1/5P2/7k b - - 0 1"),
    # three knights against two pawns about to be blocked: killers that would have been reduced
    ("knights_and_pawns", "6Nk/4P3/6K1/8/8/p1p5/8/N1N5 b - - 0 1"),
    # kings and pawns: the side to move owns no piece
    ("pawns_only", "4k3/pp4pp/8/8/8/8/PP4PP/4K3 w - - 0 1"),
    # a mate in one at the root: every later root move is searched against a mate window, and black owns a rook
    ("mate_window", "6k1/5ppp/8/8/8/8/r4PPP/1R2R1K1 w - - 0 1"),
)


@functools.lru_cache(maxsize=None)
def hand_made_games():
    return tuple((name, OracleGame(board=board_from_fen(fen))) for name, fen in HAND_MADE)


@functools.lru_cache(maxsize=None)
def games():
    """[(name, OracleGame)]: the 19 games of ``ordering_util.games()``, the nine roots with a history of
    ``repetition_util.history_games()`` and the hand-made ones."""
    return tuple(repetition_util.games()) + hand_made_games()


BIG_ROOT = ordering_util.BIG_ROOT
# the roots of the deep cases: small enough for depths 4 and 5
SMALL = ("kpk", "kbkn", "clock_96", "kqk", "blocked", "stalemate_near", "knight_shuffle", "king_shuffle", "fen_0",
         "fen_1", "fen_2", "kqk_black", "kqk_white", "kqk_nohist", "capped_cut", "knights_and_pawns", "pawns_only", "mate_window")
# (maximum depth, quiescence, budget, repetition, evaluation) of the GPU test: D in {3, 4, 5}, every shape of kernel;
# depths 4 and 5 on SMALL only; CAPPED_CASE, whose budget lets ``capped_cut`` finish depth 5, on CAPPED_ROOTS only
CAPPED_CASE = (5, 2, 3000, False, "material")
CAPPED_ROOTS = ("capped_cut",)
CASES = ((3, 0, 250, False, "material"), (3, 2, 300, True, "positional"), (4, 0, 500, False, "positional"),
         (4, 2, 500, True, "material"), (5, 0, 700, True, "material"), (5, 2, 700, False, "positional"),
         (4, 0, 132, True, "positional"), (4, 2, 196, False, "material"), (5, 2, 150, True, "positional"), CAPPED_CASE)


def in_case(name, case):
    if tuple(case) == CAPPED_CASE:
        return name in CAPPED_ROOTS
    return name in SMALL if case[0] >= 4 else True


@functools.lru_cache(maxsize=None)
def reference(max_depth, quiescence, budget, repetition, evaluation):
    """(rows, counts): ``search`` of every game of the case (None for a root the case leaves out) and the branch
    counts, computed once and never changed."""
    counts = new_counts()
    case = (max_depth, quiescence, budget, repetition, evaluation)
    rows = tuple(search(g, max_depth, budget, quiescence, repetition, evaluation, counts=counts)
                 if in_case(name, case) else None for name, g in games())
    return rows, counts
