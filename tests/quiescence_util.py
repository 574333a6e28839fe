"""CPU restatement of the built-in opponent's quiescence search (chessrl_amd/csrc/opponent.hpp, QUIESCENCE) over
``oracle.chess_oracle.OracleGame``.

TEST INFRASTRUCTURE, written from the header comment of opponent.hpp alone; the fixed-depth part (evaluation, results,
the tactical predicate) is imported from ``tests/opponent_util.py``.  Pure Python integers:

  victim_class   the class of a move in a quiescence node that stands pat: 0 .. 4 the victim Q R B N P (en passant:
                 P), 5 a promotion that captures nothing, 6 not tactical
  alphabeta_q    the search as specified with Q quiescence plies -> (move id, score, nodes, flag); ``counts`` (a dict)
                 collects how often each branch of the rule was taken
  minimax_q      no pruning, generation order everywhere, the same stand-pat and move sets -> (move id, score)
  play_ply_q     the move a side of depth d and quiescence Q plays, pushed
  ReplyAgentQ    ``opponent_reply_util.ReplyAgent`` whose real-game reply is ``alphabeta_q``
  games / CASES / reference    the set the GPU test runs: 16 roots and three set-up positions, computed once
"""
import functools

from oracle.chess_oracle import lib as oracle_lib, move_to_uci
from tests import opponent_reply_util
from tests.opponent_util import CUT, INF, MATE, MAX_DEPTH, NO_MOVE, NODE_LIMIT, SKIPPED, child, evaluate, tactical, terminal

MAX_QUIESCENCE = 6
KNOWN_ANSWER = "4k3/8/3p4/4p3/8/8/4Q3/4K3 w - - 0 1"          # depth 1 without quiescence: Qxe5, d6xe5
EN_PASSANT = "4k3/8/8/8/3p4/8/4P3/4K3 w - - 0 1"              # depth 1: e2e4, then d4xe3 inside quiescence
PROMOTIONS = "1r2k3/P7/8/8/8/8/8/4K3 w - - 0 1"               # depth 2: a8 and axb8 promotions inside quiescence
FENS = (KNOWN_ANSWER, EN_PASSANT, PROMOTIONS)
BRANCHES = ("in_check", "stand_pat_cut", "no_tactical_move", "en_passant", "promotion_capture", "promotion_quiet",
            "last_ply", "all_victims")


# (depth, quiescence) of the GPU test; depth 3 on the small roots and the three set-up positions only
CASES = ((1, 1), (1, 2), (1, 6), (2, 1), (2, 4), (2, 6), (3, 2))
DEPTH3 = ("kpk", "kbkn", "clock_96", "kqk", "blocked", "stalemate_near", "knight_shuffle", "king_shuffle")
ENDGAMES = ("kpk", "kbkn", "clock_96", "back_rank_white", "back_rank_black", "stalemate_near", "kqk", "blocked")


@functools.lru_cache(maxsize=None)
def games():
    """[(name, OracleGame)]: ``rollout_util.private_roots()`` and then FENS."""
    from oracle.chess_oracle import OracleGame, board_from_fen
    from tests import rollout_util
    return tuple(rollout_util.private_roots()) + tuple(("fen_%d" % i, OracleGame(board=board_from_fen(f)))
                                                       for i, f in enumerate(FENS))


@functools.lru_cache(maxsize=None)
def reference(depth, quiescence):
    """(rows, counts): ``alphabeta_q`` of every game (None where depth 3 leaves it out) and the branch counts of the
    case, computed once and never changed."""
    counts = new_counts()
    rows = tuple(alphabeta_q(g, depth, quiescence, counts=counts)
                 if depth < 3 or name in DEPTH3 or name.startswith("fen_") else None for name, g in games())
    return rows, counts


def in_check(game):
    return bool(oracle_lib().og_in_check(game._h))


def _piece_at(game, sq):
    b = game.board_at(0)
    for pt in range(6):
        if (int(b.bb[pt]) >> sq) & 1:
            return pt
    return None


def victim_class(game, m):
    if not tactical(game, m):
        return 6
    to = (m >> 6) & 63
    victim = _piece_at(game, to)
    if victim is not None:                                   # P N B R Q = 0 .. 4 -> classes 4 .. 0
        assert victim <= 4
        return 4 - victim
    return 5 if (m >> 12) & 7 else 4                         # a promotion that captures nothing; en passant


def _quiescence_moves(game, moves, counts):
    """The moves a stand-pat node searches, in the device's order, and the bookkeeping of the branches seen."""
    cls = [victim_class(game, m) for m in moves]
    out = [m for c in range(6) for m, k in zip(moves, cls) if k == c]
    if counts is not None:
        for m, k in zip(moves, cls):
            promo = (m >> 12) & 7
            if k == 4 and _piece_at(game, (m >> 6) & 63) is None:
                counts["en_passant"] += 1
            if promo and k < 5:
                counts["promotion_capture"] += 1
            if k == 5:
                counts["promotion_quiet"] += 1
        if set(range(5)) <= set(cls):
            counts["all_victims"] += 1
        if not out:
            counts["no_tactical_move"] += 1
    return out


class _Cut(Exception):
    pass


def new_counts():
    return dict.fromkeys(BRANCHES, 0)


def alphabeta_q(game, depth, quiescence, node_limit=NODE_LIMIT, counts=None):
    """(move id, score, nodes, flag) of the search of ``game``'s current position with ``quiescence`` plies past
    ``depth``, as opponent.hpp states it."""
    assert 1 <= depth <= MAX_DEPTH and 0 <= quiescence <= MAX_QUIESCENCE and node_limit >= 1
    if game.get_result() is not None:
        return NO_MOVE, 0, 0, SKIPPED
    st = {"nodes": 0, "best": (NO_MOVE, -INF), "first": NO_MOVE}

    def count(what):
        if counts is not None:
            counts[what] += 1

    def node(g, k, alpha, beta):
        if st["nodes"] >= node_limit:
            raise _Cut()
        moves = g.legal_move_ids()
        st["nodes"] += 1
        over, mated = terminal(g, len(moves))
        if over:
            return -(MATE - k) if mated else 0
        best = -INF
        if quiescence == 0 or k < depth:
            if k == depth:
                return evaluate(g)
            if k > 0:
                moves = [m for m in moves if tactical(g, m)] + [m for m in moves if not tactical(g, m)]
            else:
                st["first"] = moves[0]
        elif k - depth == quiescence:                                      # 4a
            count("last_ply")
            return evaluate(g)
        elif in_check(g):                                                  # 4b
            count("in_check")
            moves = [m for m in moves if tactical(g, m)] + [m for m in moves if not tactical(g, m)]
        else:                                                              # 4c
            best = evaluate(g)
            if best >= beta:
                count("stand_pat_cut")
                return best
            alpha = max(alpha, best)
            moves = _quiescence_moves(g, moves, counts)
        for m in moves:
            sc = -node(child(g, m), k + 1, -beta, -alpha)
            if sc > best:
                best = sc
                if k == 0:
                    st["best"] = (m, sc)
            alpha = max(alpha, sc)
            if alpha >= beta:
                break
        return best

    try:
        score = node(game, 0, -INF, INF)
    except _Cut:
        m, sc = st["best"]
        return (m if m != NO_MOVE else st["first"]), sc, st["nodes"], CUT
    return st["best"][0], score, st["nodes"], 0


def minimax_q(game, depth, quiescence):
    """(move id, score): no window and no cut, generation order everywhere, the first maximum; a quiescence node that
    is not in check starts from its stand-pat score and searches its tactical moves only."""
    def node(g, k):
        moves = g.legal_move_ids()
        over, mated = terminal(g, len(moves))
        if over:
            return NO_MOVE, (-(MATE - k) if mated else 0)
        if k == depth + quiescence:
            return NO_MOVE, evaluate(g)
        best, bm = None, NO_MOVE
        if k >= depth and not in_check(g):
            best = evaluate(g)
            moves = [m for m in moves if tactical(g, m)]
        for m in moves:
            sc = -node(child(g, m), k + 1)[1]
            if best is None or sc > best:
                best, bm = sc, m
        return bm, best

    return node(game, 0)


def play_ply_q(game, depth, quiescence, node_limit=NODE_LIMIT):
    """The built-in player of ``depth`` and ``quiescence`` moves in ``game``; returns the move id (NO_MOVE on a
    finished game)."""
    m = alphabeta_q(game, depth, quiescence, node_limit)[0]
    if m != NO_MOVE:
        assert game.move(move_to_uci(m))
    return m


class ReplyAgentQ(opponent_reply_util.ReplyAgent):
    """``best_move(S1, real_game=True)`` is the built-in opponent's move of ``depth`` and ``quiescence`` under
    ``limit``."""

    def __init__(self, net, depth, quiescence, limit=NODE_LIMIT, **kw):
        kw.setdefault("log_greedy", False)
        super().__init__(net, depth, limit, **kw)
        self.quiescence = quiescence

    def best_move(self, game, real_game=False, **kw):
        if not real_game:
            return super().best_move(game, real_game=False, **kw)
        m, _, nodes, flag = alphabeta_q(game, self.depth, self.quiescence, self.limit)
        assert m != NO_MOVE
        self.log.append((move_to_uci(m), None, nodes, flag))
        return move_to_uci(m)
