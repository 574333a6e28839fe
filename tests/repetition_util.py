"""CPU restatement of the built-in opponent's repetition rule under a node budget (chessrl_amd/csrc/opponent.hpp,
REPETITION) over ``oracle.chess_oracle.OracleGame``.

TEST INFRASTRUCTURE, written from the header comment of opponent.hpp alone; the evaluation, the results, the tactical
predicate, the victim classes and the check test are imported from ``tests/opponent_util.py`` and
``tests/quiescence_util.py``.  The search loop is that of ``ordering_util.ordered`` / ``iterdeep_util.iterdeep`` with
step 3b: a node below the root whose game -- the root's move stack and the line that led to the node -- holds its
position a second time (``OracleGame.repetitions() >= 2``: the oracle scans the whole stack with ``same_key``) is worth
0.  Pure Python integers:

  repeated       the rule as specified -> (move id, score, nodes, flag, depth_done); ``counts`` (a dict) collects how
                 often each branch of the rule was taken
  play_ply       the move a side of maximum depth D, budget B and quiescence Q plays with the rule, pushed
  ReplyAgentRep  ``opponent_reply_util.ReplyAgent`` whose real-game reply is ``repeated``; logs (reply, None, nodes,
                 flag, depth_done)
  games / CASES / reference    the set the GPU test runs: the 19 games of ``ordering_util.games()`` and nine roots with
                 a history, computed once
"""
import functools

from oracle.chess_oracle import OracleGame, board_from_fen, move_to_uci
from tests import long_game_util
from tests import opponent_reply_util
from tests import ordering_util
from tests import rollout_util
from tests.opponent_util import CUT, INF, MATE, MAX_DEPTH, NO_MOVE, NODE_LIMIT, SKIPPED, child, evaluate, tactical, terminal
from tests.quiescence_util import MAX_QUIESCENCE, in_check, victim_class

BRANCHES = ("history_hit", "path_hit", "hit_at_horizon", "hit_at_inner_node", "hit_in_quiescence",
            "hit_ahead_of_stand_pat_cut", "ep_legal_is_no_hit", "result_ahead_of_hit")

UNREACHED = 100000                               # a budget no search of the set reaches (and below the node limit)
KQK = "7k/8/8/8/8/8/Q7/K7 w - - 0 1"
EP_LEGAL = "4k1n1/3p4/8/4P3/8/8/8/4K1N1 b - - 0 1"
EP_NONE = "4k1n1/3p4/8/8/4P3/8/8/4K1N1 b - - 0 1"
# the six cases of the issue's table: name -> (FEN or None for the start position, the moves that follow)
TABLE = (("kqk_black", KQK, ("a2b2", "h8g8", "b2a2")),
         ("start_knights", None, ("g1f3", "g8f6", "f3g1", "f6g8")),
         ("kqk_white", KQK, ("a2b2", "h8g8", "b2a2", "g8h8")),
         ("kqk_nohist", KQK, ()),
         ("ep_legal", EP_LEGAL, ("d7d5", "g1f3", "g8f6", "f3g1")),
         ("ep_none", EP_NONE, ("d7d5", "g1f3", "g8f6", "f3g1")))
FORCED_FIFTH = ["a1b1", "a8b8"] + ["b1a1", "b8c8", "a1b1", "c8b8"] * 3 + ["b1a1", "b8a8"]    # test_gpu_opponent's line
STRADDLE_L = (250, 255)
SMALL = ("kqk_black", "kqk_white", "kqk_nohist")    # the roots of the depth-4 case
# (maximum depth, quiescence, budget) of the GPU test, each with ordering off and on; depth 4 on SMALL only
CASES = ((2, 0, 63), (3, 0, 150), (3, 0, 600), (4, 0, 2000), (3, 2, 300), (3, 2, 600), (2, 0, UNREACHED))


def table_game(name):
    fen, moves = dict((n, (f, m)) for n, f, m in TABLE)[name]
    g = OracleGame() if fen is None else OracleGame(board=board_from_fen(fen))
    for u in moves:
        assert g.move(u), (name, u)
    return g


def forced_fifth_cut():
    """``test_gpu_opponent.forced_fifth_game`` cut four plies before its end (its end: two forced plies past the 16)."""
    g = OracleGame(board=board_from_fen(rollout_util.BLOCKED))
    for u in FORCED_FIFTH[:len(FORCED_FIFTH) + 2 - 4]:
        assert g.move(u), u
    assert g.get_result() is None
    return g


@functools.lru_cache(maxsize=None)
def history_games():
    """[(name, OracleGame)]: the nine roots with a history (``kqk_nohist`` has none: its hits are path hits)."""
    out = [(name, table_game(name)) for name, _, _ in TABLE]
    out.append(("forced_fifth_cut", forced_fifth_cut()))
    out += [("straddle_%d" % L, long_game_util.straddling_fivefold(L, cut=L + 10)) for L in STRADDLE_L]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def games():
    """[(name, OracleGame)]: the 19 games of ``ordering_util.games()``, then ``history_games()``."""
    return tuple(ordering_util.games()) + history_games()


def in_case(name, case):
    return name in SMALL if case[0] == 4 else True


def new_counts():
    return dict.fromkeys(BRANCHES, 0)


def clock(game):
    return (int(game.board_at(0).state) >> 12) & 255


def _key(b):
    """_transposition_key of an oracle board: the en-passant square only where a capture there is legal (bit 20)."""
    st = int(b.state)
    ep = (st >> 5) & 127 if (st >> 20) & 1 else 64
    return tuple(int(x) for x in b.bb) + (int(b.white), st & 1, (st >> 1) & 15, ep)


def _placement(b):
    st = int(b.state)
    return tuple(int(x) for x in b.bb) + (int(b.white), st & 1, (st >> 1) & 15)


class _Cut(Exception):
    pass


def repeated(game, max_depth, budget, quiescence=0, ordering=False, counts=None):
    """(move id, score, nodes, flag, depth_done) of the search of ``game``'s current position: depths 1 ..
    ``max_depth`` under ``budget`` nodes with REPETITION and, ``ordering``, with ORDERING, as opponent.hpp states
    them."""
    assert 1 <= max_depth <= MAX_DEPTH and 0 <= quiescence <= MAX_QUIESCENCE and budget >= 1
    if game.get_result() is not None:
        return NO_MOVE, 0, 0, SKIPPED, 0
    st = {"nodes": 0, "best": (NO_MOVE, -INF), "first": NO_MOVE, "front": NO_MOVE, "depth": 0}
    killers = dict((k, [NO_MOVE, NO_MOVE]) for k in range(1, max_depth + quiescence))
    root_len = len(game)

    def count(what):
        if counts is not None:
            counts[what] += 1

    def below_root_order(g, k, moves):
        """The moves of a node at ply k >= 1 that searches all of them, in order; -> (moves, tactical moves or None)."""
        if not ordering:
            return [m for m in moves if tactical(g, m)] + [m for m in moves if not tactical(g, m)], None
        a, b = killers[k]
        cls = []
        for m in moves:
            c = victim_class(g, m)
            if c == 6:
                c = 6 if m == a else 7 if m == b else 8
            cls.append(c)
        return [m for c in range(9) for m, x in zip(moves, cls) if x == c], sum(1 for x in cls if x < 6)

    def count_hit(g, k, beta):
        """Which branches a repeated node at ply k takes (only with ``counts``)."""
        key, back, on_path, behind = _key(g.board_at(0)), 4, False, False
        while back <= clock(g) and back <= len(g):
            if _key(g.board_at(back)) == key:
                if len(g) - back >= root_len:
                    on_path = True
                else:
                    behind = True
            back += 2
        assert on_path or behind                                       # within the reversible plies, at distance >= 4
        if on_path:
            count("path_hit")
        if behind:
            count("history_hit")
        depth = st["depth"]
        if k < depth:
            count("hit_at_inner_node")
        elif quiescence == 0 or k - depth == quiescence:
            count("hit_at_horizon")
        if quiescence and k >= depth:
            count("hit_in_quiescence")
            if k - depth < quiescence and not in_check(g) and evaluate(g) >= beta:
                count("hit_ahead_of_stand_pat_cut")

    def count_miss(g):
        """A node that is no repetition only because of the en-passant part of the key (only with ``counts``)."""
        here, back = g.board_at(0), 4
        while back <= clock(g) and back <= len(g):
            then = g.board_at(back)
            if _placement(then) == _placement(here) and _key(then) != _key(here):
                count("ep_legal_is_no_hit")
                return
            back += 2

    def node(g, k, alpha, beta):
        depth = st["depth"]
        if st["nodes"] >= budget:                                          # tested before every node
            raise _Cut()
        moves = g.legal_move_ids()
        st["nodes"] += 1
        over, mated = terminal(g, len(moves))
        if over:
            if counts is not None and k >= 1 and g.repetitions() >= 2:
                count("result_ahead_of_hit")
            return -(MATE - k) if mated else 0
        if k >= 1:                                                         # 3b
            if g.repetitions() >= 2:
                if counts is not None:
                    count_hit(g, k, beta)
                return 0
            if counts is not None:
                count_miss(g)
        best = -INF
        n_tactical = None                                                  # of a node that may set a killer
        if quiescence == 0 or k < depth:
            if k == depth:
                return evaluate(g)
            if k > 0:
                moves, n_tactical = below_root_order(g, k, moves)
            else:
                st["first"] = moves[0]
                front = st["front"]
                if front != NO_MOVE:                                       # the stable move-to-front
                    moves = [front] + [m for m in moves if m != front]
        elif k - depth == quiescence:                                      # 4a
            return evaluate(g)
        elif in_check(g):                                                  # 4b
            moves, n_tactical = below_root_order(g, k, moves)
        else:                                                              # 4c
            best = evaluate(g)
            if best >= beta:
                return best
            alpha = max(alpha, best)
            cls = [victim_class(g, m) for m in moves]
            moves = [m for c in range(6) for m, x in zip(moves, cls) if x == c]
        for i, m in enumerate(moves):
            sc = -node(child(g, m), k + 1, -beta, -alpha)
            if sc > best:
                best = sc
                if k == 0:
                    st["best"] = (m, sc)
            alpha = max(alpha, sc)
            if alpha >= beta:
                if n_tactical is not None and i >= n_tactical and m != killers[k][0]:
                    pair = killers[k]
                    pair[1], pair[0] = pair[0], m
                break
        return best

    held, depth_done = (NO_MOVE, -INF), 0
    for i in range(1, max_depth + 1):
        st["depth"], st["best"], st["front"] = i, (NO_MOVE, -INF), held[0]
        try:
            score = node(game, 0, -INF, INF)
        except _Cut:
            if st["best"][0] != NO_MOVE:                                   # a root move of iteration i was completed
                return st["best"] + (st["nodes"], CUT, depth_done)
            if depth_done > 0:
                return held + (st["nodes"], CUT, depth_done)
            return st["first"], -INF, st["nodes"], CUT, 0
        held, depth_done = (st["best"][0], score), i
    return held + (st["nodes"], 0, depth_done)


def play_ply(game, max_depth, budget, quiescence=0, ordering=False):
    """The built-in player of ``max_depth``, ``budget`` and ``quiescence`` with the repetition rule moves in ``game``;
    returns the move id (NO_MOVE on a finished game)."""
    m = repeated(game, max_depth, budget, quiescence, ordering)[0]
    if m != NO_MOVE:
        assert game.move(move_to_uci(m))
    return m


class ReplyAgentRep(opponent_reply_util.ReplyAgent):
    """``best_move(S1, real_game=True)`` is the built-in opponent's move of maximum depth ``depth`` and
    ``quiescence`` under ``budget`` nodes with the repetition rule (S1 carries the game and the tree path behind it)."""

    def __init__(self, net, depth, budget, quiescence=0, ordering=False, **kw):
        kw.setdefault("log_greedy", False)
        super().__init__(net, depth, NODE_LIMIT, **kw)
        self.budget, self.quiescence, self.ordering = budget, quiescence, ordering

    def best_move(self, game, real_game=False, **kw):
        if not real_game:
            return super().best_move(game, real_game=False, **kw)
        m, _, nodes, flag, done = repeated(game, self.depth, self.budget, self.quiescence, self.ordering)
        assert m != NO_MOVE
        self.log.append((move_to_uci(m), None, nodes, flag, done))
        return move_to_uci(m)


@functools.lru_cache(maxsize=None)
def reference(max_depth, quiescence, budget, ordering=False):
    """(rows, counts): ``repeated`` of every game of the case (None for a root the case leaves out) and the branch
    counts, computed once and never changed."""
    counts = new_counts()
    case = (max_depth, quiescence, budget)
    rows = tuple(repeated(g, max_depth, budget, quiescence, ordering, counts=counts) if in_case(name, case) else None
                 for name, g in games())
    return rows, counts


def fixed_depth(game, depth, rule, counts=None):
    """(move id, score, nodes) of the plain fixed-depth alpha-beta of ``opponent_util.alphabeta`` and, ``rule``, with
    step 3b on top: how the table of cases was first measured.  ``counts``: {"hits": n} is incremented per repeated node."""
    st = {"nodes": 0, "best": (NO_MOVE, -INF)}

    def node(g, k, alpha, beta):
        moves = g.legal_move_ids()
        st["nodes"] += 1
        over, mated = terminal(g, len(moves))
        if over:
            return -(MATE - k) if mated else 0
        if rule and k >= 1 and g.repetitions() >= 2:
            if counts is not None:
                counts["hits"] = counts.get("hits", 0) + 1
            return 0
        if k == depth:
            return evaluate(g)
        if k > 0:
            moves = [m for m in moves if tactical(g, m)] + [m for m in moves if not tactical(g, m)]
        best = -INF
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

    score = node(game, 0, -INF, INF)
    return st["best"][0], score, st["nodes"]
