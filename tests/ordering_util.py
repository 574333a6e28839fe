"""CPU restatement of the built-in opponent's move ordering under a node budget (chessrl_amd/csrc/opponent.hpp,
ORDERING) over ``oracle.chess_oracle.OracleGame``.

TEST INFRASTRUCTURE, written from the header comment of opponent.hpp alone; the evaluation, the results, the tactical
predicate, the victim classes and the check test are imported from ``tests/opponent_util.py`` and
``tests/quiescence_util.py``.  Pure Python integers:

  ordered        the rule as specified -> (move id, score, nodes, flag, depth_done); ``counts`` (a dict) collects how
                 often each branch of the rule was taken
  play_ply       the move a side of maximum depth D, budget B and quiescence Q plays with ordering, pushed
  ReplyAgentOrd  ``opponent_reply_util.ReplyAgent`` whose real-game reply is ``ordered``; logs (reply, None, nodes,
                 flag, depth_done)
  games / CASES / reference    the set the GPU test runs: the 19 games of ``iterdeep_util.games()``, computed once
"""
import functools

from oracle.chess_oracle import move_to_uci
from tests import iterdeep_util
from tests import opponent_reply_util
from tests.opponent_util import CUT, INF, MATE, MAX_DEPTH, NO_MOVE, NODE_LIMIT, SKIPPED, child, evaluate, tactical, terminal
from tests.quiescence_util import MAX_QUIESCENCE, in_check, victim_class

BRANCHES = ("killer_set", "killer_shifts_a_to_b", "killer_a_ahead_of_a_quiet_move", "killer_b_ahead_of_a_quiet_move",
            "killer_absent", "killer_set_in_check_quiescence", "tactical_cut_sets_nothing", "same_killer_again",
            "victims_reordered")

UNREACHED = 100000                               # a budget no search of the set reaches (and below the node limit)
BIG_ROOT = "218_moves"                           # the root whose depth-3 search alone is 7 613 nodes
# (maximum depth, quiescence, budget) of the GPU test, on all 19 games; the last on the 18 other than BIG_ROOT.
CASES = ((2, 0, 1), (2, 0, 63), (2, 0, 200), (3, 0, 150), (3, 0, 600), (3, 2, 300), (3, 2, 600), (3, 0, UNREACHED))


def games():
    """[(name, OracleGame)]: ``iterdeep_util.games()``, the 16 private roots and then the three set-up positions."""
    return iterdeep_util.games()


def in_case(name, case):
    return not (case[2] == UNREACHED and name == BIG_ROOT)


def new_counts():
    return dict.fromkeys(BRANCHES, 0)


class _Cut(Exception):
    pass


def ordered(game, max_depth, budget, quiescence=0, counts=None):
    """(move id, score, nodes, flag, depth_done) of the search of ``game``'s current position: depths 1 ..
    ``max_depth`` under ``budget`` nodes with ORDERING, as opponent.hpp states it."""
    assert 1 <= max_depth <= MAX_DEPTH and 0 <= quiescence <= MAX_QUIESCENCE and budget >= 1
    if game.get_result() is not None:
        return NO_MOVE, 0, 0, SKIPPED, 0
    st = {"nodes": 0, "best": (NO_MOVE, -INF), "first": NO_MOVE, "front": NO_MOVE, "depth": 0}
    # one pair (A, B) per ply 1 .. D + Q - 1, NO_MOVE when the search starts, kept across the iterations
    killers = dict((k, [NO_MOVE, NO_MOVE]) for k in range(1, max_depth + quiescence))

    def count(what):
        if counts is not None:
            counts[what] += 1

    def nine_classes(g, k, moves):
        """The moves of a node at ply k >= 1 that searches all of them, in order; -> (moves, tactical moves)."""
        a, b = killers[k]
        cls = []
        for m in moves:
            c = victim_class(g, m)
            if c == 6:
                c = 6 if m == a else 7 if m == b else 8
            cls.append(c)
        out = [m for c in range(9) for m, x in zip(moves, cls) if x == c]
        if counts is not None:
            if a != NO_MOVE and a not in moves:
                count("killer_absent")
            for klass, name in ((6, "killer_a_ahead_of_a_quiet_move"), (7, "killer_b_ahead_of_a_quiet_move")):
                if klass in cls and 8 in cls[:cls.index(klass)]:
                    count(name)
            tact = [m for m, x in zip(moves, cls) if x < 6]
            if tact != out[:len(tact)]:
                count("victims_reordered")
        return out, sum(1 for x in cls if x < 6)

    def node(g, k, alpha, beta):
        depth = st["depth"]
        if st["nodes"] >= budget:                                          # tested before every node
            raise _Cut()
        moves = g.legal_move_ids()
        st["nodes"] += 1
        over, mated = terminal(g, len(moves))
        if over:
            return -(MATE - k) if mated else 0
        best = -INF
        n_tactical = None                                                  # of a node that may set a killer
        check_evasion = False
        if quiescence == 0 or k < depth:
            if k == depth:
                return evaluate(g)
            if k > 0:
                moves, n_tactical = nine_classes(g, k, moves)
            else:
                st["first"] = moves[0]
                front = st["front"]
                if front != NO_MOVE:                                       # the stable move-to-front
                    moves = [front] + [m for m in moves if m != front]
        elif k - depth == quiescence:                                      # 4a
            return evaluate(g)
        elif in_check(g):                                                  # 4b: all nine classes
            moves, n_tactical = nine_classes(g, k, moves)
            check_evasion = True
        else:                                                              # 4c: classes 0 .. 5 only, as without ORDERING
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
                if n_tactical is not None:                                 # (k >= 1, not a stand-pat node)
                    pair = killers[k]
                    if i < n_tactical:
                        assert tactical(g, m)
                        count("tactical_cut_sets_nothing")
                    elif m == pair[0]:
                        count("same_killer_again")
                    else:
                        assert not tactical(g, m)
                        count("killer_set")
                        if pair[0] != NO_MOVE:
                            count("killer_shifts_a_to_b")
                        if check_evasion:
                            count("killer_set_in_check_quiescence")
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


def play_ply(game, max_depth, budget, quiescence=0):
    """The built-in player of ``max_depth``, ``budget`` and ``quiescence`` with ordering moves in ``game``; returns
    the move id (NO_MOVE on a finished game)."""
    m = ordered(game, max_depth, budget, quiescence)[0]
    if m != NO_MOVE:
        assert game.move(move_to_uci(m))
    return m


class ReplyAgentOrd(opponent_reply_util.ReplyAgent):
    """``best_move(S1, real_game=True)`` is the built-in opponent's move of maximum depth ``depth`` and
    ``quiescence`` under ``budget`` nodes with ordering."""

    def __init__(self, net, depth, budget, quiescence=0, **kw):
        kw.setdefault("log_greedy", False)
        super().__init__(net, depth, NODE_LIMIT, **kw)
        self.budget, self.quiescence = budget, quiescence

    def best_move(self, game, real_game=False, **kw):
        if not real_game:
            return super().best_move(game, real_game=False, **kw)
        m, _, nodes, flag, done = ordered(game, self.depth, self.budget, self.quiescence)
        assert m != NO_MOVE
        self.log.append((move_to_uci(m), None, nodes, flag, done))
        return move_to_uci(m)


@functools.lru_cache(maxsize=None)
def reference(max_depth, quiescence, budget):
    """(rows, counts): ``ordered`` of every game of the case (None for the root the case leaves out) and the branch
    counts, computed once and never changed."""
    counts = new_counts()
    case = (max_depth, quiescence, budget)
    rows = tuple(ordered(g, max_depth, budget, quiescence, counts=counts) if in_case(name, case) else None
                 for name, g in games())
    return rows, counts
