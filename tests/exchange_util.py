"""CPU restatement of the built-in opponent's delta and exchange pruning in quiescence (chessrl_amd/csrc/opponent.hpp,
EXCHANGE) over ``oracle.chess_oracle.OracleGame``.

TEST INFRASTRUCTURE, written from the header comment of opponent.hpp alone; the evaluations, the results, the tactical
predicate, the victim classes, the check test, the null child and the guards of SELECTIVE are imported from
``tests/opponent_util.py``, ``tests/quiescence_util.py``, ``tests/evaluation_util.py`` and ``tests/selective_util.py``.
The search loop is that of ``selective_util.search`` with the filter behind the victim partition of 4c.  Pure Python
integers:

  attackers      the pieces of a colour that stand in an occupancy and attack a square in it -> [(type, square)]
  see            SEE(m) by the definition: the list of gains, minimax back
  see_not_negative   the alternating-bound form the kernel uses: one balance, one answer bit
  judge          (tactical, kept by the exchange test) of a move: what ``Context.opponent_exchange`` reports
  search         the rule as specified -> (move id, score, nodes, flag, depth_done); ``exchange=False`` is
                 ``selective_util.search``; ``counts`` (a dict) collects what the filter did
  play_ply / ReplyAgentExc / HAND_MADE / games / CASES / reference    as in the other restatements
"""
import functools

from oracle.chess_oracle import OracleGame, board_from_fen, move_to_uci
from tests import evaluation_util
from tests import opponent_reply_util
from tests import ordering_util
from tests import selective_util
from tests.opponent_util import CUT, INF, MATE, MAX_DEPTH, NO_MOVE, NODE_LIMIT, SKIPPED, child, tactical, terminal
from tests.quiescence_util import MAX_QUIESCENCE, in_check, victim_class
from tests.selective_util import LMR_FROM, NULL_MATE, NULL_REDUCTION, has_piece, null_child

VALUE = (100, 320, 330, 500, 900, 0)             # P N B R Q; a king's value is never read
MARGIN = 200
P, N, B, R, Q, K = range(6)
COUNTS = ("nodes_4c", "tactical_moves", "delta_removed", "exchange_removed", "promotion_spared_by_delta",
          "list_emptied", "in_check_unfiltered", "filtered_nodes")
KNIGHT_STEPS = evaluation_util.KNIGHT_STEPS
KING_STEPS = evaluation_util.KING_STEPS
DIAGONALS = evaluation_util.DIAGONALS
ORTHOGONALS = evaluation_util.ORTHOGONALS


def new_counts():
    return dict.fromkeys(COUNTS, 0)


def position(game):
    """([bitboard of P, N, B, R, Q, K], white mask, occupancy, white to move) of ``game``'s current position."""
    b = game.board_at(0)
    bbs = [int(b.bb[pt]) for pt in range(6)]
    occ = 0
    for x in bbs:
        occ |= x
    return bbs, int(b.white), occ, bool(int(b.state) & 1)


def _piece(bbs, sq):
    for pt in range(6):
        if (bbs[pt] >> sq) & 1:
            return pt
    return None


def attackers(bbs, white, sq, occ, by_white):
    """[(type, square)] of the pieces of the colour ``by_white`` that stand in ``occ`` and attack ``sq`` in ``occ``:
    sliders stop at the first piece of ``occ``."""
    f, r = sq & 7, sq >> 3
    found = []

    def look(s, types):
        if (occ >> s) & 1 and bool((white >> s) & 1) == by_white:
            pt = _piece(bbs, s)
            if pt in types:
                found.append((pt, s))

    for df in (-1, 1):                                     # a white pawn attacks from one rank below
        ff, rr = f + df, (r - 1 if by_white else r + 1)
        if 0 <= ff < 8 and 0 <= rr < 8:
            look(rr * 8 + ff, (P,))
    for steps, types in ((KNIGHT_STEPS, (N,)), (KING_STEPS, (K,))):
        for df, dr in steps:
            ff, rr = f + df, r + dr
            if 0 <= ff < 8 and 0 <= rr < 8:
                look(rr * 8 + ff, types)
    for lines, types in ((DIAGONALS, (B, Q)), (ORTHOGONALS, (R, Q))):
        for df, dr in lines:
            ff, rr = f + df, r + dr
            while 0 <= ff < 8 and 0 <= rr < 8:
                s = rr * 8 + ff
                if (occ >> s) & 1:
                    look(s, types)
                    break
                ff, rr = ff + df, rr + dr
    return found


def victim_value(game, m):
    """value(victim) of the tactical move ``m``: en passant P, a promotion onto an empty square 0."""
    bbs, _, occ, _ = position(game)
    to = (m >> 6) & 63
    if (occ >> to) & 1:
        return VALUE[_piece(bbs, to)]
    return 0 if (m >> 12) & 7 else VALUE[P]


def _start(game, m):
    """(bbs, white mask, destination, occupancy, gain[0], type on the destination, white moved) after ``m``."""
    bbs, white, occ, wtm = position(game)
    frm, to, promo = m & 63, (m >> 6) & 63, (m >> 12) & 7
    first = victim_value(game, m)
    if not (occ >> to) & 1 and not promo:                  # en passant: the captured pawn leaves the occupancy
        occ &= ~(1 << (to - 8 if wtm else to + 8))
    occ = (occ & ~(1 << frm)) | (1 << to)
    on = _piece(bbs, frm)
    if promo:
        on = promo - 1
        first += VALUE[on] - VALUE[P]
    return bbs, white, to, occ, first, on, wtm


def see(game, m):
    """SEE(m) by the definition, for a tactical move of ``game``'s current position."""
    assert tactical(game, m)
    bbs, white, to, occ, first, on, wtm = _start(game, m)
    gain = [first]
    side = not wtm
    while True:
        att = attackers(bbs, white, to, occ, side)
        if not att:
            break
        pt, sq = min(att)                                  # P, N, B, R, Q, K; the lowest square inside a type
        if pt == K and attackers(bbs, white, to, occ, not side):
            break                                          # the king may not capture: the sequence ends before it
        gain.append(VALUE[on] - gain[-1])
        occ &= ~(1 << sq)
        on = pt
        side = not side
        if pt == K:
            break                                          # a king's capture ends the sequence
    while len(gain) > 1:
        last = gain.pop()
        gain[-1] = -max(-gain[-1], last)
    return gain[0]


def see_not_negative(game, m):
    """Whether SEE(m) >= 0, by the form the kernel uses: one balance and one answer bit, no list."""
    assert tactical(game, m)
    bbs, white, to, occ, first, on, wtm = _start(game, m)
    balance = VALUE[on] - first
    if balance <= 0:
        return True
    answer, side = True, wtm
    while True:
        side = not side
        att = attackers(bbs, white, to, occ, side)
        if not att:
            break
        pt, sq = min(att)
        if pt == K:
            if not attackers(bbs, white, to, occ, not side):
                answer = not answer
            break
        answer = not answer
        occ &= ~(1 << sq)
        balance = VALUE[pt] - balance
        if balance < int(answer):
            break
    return answer


def judge(game, m):
    """(tactical, kept) of the legal move ``m``: what ``Context.opponent_exchange`` reports for it."""
    if not tactical(game, m):
        return False, True
    return True, see(game, m) >= 0


def filtered(game, moves, stand, alpha, counts=None):
    """The tactical moves ``moves`` of the stand-pat node ``game`` (in the order of the victim partition) that pass the
    two tests, in that order."""
    out, removed = [], 0
    for m in moves:
        hopeless = stand + victim_value(game, m) + MARGIN <= alpha
        if (m >> 12) & 7:
            if hopeless and counts is not None:
                counts["promotion_spared_by_delta"] += 1
        elif hopeless:
            if counts is not None:
                counts["delta_removed"] += 1
            removed += 1
            continue
        if see(game, m) < 0:
            if counts is not None:
                counts["exchange_removed"] += 1
            removed += 1
            continue
        out.append(m)
    if counts is not None:
        counts["nodes_4c"] += 1
        counts["tactical_moves"] += len(moves)
        counts["filtered_nodes"] += removed > 0
        counts["list_emptied"] += bool(moves) and not out
    return out


class _Cut(Exception):
    pass


def search(game, max_depth, budget, quiescence=1, repetition=False, evaluation="material", selective=False,
           exchange=True, counts=None):
    """(move id, score, nodes, flag, depth_done) of the search of ``game``'s current position: depths 1 ..
    ``max_depth`` under ``budget`` nodes with ORDERING, with REPETITION, the EVALUATION and SELECTIVE as asked for and,
    ``exchange``, with EXCHANGE, as opponent.hpp states them."""
    assert 1 <= max_depth <= MAX_DEPTH and 0 <= quiescence <= MAX_QUIESCENCE and budget >= 1
    assert quiescence >= 1 or not exchange
    evaluate = evaluation_util.EVALUATIONS[evaluation]
    if game.get_result() is not None:
        return NO_MOVE, 0, 0, SKIPPED, 0
    st = {"nodes": 0, "best": (NO_MOVE, -INF), "first": NO_MOVE, "front": NO_MOVE}
    killers = dict((k, [NO_MOVE, NO_MOVE]) for k in range(0, max_depth + quiescence))   # (ply 0: never set)

    def nine_classes(g, k, moves):
        a, b = killers[k]
        cls = []
        for m in moves:
            c = victim_class(g, m)
            if c == 6:
                c = 6 if m == a else 7 if m == b else 8
            cls.append(c)
        return [m for c in range(9) for m, x in zip(moves, cls) if x == c], sum(1 for x in cls if x < 6)

    def node(g, k, alpha, beta, r, j, after_null):
        if st["nodes"] >= budget:                                          # tested before every node
            raise _Cut()
        moves = g.legal_move_ids()
        st["nodes"] += 1
        over, mated = terminal(g, len(moves))
        if over:
            return -(MATE - k) if mated else 0
        if repetition and k >= 1 and g.repetitions() >= 2:                 # 3b
            return 0
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
            return evaluate(g)
        elif checked:                                                      # 4b: all nine classes, never filtered
            moves, n_tactical = nine_classes(g, k, moves)
            if counts is not None and exchange and any(see(g, m) < 0 for m in moves[:n_tactical]):
                counts["in_check_unfiltered"] += 1
        else:                                                              # 4c: classes 0 .. 5 only
            best = evaluate(g)
            if best >= beta:
                return best
            alpha = max(alpha, best)
            cls = [victim_class(g, m) for m in moves]
            moves = [m for c in range(6) for m, x in zip(moves, cls) if x == c]
            if exchange:
                moves = filtered(g, moves, best, alpha, counts)
        # ---- SELECTIVE: the null move
        if selective and k >= 1 and r >= 2 and not checked and has_piece(g) and not after_null \
                and abs(beta) < NULL_MATE and evaluate(g) >= beta:
            s = -node(null_child(g), k + 1, -beta, -beta + 1, r - NULL_REDUCTION, 0, True)
            if s >= beta:
                return beta if s >= NULL_MATE else s
        # ---- the moves
        for c, m in enumerate(moves):
            kid = child(g, m)
            full = (r - 1, 0) if r > 0 else (r - 1, j + 1)
            sc = None
            if selective and r >= LMR_FROM and not checked and c >= LMR_FROM and not tactical(g, m) \
                    and m not in killers[k] and not in_check(kid):
                sc = -node(kid, k + 1, -alpha - 1, -alpha, r - 2, 0, False)
                if sc > alpha:
                    sc = None
            if sc is None:
                sc = -node(kid, k + 1, -beta, -alpha, full[0], full[1], False)
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
            score = node(game, 0, -INF, INF, i, 0, False)
        except _Cut:
            if st["best"][0] != NO_MOVE:                                   # a root move of iteration i was completed
                return st["best"] + (st["nodes"], CUT, depth_done)
            if depth_done > 0:
                return held + (st["nodes"], CUT, depth_done)
            return st["first"], -INF, st["nodes"], CUT, 0
        held, depth_done = (st["best"][0], score), i
    return held + (st["nodes"], 0, depth_done)


def play_ply(game, max_depth, budget, quiescence=1, repetition=False, evaluation="material", selective=False,
             exchange=True):
    """The built-in player with these settings moves in ``game``; returns the move id (NO_MOVE on a finished game)."""
    m = search(game, max_depth, budget, quiescence, repetition, evaluation, selective, exchange)[0]
    if m != NO_MOVE:
        assert game.move(move_to_uci(m))
    return m


class ReplyAgentExc(opponent_reply_util.ReplyAgent):
    """``best_move(S1, real_game=True)`` is the built-in opponent's ordered move of maximum depth ``depth`` under
    ``budget`` nodes with these settings; logs (reply, None, nodes, flag, depth_done)."""

    def __init__(self, net, depth, budget, quiescence=1, repetition=False, evaluation="material", selective=False,
                 exchange=True, **kw):
        kw.setdefault("log_greedy", False)
        super().__init__(net, depth, NODE_LIMIT, **kw)
        self.settings = (budget, quiescence, repetition, evaluation, selective, exchange)

    def best_move(self, game, real_game=False, **kw):
        if not real_game:
            return super().best_move(game, real_game=False, **kw)
        m, _, nodes, flag, done = search(game, self.depth, *self.settings)
        assert m != NO_MOVE
        self.log.append((move_to_uci(m), None, nodes, flag, done))
        return move_to_uci(m)


# ---- hand-made positions: name -> (FEN, the move judged, SEE worked out by hand in tests/test_exchange_cpu.py)
HAND_MADE = (
    ("rook_takes_loose_pawn", "4k3/8/8/3p4/8/8/8/3RK3 w - - 0 1", "d1d5", 100),
    ("xrays_both_sides", "q5k1/1b6/5n2/3p4/8/2N2B2/8/6KQ w - - 0 1", "c3d5", -220),
    ("en_passant_opens_the_file", "4k3/2p5/8/3pP3/8/8/8/3RK3 w - d6 0 1", "e5d6", 100),
    ("promotions", "1r2k3/P7/8/8/8/8/8/4K3 w - - 0 1", "a7b8q", 1300),
    ("king_may_capture", "8/8/4k3/3p4/8/8/8/3RK3 w - - 0 1", "d1d5", -400),
    ("king_may_not_capture", "8/8/4k3/3p4/8/8/6B1/3RK3 w - - 0 1", "d1d5", 100),
)
QUIET_PROMOTION = ("promotions", "a7a8q", -100)
MIDDLEGAME_FEN = "r2q1rk1/pp2bppp/2n1bn2/3p4/3P4/2NBPN2/PP3PPP/R1BQ1RK1 w - - 0 10"
TACTICAL_FEN = "r1bq1rk1/ppp2ppp/2n2n2/2bpp3/2B1P3/2NP1N2/PPP2PPP/R1BQ1RK1 w - - 0 7"


def from_fen(fen):
    return OracleGame(board=board_from_fen(fen))


@functools.lru_cache(maxsize=None)
def hand_made_games():
    return tuple((name, from_fen(fen)) for name, fen, _, _ in HAND_MADE)


BIG_ROOT = ordering_util.BIG_ROOT                # 218 legal moves: four passes of the exchange kernel
ROOTS_FROM_THE_SET = ("fen_0", "fen_1", "capped_cut")


@functools.lru_cache(maxsize=None)
def games():
    """[(name, OracleGame)]: the roots of the GPU test -- the hand-made positions, two middlegames and a few roots of
    ``selective_util.games()``."""
    named = dict(selective_util.games())
    return (hand_made_games() + (("middlegame", from_fen(MIDDLEGAME_FEN)), ("tactical", from_fen(TACTICAL_FEN))) +
            tuple((n, named[n]) for n in ROOTS_FROM_THE_SET))


UNREACHED = 3000
# (maximum depth, quiescence, budget, repetition, evaluation, selective) of the GPU test: every kernel shape
CASES = ((2, 1, UNREACHED, False, "material", False), (3, 2, 600, True, "material", False),
         (3, 4, 900, False, "positional", False), (2, 2, UNREACHED, True, "positional", False),
         (4, 2, 800, False, "material", True), (3, 1, 300, True, "material", True),
         (4, 4, 1000, False, "positional", True), (3, 2, 150, True, "positional", True))


@functools.lru_cache(maxsize=None)
def reference(max_depth, quiescence, budget, repetition, evaluation, selective, exchange=True):
    """(rows, counts, counts per root): ``search`` of every game of the set and what the filter did, in all and root
    by root, computed once and never changed."""
    per_root = tuple(new_counts() for _ in games())
    rows = tuple(search(g, max_depth, budget, quiescence, repetition, evaluation, selective, exchange, counts=c)
                 for (_, g), c in zip(games(), per_root))
    counts = dict((k, sum(c[k] for c in per_root)) for k in COUNTS)
    return rows, counts, per_root


@functools.lru_cache(maxsize=None)
def random_positions(n_games=12, plies=40, seed=11):
    """Every position of ``n_games`` games of up to ``plies`` random plies from the standard position (the opening
    included), each a game of its own; the first plies of a game are its own so that the games differ early."""
    import random
    rng = random.Random(seed)
    out = []
    for _ in range(n_games):
        g = OracleGame()
        for _ in range(plies):
            if g.get_result() is not None:
                break
            out.append(g.get_copy())
            assert g.move(move_to_uci(rng.choice(g.legal_move_ids())))
    return tuple(out)
