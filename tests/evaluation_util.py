"""CPU restatement of the built-in opponent's positional evaluation (chessrl_amd/csrc/opponent.hpp, EVALUATION) over
``oracle.chess_oracle.OracleGame``.

TEST INFRASTRUCTURE, written from the header comment of opponent.hpp alone, square by square in plain Python integers
(no bitboard fills: the kernel's fills are what this checks).  The searches are NOT restated again: ``using`` rebinds
the module-level name ``evaluate`` of ``quiescence_util``, ``iterdeep_util``, ``ordering_util`` and ``repetition_util``
for the duration of a call, so their search loops run with the evaluation asked for.

  terms          every term of the table that applies in a position: [(row name, MG, EG)] signed for white
  sums           (MG, EG, ph) with the bishop pair, before the taper
  positional     the score, like ``opponent_util.evaluate`` over ``board_at(0)``
  EVALUATIONS    name -> function, "material" being ``opponent_util.evaluate``
  using          the context manager
  search         (move id, score, nodes, flag, depth_done) of the budgeted search with an evaluation
  play_ply, ReplyAgentEv
  flip_game / flip_fen    the colour flip of a position
  SETUPS / setup_games / games / CASES / reference    the sets the GPU test runs, computed once
"""
import contextlib
import functools

from oracle.chess_oracle import OcBoard, OracleGame, board_from_fen, move_to_uci
from tests import iterdeep_util
from tests import opponent_reply_util
from tests import opponent_util
from tests import ordering_util
from tests import quiescence_util
from tests import repetition_util
from tests.opponent_util import NO_MOVE, NODE_LIMIT, ring

P, N, B, R, Q, K = range(6)
MATERIAL = (100, 320, 330, 500, 900, 0)
PASSED_MG = (0, 5, 10, 20, 40, 70)
PASSED_EG = (0, 10, 20, 40, 80, 140)
KING_ATTACK = {N: 8, B: 8, R: 12, Q: 20}
TEMPO = 10
BOUND = 14528                                   # the header's bound on |score|
# every row of the header's table (and the per-side term): what ``terms`` can name
ROWS = ("pawn material", "pawn advancement", "pawn passed", "pawn doubled", "pawn isolated",
        "knight material", "knight position", "knight mobility", "bishop material", "bishop position",
        "bishop mobility", "rook material", "rook mobility", "rook open file", "rook half-open file", "rook seventh",
        "queen material", "queen position", "queen mobility", "king position", "king shelter",
        "knight king attack", "bishop king attack", "rook king attack", "queen king attack", "bishop pair")
NAMES = ("pawn", "knight", "bishop", "rook", "queen", "king")


class Position:
    """The squares of a board: ``piece[sq]`` = (type, is white) or None."""

    def __init__(self, board):
        self.piece = [None] * 64
        for pt in range(6):
            bb = int(board.bb[pt])
            for sq in range(64):
                if (bb >> sq) & 1:
                    self.piece[sq] = (pt, bool((int(board.white) >> sq) & 1))
        self.white_to_move = bool(int(board.state) & 1)

    def squares(self, pt, white):
        return [sq for sq in range(64) if self.piece[sq] == (pt, white)]

    def pawn_attacked(self, by_white):
        """PA: the squares the pawns of a colour attack."""
        out = set()
        for sq in self.squares(P, by_white):
            f, r = sq & 7, (sq >> 3) + (1 if by_white else -1)
            for ff in (f - 1, f + 1):
                if 0 <= ff <= 7 and 0 <= r <= 7:
                    out.add(r * 8 + ff)
        return out

    def steps(self, sq, deltas):
        f, r = sq & 7, sq >> 3
        return set((r + dr) * 8 + f + df for df, dr in deltas if 0 <= f + df <= 7 and 0 <= r + dr <= 7)

    def slides(self, sq, directions):
        """Along each direction up to and including the first piece of either colour."""
        out = set()
        for df, dr in directions:
            f, r = (sq & 7) + df, (sq >> 3) + dr
            while 0 <= f <= 7 and 0 <= r <= 7:
                out.add(r * 8 + f)
                if self.piece[r * 8 + f] is not None:
                    break
                f, r = f + df, r + dr
        return out

    def zone(self, white):
        out = set()
        for sq in self.squares(K, white):
            out |= self.steps(sq, KING_STEPS) | {sq}
        return out


KING_STEPS = [(df, dr) for df in (-1, 0, 1) for dr in (-1, 0, 1) if (df, dr) != (0, 0)]
KNIGHT_STEPS = [(1, 2), (2, 1), (2, -1), (1, -2), (-1, -2), (-2, -1), (-2, 1), (-1, 2)]
DIAGONALS = [(1, 1), (1, -1), (-1, 1), (-1, -1)]
ORTHOGONALS = [(1, 0), (-1, 0), (0, 1), (0, -1)]


def terms(game):
    """[(row, MG, EG)]: every term that applies, signed (a white piece adds, a black piece subtracts)."""
    pos = Position(game.board_at(0))
    out = []
    for sq in range(64):
        if pos.piece[sq] is None:
            continue
        pt, white = pos.piece[sq]
        sign = 1 if white else -1
        f, r = sq & 7, sq >> 3
        rel = r if white else 7 - r
        own = set(s for s in range(64) if pos.piece[s] is not None and pos.piece[s][1] == white)
        pa_enemy = pos.pawn_attacked(not white)
        zone_enemy = pos.zone(not white)

        def add(row, mg, eg):
            out.append((NAMES[pt] + " " + row, sign * mg, sign * eg))

        if pt != K:
            add("material", MATERIAL[pt], MATERIAL[pt])
        if pt == P:
            adv = rel - 1
            add("advancement", 5 * ring(sq) + 6 * adv, 12 * adv)
            ahead = [rr for rr in range(8) if (rr > r if white else rr < r)]
            own_pawns, enemy_pawns = pos.squares(P, white), pos.squares(P, not white)
            if not any(abs((s & 7) - f) <= 1 and (s >> 3) in ahead for s in enemy_pawns):
                add("passed", PASSED_MG[adv], PASSED_EG[adv])
            if any((s & 7) == f and (s >> 3) in ahead for s in own_pawns):
                add("doubled", -10, -20)
            if not any(abs((s & 7) - f) == 1 for s in own_pawns):
                add("isolated", -10, -15)
            continue
        if pt == K:
            add("position", -10 * ring(sq), 10 * ring(sq))
            if rel <= 1:
                step = 1 if white else -1
                n = sum(1 for s in pos.squares(P, white)
                        if abs((s & 7) - f) <= 1 and (s >> 3) in (r + step, r + 2 * step))
                add("shelter", 8 * n, 0)
            continue
        if pt == N:
            attack = pos.steps(sq, KNIGHT_STEPS)
            m = len(attack - own - pa_enemy)
            add("position", 10 * ring(sq), 10 * ring(sq))
            add("mobility", 4 * m, 4 * m)
        elif pt == B:
            attack = pos.slides(sq, DIAGONALS)
            m = len(attack - own - pa_enemy)
            add("position", 5 * ring(sq), 5 * ring(sq))
            add("mobility", 4 * m, 4 * m)
        elif pt == R:
            attack = pos.slides(sq, ORTHOGONALS)
            m = len(attack - own)
            add("mobility", 2 * m, 4 * m)
            own_on_file = any((s & 7) == f for s in pos.squares(P, white))
            enemy_on_file = any((s & 7) == f for s in pos.squares(P, not white))
            if not own_on_file and not enemy_on_file:
                add("open file", 20, 10)
            elif not own_on_file:
                add("half-open file", 10, 5)
            if rel == 6:
                add("seventh", 10, 20)
        else:
            attack = pos.slides(sq, DIAGONALS + ORTHOGONALS)
            m = len(attack - own - pa_enemy)
            add("position", 2 * ring(sq), 2 * ring(sq))
            add("mobility", m, 2 * m)
        if attack & zone_enemy:
            add("king attack", KING_ATTACK[pt], 0)
    for white in (True, False):
        if len(pos.squares(B, white)) >= 2:
            out.append(("bishop pair", 30 if white else -30, 40 if white else -40))
    assert all(row in ROWS for row, _, _ in out), [row for row, _, _ in out if row not in ROWS]
    return out


def phase(game):
    pos = Position(game.board_at(0))
    count = lambda pt: len(pos.squares(pt, True)) + len(pos.squares(pt, False))
    return min(24, count(N) + count(B) + 2 * count(R) + 4 * count(Q))


def sums(game):
    """(MG, EG, ph)."""
    t = terms(game)
    return sum(mg for _, mg, _ in t), sum(eg for _, _, eg in t), phase(game)


def trunc_div(a, b):
    """a / b truncating toward zero (b > 0)."""
    return a // b if a >= 0 else -((-a) // b)


def positional(game):
    mg, eg, ph = sums(game)
    white = trunc_div(mg * ph + eg * (24 - ph), 24)
    return (white if int(game.board_at(0).state) & 1 else -white) + TEMPO


EVALUATIONS = {"material": opponent_util.evaluate, "positional": positional}
_SEARCH_MODULES = (quiescence_util, iterdeep_util, ordering_util, repetition_util)


@contextlib.contextmanager
def using(evaluation):
    """Inside, the search restatements read ``EVALUATIONS[evaluation]`` where they read ``evaluate``."""
    fn = EVALUATIONS[evaluation]
    saved = [m.evaluate for m in _SEARCH_MODULES]
    for m in _SEARCH_MODULES:
        m.evaluate = fn
    try:
        yield
    finally:
        for m, old in zip(_SEARCH_MODULES, saved):
            m.evaluate = old


def search(game, max_depth, budget, quiescence=0, ordering=False, repetition=False, evaluation="positional"):
    """(move id, score, nodes, flag, depth_done) of the budgeted search with the evaluation, through the restatement of
    the rule set asked for."""
    with using(evaluation):
        if repetition:
            return repetition_util.repeated(game, max_depth, budget, quiescence, ordering)
        if ordering:
            return ordering_util.ordered(game, max_depth, budget, quiescence)
        return iterdeep_util.iterdeep(game, max_depth, budget, quiescence)


def play_ply(game, max_depth, budget, quiescence=0, ordering=False, repetition=False, evaluation="positional"):
    """The built-in player with these settings moves in ``game``; returns the move id (NO_MOVE on a finished game)."""
    m = search(game, max_depth, budget, quiescence, ordering, repetition, evaluation)[0]
    if m != NO_MOVE:
        assert game.move(move_to_uci(m))
    return m


class ReplyAgentEv(opponent_reply_util.ReplyAgent):
    """``best_move(S1, real_game=True)`` is the built-in opponent's move of maximum depth ``depth`` under ``budget``
    nodes with the evaluation; logs (reply, None, nodes, flag, depth_done)."""

    def __init__(self, net, depth, budget, quiescence=0, ordering=False, repetition=False, evaluation="positional", **kw):
        kw.setdefault("log_greedy", False)
        super().__init__(net, depth, NODE_LIMIT, **kw)
        self.settings = (budget, quiescence, ordering, repetition, evaluation)

    def best_move(self, game, real_game=False, **kw):
        if not real_game:
            return super().best_move(game, real_game=False, **kw)
        m, _, nodes, flag, done = search(game, self.depth, *self.settings)
        assert m != NO_MOVE
        self.log.append((move_to_uci(m), None, nodes, flag, done))
        return move_to_uci(m)


# ---- the set-up positions of the static test: name -> FEN.  Nothing is searched from them, but every one is a legal
# position with few moves (the side that has moved is not in check; no move list can overflow)
SETUPS = (
    ("passed_pawns", "4k3/2p5/8/P3P3/6p1/8/1P6/4K3 w - - 0 1"),
    ("doubled_isolated", "4k3/5p2/5p2/8/8/2P5/2P3P1/4K3 b - - 0 1"),
    ("rook_files", "3rk3/R4p2/8/8/8/8/1P1P1r2/1R2KR2 w - - 0 1"),
    ("bishop_pair", "2b1kb2/8/8/8/8/8/8/2B1KN2 w - - 0 1"),
    ("sheltered_kings", "6k1/5ppp/8/8/8/8/5PPP/6K1 w - - 0 1"),
    ("bare_king_and_shelter", "4k3/8/8/8/8/5P2/6PP/6K1 b - - 0 1"),
    ("knight_attacker", "6k1/8/5N2/8/8/8/8/4K3 b - - 0 1"),
    ("bishop_attacker", "6k1/8/8/8/8/8/1B6/4K3 w - - 0 1"),
    ("rook_attacker", "6k1/8/8/8/8/8/8/4K1R1 b - - 0 1"),
    ("queen_attacker", "6k1/8/8/8/3Q4/8/8/4K3 w - - 0 1"),
    ("nine_queens", "QQQQQQQQ/7Q/8/8/8/8/k7/7K b - - 0 1"),
    ("black_to_move", "rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq e3 0 1"),
    ("bare_kings", "4k3/8/8/8/8/8/8/4K3 w - - 0 1"),
    ("middlegame", "r2q1rk1/pp2bppp/2n1bn2/3p4/3P4/2NBPN2/PP3PPP/R1BQ1RK1 w - - 0 10"),
    ("black_ahead", "3qk3/8/8/8/8/8/4P3/4K3 w - - 0 1"),
)


def from_fen(fen):
    return OracleGame(board=board_from_fen(fen))


@functools.lru_cache(maxsize=None)
def setup_games():
    return tuple((name, from_fen(fen)) for name, fen in SETUPS)


@functools.lru_cache(maxsize=None)
def games():
    """[(name, OracleGame)]: the searched roots -- the 28 of ``repetition_util.games()`` (the 19 of ``opponent_util`` /
    ``quiescence_util`` / ``ordering_util`` and the nine with a history)."""
    return tuple(repetition_util.games())


@functools.lru_cache(maxsize=None)
def static_games():
    """The static test's positions: the searched roots, then the set-up positions."""
    return games() + setup_games()


UNREACHED = repetition_util.UNREACHED
# (maximum depth, quiescence, budget, ordering, repetition) of the GPU search test: every shape of kernel, a budget that
# cuts and one nothing reaches (that one without the root whose depth-2 search alone is large)
CASES = ((1, 0, 5, False, False), (2, 0, 63, False, False), (2, 2, 60, False, False), (3, 0, 150, True, False),
         (3, 2, 200, True, False), (3, 0, 200, False, True), (2, 2, 150, False, True), (3, 0, 300, True, True),
         (3, 2, 200, True, True), (2, 0, UNREACHED, True, True))


def in_case(name, case):
    return not (case[2] == UNREACHED and name == ordering_util.BIG_ROOT)


@functools.lru_cache(maxsize=None)
def reference(max_depth, quiescence, budget, ordering, repetition, evaluation="positional"):
    """``search`` of every game of the case (None for a root the case leaves out), computed once and never changed."""
    case = (max_depth, quiescence, budget, ordering, repetition)
    return tuple(search(g, max_depth, budget, quiescence, ordering, repetition, evaluation) if in_case(name, case)
                 else None for name, g in games())


def flip_fen(fen):
    """Ranks mirrored, colours and the side to move exchanged; castling rights exchanged, the en-passant square
    mirrored."""
    board, turn, castling, ep, half, full = fen.split()
    board = "/".join(row.swapcase() for row in reversed(board.split("/")))
    turn = "b" if turn == "w" else "w"
    castling = "".join(sorted(castling.swapcase())) if castling != "-" else "-"
    if ep != "-":
        ep = ep[0] + str(9 - int(ep[1]))
    return " ".join((board, turn, castling, ep, half, full))


def _mirror(bb):
    """The ranks of a bitboard mirrored."""
    return int.from_bytes(int(bb).to_bytes(8, "little"), "big")


def flip_game(game):
    """A game whose only position is the colour flip of ``game``'s current one (no history: the static evaluation
    reads none)."""
    b, f = game.board_at(0), OcBoard()
    occ = 0
    for pt in range(6):
        f.bb[pt] = _mirror(b.bb[pt])
        occ |= int(b.bb[pt])
    f.white = _mirror(occ & ~int(b.white))
    st = int(b.state)
    castle, ep = (st >> 1) & 15, (st >> 5) & 127
    castle = ((castle & 3) << 2) | (castle >> 2)
    if ep < 64:
        ep ^= 56
    f.state = ((st & 1) ^ 1) | (castle << 1) | (ep << 5) | (st & ~0xFFF)
    return OracleGame(board=f)
