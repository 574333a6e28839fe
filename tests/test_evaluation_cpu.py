"""The positional evaluation of the built-in opponent (csrc/opponent.hpp, EVALUATION) without a GPU: what
tests/evaluation_util.py restates, held to the header's table by positions set up for it.

1. the material kind is ``opponent_util.evaluate``; ``using`` rebinds the search restatements' evaluation and puts it
   back;
2. a position and its colour flip score the same, for both kinds, on every root and set-up position of the GPU set;
3. per term of the table a pair of positions that differ in that term alone: the difference of their (MG, EG) sums is
   the weight.  Material, position and mobility of a piece cannot be told apart by moving the piece (its square decides
   all three), so for those the piece is added to a bare board and the sum is written out by hand;
4. both ends of the phase, the taper's truncation toward zero, the tempo;
5. the bound of the header, on nine queens and on every position of the set;
6. every row of the table is reached by the positions the GPU test evaluates, and by the searches it runs;
7. the host-side refusals, ``SearchMode.key``, the header, the symbol list and the command-line flags.
"""
import os
import re

import pytest

from tests import evaluation_util as ev
from tests import iterdeep_util
from tests import opponent_util as ou
from tests import ordering_util
from tests import quiescence_util
from tests import repetition_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1 ---------------------------------------------------------------------------------------------------------
def test_material_is_the_evaluation_of_opponent_util_and_using_puts_it_back():
    assert ev.EVALUATIONS["material"] is ou.evaluate
    modules = (quiescence_util, iterdeep_util, ordering_util, repetition_util)
    assert all(m.evaluate is ou.evaluate for m in modules)
    with ev.using("positional"):
        assert all(m.evaluate is ev.positional for m in modules)
        with pytest.raises(KeyError):
            with ev.using("unknown"):
                pass
        assert all(m.evaluate is ev.positional for m in modules)
    assert all(m.evaluate is ou.evaluate for m in modules)
    g = dict(ev.games())["kqk"]
    assert ev.search(g, 2, 63, evaluation="material") == iterdeep_util.iterdeep(g, 2, 63)
    assert ev.search(g, 2, 63, ordering=True, evaluation="material") == ordering_util.ordered(g, 2, 63)
    assert ev.search(g, 2, 63, repetition=True, evaluation="material") == repetition_util.repeated(g, 2, 63)
    start = ev.from_fen("rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1")
    assert ev.search(start, 1, 100)[1] != iterdeep_util.iterdeep(start, 1, 100)[1]     # another evaluation, another score
    assert all(m.evaluate is ou.evaluate for m in modules)


# ---- 2 ---------------------------------------------------------------------------------------------------------
def test_a_colour_flip_keeps_the_score():
    assert len(ev.static_games()) == 28 + len(ev.SETUPS)
    for name, g in ev.static_games():
        f = ev.flip_game(g)
        assert ev.positional(f) == ev.positional(g), name
        assert ou.evaluate(f) == ou.evaluate(g), name
        mg, eg, ph = ev.sums(g)
        assert ev.sums(f) == (-mg, -eg, ph), name
    for name, fen in ev.SETUPS:                                  # the two flips agree
        assert ev.positional(ev.from_fen(ev.flip_fen(fen))) == ev.positional(ev.from_fen(fen)), name


# ---- 3 ---------------------------------------------------------------------------------------------------------
# (row, position with the term, position without, (MG, EG) of with - without)
PAIRS = (
    ("pawn material", "7k/8/8/8/8/8/PPP5/7K w - - 0 1", "7k/8/8/8/8/8/1PP5/7K w - - 0 1", (100, 100)),
    ("pawn advancement", "7k/1p6/8/8/8/1P6/P1P5/7K w - - 0 1", "7k/1p6/8/8/8/8/PPP5/7K w - - 0 1", (6, 12)),
    ("pawn advancement", "7k/1p6/8/8/8/2P5/PP6/7K w - - 0 1", "7k/1p6/8/8/8/8/PPP5/7K w - - 0 1", (5 + 6, 12)),
    ("pawn passed", "7k/4p3/8/1P6/8/8/P1P5/7K w - - 0 1", "7k/1p6/8/1P6/8/8/P1P5/7K w - - 0 1", (20, 40)),
    ("pawn doubled", "7k/1p6/8/8/1P6/P7/1P6/7K w - - 0 1", "7k/1p6/8/8/1P6/P7/2P5/7K w - - 0 1", (-10, -20)),
    ("pawn isolated", "7k/8/8/8/8/8/PP1P4/7K w - - 0 1", "7k/8/8/8/8/8/PPP5/7K w - - 0 1", (-10, -15)),
    ("knight mobility", "4k3/8/8/8/8/8/1K6/N7 w - - 0 1", "4k3/8/8/8/8/1K6/8/N7 w - - 0 1", (4, 4)),
    ("knight mobility", "4k3/8/8/8/7p/8/8/N3K3 w - - 0 1", "4k3/8/8/8/p7/8/8/N3K3 w - - 0 1", (4, 4)),    # ~PA(enemy)
    ("bishop mobility", "k7/8/8/8/4K3/8/6P1/B7 w - - 0 1", "k7/8/8/8/4K3/8/1P6/B7 w - - 0 1", (4 * 7, 4 * 7)),
    ("rook mobility", "4k3/8/8/8/8/K7/8/R7 w - - 0 1", "4k3/8/8/8/8/8/K7/R7 w - - 0 1", (2, 4)),
    ("rook open file", "4k3/7p/8/8/8/8/K7/R7 w - - 0 1", "4k3/p7/8/8/8/8/K7/R7 w - - 0 1", (20 - 10, 10 - 5)),
    ("rook open file", "4k3/8/8/4P3/8/8/3K4/3R4 w - - 0 1", "4k3/8/8/3P4/8/8/3K4/3R4 w - - 0 1", (20, 10)),
    ("rook seventh", "8/R7/8/8/2K5/8/7k/8 w - - 0 1", "8/8/R7/8/2K5/8/7k/8 w - - 0 1", (10, 20)),
    ("king position", "4k3/8/8/8/8/8/1K6/8 w - - 0 1", "4k3/8/8/8/8/8/8/K7 w - - 0 1", (-10, 10)),
    ("king shelter", "4k3/8/8/8/8/8/5PPP/6K1 w - - 0 1", "4k3/8/8/8/8/8/5PPP/1K6 w - - 0 1", (3 * 8, 0)),
    ("king shelter", "4k3/8/8/8/8/7P/5PP1/6K1 w - - 0 1", "4k3/8/8/8/8/7P/5PP1/1K6 w - - 0 1", (3 * 8, 0)),
    ("knight king attack", "6k1/8/5N2/8/8/8/8/4K3 w - - 0 1", "k7/8/5N2/8/8/8/8/4K3 w - - 0 1", (8, 0)),
    ("bishop king attack", "6k1/8/8/8/8/8/1B6/4K3 w - - 0 1", "k7/8/8/8/8/8/1B6/4K3 w - - 0 1", (8, 0)),
    ("rook king attack", "6k1/8/8/8/8/2K5/8/6R1 w - - 0 1", "k7/8/8/8/8/2K5/8/6R1 w - - 0 1", (12, 0)),
    ("queen king attack", "6k1/8/8/8/8/8/1Q6/4K3 w - - 0 1", "4k3/8/8/8/8/8/1Q6/4K3 w - - 0 1", (20, 0)),
)
# (rows, position with the piece, position without, the sum by hand): a piece on a bare board
ADDED = (
    (("knight material", "knight position", "knight mobility"),
     "4k3/8/8/8/8/8/8/N3K3 w - - 0 1", "4k3/8/8/8/8/8/8/4K3 w - - 0 1", (320 + 10 * 0 + 4 * 2,) * 2),
    (("bishop material", "bishop position", "bishop mobility"),
     "4k3/8/8/8/3B4/8/8/4K3 w - - 0 1", "4k3/8/8/8/8/8/8/4K3 w - - 0 1", (330 + 5 * 3 + 4 * 13,) * 2),
    (("bishop pair",),                            # the second bishop on f1: seven squares, and the pair
     "4k3/8/8/8/8/8/8/2B1KB2 w - - 0 1", "4k3/8/8/8/8/8/8/2B1K3 w - - 0 1", (330 + 4 * 7 + 30, 330 + 4 * 7 + 40)),
    (("rook material", "rook mobility", "rook open file"),     # a1: seven squares of the file, three of the rank
     "4k3/8/8/8/8/8/8/R3K3 w - - 0 1", "4k3/8/8/8/8/8/8/4K3 w - - 0 1", (500 + 2 * 10 + 20, 500 + 4 * 10 + 10)),
    (("queen material", "queen position", "queen mobility"),   # a1: 21 squares, no king in reach
     "2K5/8/8/8/8/5k2/8/Q7 w - - 0 1", "2K5/8/8/8/8/5k2/8/8 w - - 0 1", (900 + 2 * 0 + 21, 900 + 2 * 0 + 2 * 21)),
)


def difference(with_fen, without_fen):
    a, b = ev.sums(ev.from_fen(with_fen)), ev.sums(ev.from_fen(without_fen))
    return a[0] - b[0], a[1] - b[1]


def changed_rows(with_fen, without_fen):
    """The rows whose total differs between the two positions."""
    def totals(fen):
        out = {}
        for row, mg, eg in ev.terms(ev.from_fen(fen)):
            m, e = out.get(row, (0, 0))
            out[row] = (m + mg, e + eg)
        return out
    a, b = totals(with_fen), totals(without_fen)
    return set(row for row in set(a) | set(b) if a.get(row, (0, 0)) != b.get(row, (0, 0)))


@pytest.mark.parametrize("row,with_fen,without_fen,weight", PAIRS)
def test_a_pair_of_positions_differs_by_the_weight_of_the_table(row, with_fen, without_fen, weight):
    assert difference(with_fen, without_fen) == weight
    # the pair differs in that row alone (the half-open file turns into an open one in one pair)
    assert changed_rows(with_fen, without_fen) - {"rook half-open file"} == {row}
    # and black's term is the negative
    assert difference(ev.flip_fen(with_fen), ev.flip_fen(without_fen)) == (-weight[0], -weight[1])


@pytest.mark.parametrize("rows,with_fen,without_fen,total", ADDED)
def test_a_piece_added_to_a_bare_board_is_worth_the_sum_by_hand(rows, with_fen, without_fen, total):
    assert difference(with_fen, without_fen) == total
    assert set(rows) <= set(row for row, _, _ in ev.terms(ev.from_fen(with_fen)))
    assert changed_rows(with_fen, without_fen) <= set(rows) | {"bishop material", "bishop mobility"}
    assert difference(ev.flip_fen(with_fen), ev.flip_fen(without_fen)) == (-total[0], -total[1])


def test_the_pairs_cover_the_table():
    covered = set(row for row, _, _, _ in PAIRS) | set(r for rows, _, _, _ in ADDED for r in rows)
    assert covered | {"rook half-open file"} == set(ev.ROWS)
    assert any(w == (10, 5) for row, _, _, w in PAIRS if row == "rook open file")       # open - half-open = (10, 5)


# ---- 4 ---------------------------------------------------------------------------------------------------------
def test_phase_taper_and_tempo():
    setups = dict(ev.setup_games())
    assert ev.positional(setups["bare_kings"]) == 10                                    # nothing but the tempo
    # ph = 0: the endgame sum alone; ph = 24: the middlegame sum alone
    for name, ph in (("passed_pawns", 0), ("doubled_isolated", 0), ("black_to_move", 24), ("middlegame", 24),
                     ("nine_queens", 24)):
        g = setups[name]
        mg, eg, got = ev.sums(g)
        assert got == ph, name
        white = eg if ph == 0 else mg
        assert ev.positional(g) == (white if g.turn else -white) + 10, name
    assert ev.sums(setups["passed_pawns"])[0] != ev.sums(setups["passed_pawns"])[1]     # the two sums do differ there
    # in between, and truncating toward zero where white is behind
    mg, eg, ph = ev.sums(setups["black_ahead"])
    assert 0 < ph < 24 and mg < 0 and (mg * ph + eg * (24 - ph)) % 24 != 0
    white = -((-(mg * ph + eg * (24 - ph))) // 24)
    assert ev.positional(setups["black_ahead"]) == white + 10
    assert white == (mg * ph + eg * (24 - ph)) // 24 + 1                                # not the floor
    assert ev.trunc_div(-25, 24) == -1 and ev.trunc_div(25, 24) == 1 and ev.trunc_div(-24, 24) == -1
    # nine queens and more: the phase stops at 24
    assert ev.phase(setups["nine_queens"]) == 24 and 4 * 9 > 24
    # the tempo belongs to the side to move
    w, b = ev.from_fen("4k3/8/8/8/8/8/4P3/4K3 w - - 0 1"), ev.from_fen("4k3/8/8/8/8/8/4P3/4K3 b - - 0 1")
    assert ev.positional(w) - 10 == -(ev.positional(b) - 10) != 0


# ---- 5 ---------------------------------------------------------------------------------------------------------
def test_the_bound_holds():
    header = open(os.path.join(ROOT, "chessrl_amd", "csrc", "opponent.hpp")).read()
    assert "|score| <= %d" % ev.BOUND in header
    assert ev.BOUND == 15 * 960 + 48 + 40 + 30 + 10 and ev.BOUND < ou.MATE - 11 - 10000
    nine = dict(ev.setup_games())["nine_queens"]
    mg, eg, _ = ev.sums(nine)
    assert len([t for t in ev.terms(nine) if t[0] == "queen material"]) == 9
    assert 9 * 900 < abs(ev.positional(nine)) <= ev.BOUND and max(abs(mg), abs(eg)) < 2 ** 15
    for name, g in ev.static_games():
        assert abs(ev.positional(g)) <= ev.BOUND, name
        # every per-piece term fits the packed reduction's halves
        assert all(abs(m) < 2 ** 15 and abs(e) < 2 ** 15 for _, m, e in ev.terms(g)), name


# ---- 6 ---------------------------------------------------------------------------------------------------------
def test_every_row_is_reached_by_the_gpu_set():
    static_rows = set(row for _, g in ev.static_games() for row, _, _ in ev.terms(g))
    assert static_rows == set(ev.ROWS)
    root_rows = set(row for _, g in ev.games() for row, _, _ in ev.terms(g))
    print("rows the searched roots do not hold themselves:", sorted(set(ev.ROWS) - root_rows))
    assert len(root_rows) >= 20
    names = [n for n, _ in ev.setup_games()]
    for needed in ("passed_pawns", "doubled_isolated", "rook_files", "bishop_pair", "sheltered_kings",
                   "bare_king_and_shelter", "knight_attacker", "bishop_attacker", "rook_attacker", "queen_attacker",
                   "nine_queens", "black_to_move", "bare_kings"):
        assert needed in names
    # the cases: every shape of kernel (quiescence x ordering x repetition), D <= 3, Q <= 2, a budget that cuts and one
    # nothing reaches
    shapes = set((q > 0, o, r) for _, q, _, o, r in ev.CASES)
    assert len(shapes) == 8 and all(d <= 3 and q <= 2 for d, q, _, _, _ in ev.CASES)
    assert any(b == ev.UNREACHED for _, _, b, _, _ in ev.CASES)


# ---- 7 ---------------------------------------------------------------------------------------------------------
def test_host_refusals_the_mode_key_and_the_header():
    from chessrl_amd import _lib
    from chessrl_amd import benchmark as bm
    from chessrl_amd import gen_data as gd
    from chessrl_amd.opponent import GameOpponent, MinimaxPlayer
    from chessrl_amd.searchmode import SearchMode
    p = MinimaxPlayer(False, 3, node_budget=300, evaluation="positional")
    assert (p.evaluation, MinimaxPlayer(True).evaluation, MinimaxPlayer(True, node_budget=300).evaluation) == (
        "positional", "material", "material")
    assert MinimaxPlayer(False, 3, ou.NODE_LIMIT, 0, 300, True, True).evaluation == "material"   # positional calls stay
    needs = "evaluation needs a node_budget"
    with pytest.raises(ValueError, match=needs):
        MinimaxPlayer(True, evaluation="positional")
    with pytest.raises(ValueError, match=needs):
        bm.benchmark(None, games=4, opponent_evaluation="positional", model=object())
    with pytest.raises(ValueError, match=needs):
        gd.gen_data("unused.json", num_games=4, evaluation="positional")
    with pytest.raises(ValueError, match=needs):
        _lib.Context.opponent_moves(None, [1], evaluation="positional")             # before any device call
    with pytest.raises(ValueError, match=needs):
        _lib.Context.sim_reply_opponent(None, 0, 1000, 0, 0, 0, evaluation="positional")
    unknown = "evaluation must be one of"
    for bad in ("Positional", "pst", None, 1, True):
        with pytest.raises(ValueError, match=unknown):
            MinimaxPlayer(True, node_budget=300, evaluation=bad)
        with pytest.raises(ValueError, match=unknown):
            _lib.Context.opponent_moves(None, [1], node_budget=300, evaluation=bad)
        with pytest.raises(ValueError, match=unknown):
            _lib.Context.sim_reply_opponent(None, 0, 1000, 0, 0, 0, node_budget=300, evaluation=bad)
        with pytest.raises(ValueError, match=unknown):
            _lib.Context.opponent_evaluate(None, bad)
        with pytest.raises(ValueError, match=unknown):
            bm.benchmark(None, games=4, opponent_budget=300, opponent_evaluation=bad, model=object())
        with pytest.raises(ValueError, match=unknown):
            gd.gen_data("unused.json", num_games=4, node_budget=300, evaluation=bad)
    # the older refusals keep their words
    with pytest.raises(ValueError, match="ordering needs a node_budget"):
        MinimaxPlayer(True, ordering=True, evaluation="positional")
    with pytest.raises(ValueError, match="repetition needs a node_budget"):
        _lib.Context.opponent_moves(None, [1], repetition=True, evaluation="positional")
    assert "opponent_evaluation" in GameOpponent.__init__.__code__.co_varnames
    key = lambda **kw: SearchMode(reply=MinimaxPlayer(False, 3, node_budget=300, **kw)).key
    assert key(evaluation="positional") == SearchMode(
        reply=MinimaxPlayer(True, 3, node_budget=300, evaluation="positional")).key
    assert len({key(), key(evaluation="positional"), key(ordering=True, evaluation="positional"),
                key(repetition=True, evaluation="positional"), key(repetition=True)}) == 5
    assert key(evaluation="material") == key()
    mode = SearchMode(reply=p)
    assert mode.kind == "opponent" and [name for _, name in mode.plan] == [
        "phase_select_expand", "phase_reply_opponent", "phase_tower_s2"]
    text = open(os.path.join(ROOT, "include", "chessrl_hip.h")).read()
    for name in ("crl_opponent_moves_ev", "crl_sim_reply_opponent_ev"):
        assert name in _lib.SYMBOLS
        decl = re.search(r"int  %s\(.*?\);" % name, text, re.S).group(0)
        assert "int ordering, int repetition, int evaluation" in decl, name
    assert "crl_opponent_evaluate" in _lib.SYMBOLS
    assert re.search(r"int  crl_opponent_evaluate\(crl_ctx \*ctx, int evaluation, int32_t \*scores", text)
    assert "#define CRL_OPP_EVAL_MATERIAL 0" in text and "#define CRL_OPP_EVAL_POSITIONAL 1" in text
    assert _lib.OPP_EVALUATIONS == {"material": 0, "positional": 1}
    header = open(os.path.join(ROOT, "chessrl_amd", "csrc", "opponent.hpp")).read()
    assert "// EVALUATION (" in header and "static_assert(ID || !POS" in header
    assert "int opp_evaluate_positional(const Board &b, int lane)" in header
    assert re.search(r"void k_opponent_evaluate\(", header)
    # the budgeted kernels are two templates over the six flags (POS among them), their legal shapes stated once
    for k in ("k_opponent_moves_id", "k_reply_opponent_id"):
        assert re.search(r"template <bool QS, bool ORD, bool REP, bool POS, bool SEL, bool EXC>\s*"
                         r"__global__ __launch_bounds__\(64\) void %s\(" % k, header), k
    assert re.search(r"constexpr bool opp_shape_legal\(bool QS, bool ORD,", header)
    assert re.search(r"static_assert\(opp_legal_shapes\(\) == 32,", header)
    assert "static_assert(opp_shape_legal(QS, ORD, REP, POS, SEL, EXC)" in header


def test_cli_flags():
    from chessrl_amd import benchmark as bm
    from chessrl_amd import gen_data as gd
    for module in (bm, gd):
        with pytest.raises(SystemExit):
            module.main(["somewhere", "--eval", "pst"])
    with pytest.raises(ValueError, match="evaluation needs a node_budget"):
        gd.main(["unused.json", "--games", "2", "--eval", "positional"])
