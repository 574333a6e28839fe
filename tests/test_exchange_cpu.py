"""The restatement of the built-in opponent's delta and exchange pruning (tests/exchange_util.py; csrc/opponent.hpp
EXCHANGE) held to its own definition, to the existing restatements and to what the GPU test needs, without a GPU.

1. the two forms of the exchange test -- the list of gains by the definition, the balance and answer bit of the kernel --
   agree on every tactical move of a few hundred positions from random games;
2. hand-made positions whose values are worked out by hand below;
3. with ``exchange`` off the search is ``selective_util.search`` (and so ``evaluation_util`` / ``ordering_util``) on
   their own roots, output for output;
4. the preconditions of the GPU test's roots, from the restatement's counters;
5. the ``ValueError``s of the keyword.
"""
import pytest

from oracle.chess_oracle import move_to_uci, uci_to_move
from tests import exchange_util as xu
from tests import opponent_util as ou
from tests import ordering_util as od
from tests import selective_util as su


# ---- 1 ---------------------------------------------------------------------------------------------------------
def test_the_two_forms_agree_on_random_positions():
    positions = xu.random_positions()
    assert len(positions) >= 300
    judged = negative = long_lists = 0
    for g in positions:
        for m in g.legal_move_ids():
            if not ou.tactical(g, m):
                assert xu.judge(g, m) == (False, True)
                continue
            value = xu.see(g, m)
            assert xu.see_not_negative(g, m) == (value >= 0), (g.get_fen(), move_to_uci(m), value)
            assert xu.judge(g, m) == (True, value >= 0)
            assert value <= xu.victim_value(g, m) + 800             # gain[0] bounds it; 800: a queen promoted
            judged += 1
            negative += value < 0
    print("tactical moves judged:", judged, "with a negative value:", negative)
    assert judged >= 300 and 30 < negative < judged - 30


# ---- 2 ---------------------------------------------------------------------------------------------------------
def values(name):
    fen = dict((n, f) for n, f, _, _ in xu.HAND_MADE)[name]
    g = xu.from_fen(fen)
    out = {}
    for m in g.legal_move_ids():
        if ou.tactical(g, m):
            out[move_to_uci(m)] = xu.see(g, m)
            assert xu.see_not_negative(g, m) == (out[move_to_uci(m)] >= 0), (name, move_to_uci(m))
    return out


def test_hand_made_values():
    for name, fen, uci, want in xu.HAND_MADE:                       # the table is the comments below
        g = xu.from_fen(fen)
        assert uci_to_move(uci) in g.legal_move_ids(), name
        assert values(name)[uci] == want, name
    # Rd1xd5, nothing attacks d5 (the king on e8 does not): gains [100] -> +100, kept
    assert values("rook_takes_loose_pawn") == {"d1d5": 100}
    # Nc3xd5 with a8-h1 holding q, b, (c6), the pawn, (e4), B, (g2), Q and a knight on f6:
    #   N takes P +100 | n takes N: 320 - 100 = 220 | B takes n: 320 - 220 = 100 | b takes B: 330 - 100 = 230 |
    #   Q takes b through f3 (x-ray): 330 - 230 = 100 | q takes Q through b7 (x-ray): 900 - 100 = 800 | nothing left
    #   back: 100 -> -max(-100, 800) = -800; 230 -> -max(-230, -800) = 230; 100 -> -max(-100, 230) = -230;
    #   220 -> -max(-220, -230) = 220; gain[0] = -max(-100, 220) = -220: removed
    assert values("xrays_both_sides")["c3d5"] == -220
    # the same exchange without the black queen's x-ray ends one capture earlier: gains [100, 220, 100, 230, 100] ->
    # 230 -> -max(-230, 100) = -100; 100 -> -max(-100, -100) = 100; 220 -> -max(-220, 100) = -100; gain[0] = +100.
    # With the white queen's x-ray missing as well it is [100, 220, 100, 230] -> -220 again: a form that sees no
    # x-ray at all is right here by accident, one that sees only the mover's is not
    no_q = xu.from_fen("6k1/1b6/5n2/3p4/8/2N2B2/8/6KQ w - - 0 1")
    assert xu.see(no_q, uci_to_move("c3d5")) == 100
    no_queens = xu.from_fen("6k1/1b6/5n2/3p4/8/2N2B2/8/6K1 w - - 0 1")
    assert xu.see(no_queens, uci_to_move("c3d5")) == -220
    # e5xd6 en passant: +100 | c7xd6: 100 - 100 = 0 | Rd1xd6, its file opened by the captured pawn: 100 - 0 = 100
    #   back: 0 -> -max(0, 100) = -100; gain[0] = -max(-100, -100) = +100 (with the pawn still on d5 it would be 0)
    assert values("en_passant_opens_the_file")["e5d6"] == 100
    # a7xb8=Q: 500 + 800 = 1300, nothing attacks b8.  a7-a8=Q: 0 + 800 | r takes Q: 900 - 800 = 100 -> -100, removed;
    # the under-promotions likewise: N 220 | 320 - 220 = 100 -> -100
    assert values("promotions") == {"a7b8q": 1300, "a7b8r": 900, "a7b8b": 730, "a7b8n": 720,
                                    "a7a8q": -100, "a7a8r": -100, "a7a8b": -100, "a7a8n": -100}
    assert xu.QUIET_PROMOTION == ("promotions", "a7a8q", -100)
    # Rd1xd5 +100 | the king on e6 is the last attacker and white has none left: k takes R 500 - 100 = 400 -> -400
    assert values("king_may_capture") == {"d1d5": -400}
    # the same with a bishop on g2 behind d5: white still attacks d5, the king may not capture -> [100] -> +100
    assert values("king_may_not_capture") == {"d1d5": 100, "g2d5": 100}


# ---- 3 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,quiescence,budget,repetition,evaluation,selective",
                         [(3, 2, 300, True, "positional", True), (3, 2, 200, False, "material", False),
                          (4, 2, 196, False, "material", True), (3, 0, 150, True, "material", False)])
def test_exchange_off_is_the_existing_restatement(depth, quiescence, budget, repetition, evaluation, selective):
    cut = 0
    for name, g in su.games():
        mine = xu.search(g, depth, budget, quiescence, repetition, evaluation, selective, exchange=False)
        assert mine == su.search(g, depth, budget, quiescence, repetition, evaluation, selective), name
        cut += mine[3] == ou.CUT
    assert 0 < cut < len(su.games())
    if not repetition and evaluation == "material" and not selective:
        for name, g in od.games():
            assert xu.search(g, depth, budget, quiescence, exchange=False) == od.ordered(g, depth, budget, quiescence)


# ---- 4 ---------------------------------------------------------------------------------------------------------
def test_the_gpu_set_meets_its_preconditions():
    names = [n for n, _ in xu.games()]
    assert 10 <= len(names) <= 16 and set(n for n, _, _, _ in xu.HAND_MADE) <= set(names)
    assert len(xu.CASES) == 8 and {(rep, kind, sel) for _, _, _, rep, kind, sel in xu.CASES} == {
        (rep, kind, sel) for rep in (False, True) for kind in ("material", "positional") for sel in (False, True)}
    assert {c[0] for c in xu.CASES} <= {2, 3, 4} and {c[1] for c in xu.CASES} == {1, 2, 4}
    assert max(c[2] for c in xu.CASES) <= 3000
    total = xu.new_counts()
    differs = unchanged = cut = whole = nodes = 0
    for case in xu.CASES:
        rows, counts, per_root = xu.reference(*case)
        off = xu.reference(*case, exchange=False)[0]
        for (name, g), on, plain, c in zip(xu.games(), rows, off, per_root):
            move, score, n, flag, done = on
            assert move in g.legal_move_ids() and n <= case[2] and (flag == ou.CUT) == (done < case[0]), name
            differs += on[:2] != plain[:2]
            if c["delta_removed"] + c["exchange_removed"] == 0:     # consequence (b): nothing removable, nothing changes
                assert on == plain, (name, case)
                unchanged += c["nodes_4c"] > 0
            cut += flag == ou.CUT
            whole += flag == 0
            nodes += n
        for k, v in counts.items():
            total[k] += v
        print(case, counts)
    print("nodes of the GPU set:", nodes, total, "roots that differ:", differs, "unchanged:", unchanged)
    for k in ("delta_removed", "exchange_removed", "promotion_spared_by_delta", "list_emptied", "in_check_unfiltered"):
        assert total[k] > 0, k
    assert differs > 0 and unchanged > 0 and cut > 0 and whole > 0
    assert nodes < 60000


# ---- 5 ---------------------------------------------------------------------------------------------------------
def test_value_errors():
    from chessrl_amd import _lib
    from chessrl_amd.opponent import MinimaxPlayer
    options = lambda exchange, ordering, node_budget, quiescence: _lib.OpponentOptions(
        quiescence=quiescence, node_budget=node_budget, ordering=ordering, exchange=exchange)
    assert options(False, False, None, 0).exchange is False
    assert options(True, True, 100, 1).exchange is True
    with pytest.raises(ValueError, match="exchange needs ordering"):
        options(True, False, 100, 2)
    with pytest.raises(ValueError, match="ordering needs a node_budget"):
        options(True, True, None, 2)
    with pytest.raises(ValueError, match="exchange needs quiescence"):
        options(True, True, 100, 0)
    with pytest.raises(ValueError, match="exchange needs ordering"):
        MinimaxPlayer(True, 3, node_budget=100, quiescence=2, exchange=True)
    with pytest.raises(ValueError, match="ordering needs a node_budget"):
        MinimaxPlayer(True, 3, ordering=True, quiescence=2, exchange=True)
    with pytest.raises(ValueError, match="exchange needs quiescence"):
        MinimaxPlayer(True, 3, node_budget=100, ordering=True, exchange=True)
    p = MinimaxPlayer(True, 3, node_budget=100, ordering=True, quiescence=1, exchange=True)
    assert p.exchange is True and MinimaxPlayer(True, 3).exchange is False
