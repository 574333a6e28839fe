"""No GPU: the restatement of the built-in opponent's quiescence search (tests/quiescence_util.py) and what
tests/test_gpu_quiescence.py leans on, asserted with the oracle alone.

1. quiescence 0 is ``opponent_util.alphabeta``;
2. alpha-beta with the victim order equals the pruning-free minimax in move and score;
3. the known answer: without quiescence depth 1 takes a defended pawn with its queen; with it, never;
4. the set the GPU test runs reaches every branch of the rule;
5. the node limit cuts deterministically.
"""
import pytest

from oracle.chess_oracle import OracleGame, board_from_fen, move_to_uci, uci_to_move
from tests import opponent_util as ou
from tests import quiescence_util as q


def named(name):
    return dict(q.games())[name]


def test_quiescence_zero_is_the_fixed_depth_search():
    for name, g in q.games()[:16]:
        for depth in (1, 2):
            assert q.alphabeta_q(g, depth, 0) == ou.alphabeta(g, depth), (name, depth)
    g = named("midgame_40")
    assert q.alphabeta_q(g, 2, 0, node_limit=50) == ou.alphabeta(g, 2, node_limit=50)


@pytest.mark.parametrize("depth,quiescence", [(1, 1), (1, 2), (2, 1)])
def test_alphabeta_equals_minimax(depth, quiescence):
    for name, g in q.games()[:16]:
        if depth == 2 and name not in q.ENDGAMES:
            continue
        got = q.alphabeta_q(g, depth, quiescence)
        assert got[:2] == q.minimax_q(g, depth, quiescence) and got[3] == 0, (name, depth, quiescence)


def test_victim_class():
    # every victim on one board: the white queen on d4 can take q r b n p, the pawn on g7 promotes with and without
    # a capture, and a quiet move stays out
    g = OracleGame(board=board_from_fen("k4n2/6P1/1r6/8/q2Q2n1/8/1b3p2/7K w - - 0 1"))
    cls = {move_to_uci(m): q.victim_class(g, m) for m in g.legal_move_ids()}
    assert (cls["d4a4"], cls["d4b6"], cls["d4b2"], cls["d4g4"], cls["d4f2"]) == (0, 1, 2, 3, 4)
    assert cls["g7f8q"] == cls["g7f8n"] == 3 and cls["g7g8q"] == cls["g7g8r"] == 5 and cls["d4d5"] == 6
    e = OracleGame(board=board_from_fen("4k3/8/8/8/3p4/8/4P3/4K3 w - - 0 1"))
    assert e.move("e2e4")
    assert q.victim_class(e, uci_to_move("d4e3")) == 4 and q.victim_class(e, uci_to_move("d4d3")) == 6


def test_the_known_answer():
    g = OracleGame(board=board_from_fen(q.KNOWN_ANSWER))
    assert move_to_uci(q.alphabeta_q(g, 1, 0)[0]) == "e2e5"
    for quiescence in (1, 2, 4, 6):
        m = q.alphabeta_q(g, 1, quiescence)[0]
        after = q.child(g, m)
        print("quiescence", quiescence, move_to_uci(m))
        assert move_to_uci(m) != "e2e5"
        assert uci_to_move("d6e5") not in after.legal_move_ids()          # the queen is not left to the pawn


def test_the_gpu_set_reaches_every_branch():
    total = q.new_counts()
    nodes = 0
    for depth, quiescence in q.CASES:
        rows, counts = q.reference(depth, quiescence)
        assert not any(r[3] for r in rows if r is not None)                # nothing is cut at the default limit
        nodes += sum(r[2] for r in rows if r is not None)
        for k, v in counts.items():
            total[k] += v
    print(nodes, "nodes", total)
    assert all(total[k] > 0 for k in q.BRANCHES if k != "all_victims"), total
    assert 20000 < nodes < 100000
    # where the issue's three positions give what they were chosen for
    fen = {f: i + 16 for i, f in enumerate(q.FENS)}

    def counts_of(f, depth, quiescence):
        c = q.new_counts()
        q.alphabeta_q(q.games()[fen[f]][1], depth, quiescence, counts=c)
        return c
    assert counts_of(q.EN_PASSANT, 1, 1)["en_passant"] > 0
    c = counts_of(q.PROMOTIONS, 2, 1)
    assert c["promotion_capture"] > 0 and c["promotion_quiet"] > 0
    for depth in (1, 2):                                                   # a node at ply d + Q with Q = 6
        assert q.reference(depth, 6)[1]["last_ply"] > 0


def test_the_cut_is_deterministic():
    g = named("midgame_40")
    legal = g.legal_move_ids()
    whole = q.alphabeta_q(g, 2, 6)
    full = whole[2]
    assert whole[3] == 0 and full > 1000
    for limit in (full + 1, full):
        assert q.alphabeta_q(g, 2, 6, node_limit=limit) == whole
    for limit in (full - 1, full // 2, 1):
        m, score, nodes, flag = q.alphabeta_q(g, 2, 6, node_limit=limit)
        assert (flag, nodes) == (ou.CUT, limit) and m in legal
        assert q.alphabeta_q(g, 2, 6, node_limit=limit) == (m, score, nodes, flag)


def test_host_refusals():
    from chessrl_amd import _lib
    from chessrl_amd import benchmark as bm
    from chessrl_amd.opponent import MinimaxPlayer
    assert _lib.OPP_MAX_QUIESCENCE == q.MAX_QUIESCENCE == 6
    assert MinimaxPlayer(True).quiescence == 0 and MinimaxPlayer(False, 1, quiescence=6).quiescence == 6
    for bad in (-1, 7):
        with pytest.raises(ValueError, match="quiescence"):
            MinimaxPlayer(True, quiescence=bad)
        with pytest.raises(ValueError, match="quiescence"):
            bm.benchmark(None, games=4, opponent_quiescence=bad, model=object())
