"""No GPU: the built-in opponent's repetition rule (csrc/opponent.hpp REPETITION) through its CPU restatement
(tests/repetition_util.py), the preconditions of tests/test_gpu_repetition.py and the host-side surface.

1. the table of cases: scores, moves and the two en-passant children;
2. consequence (a): with a budget nothing reaches, ordering on and off agree in everything but the nodes, on every root;
3. consequence (b): from the roots with halfmove clock 0 and D + Q <= 3 every output, nodes included, is that of the
   search without the rule;
4. every budget from 1 to the whole search and one more on two small roots;
5. the set the GPU test runs reaches the branches of ``repetition_util.BRANCHES``;
6. six games of depth 2 against itself: four end by the fifth occurrence without the rule, fewer with it;
7. the host-side refusals, ``SearchMode.key``, the header and the symbol list.
"""
import os
import random
import re

import pytest

from oracle.chess_oracle import OracleGame, move_to_uci, uci_to_move
from tests import iterdeep_util as it
from tests import opponent_util as ou
from tests import ordering_util as od
from tests import repetition_util as rp
from tests import rollout_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = rp.UNREACHED


def uci(m):
    return move_to_uci(m)


# ---- 1 ---------------------------------------------------------------------------------------------------------
def test_the_table_of_cases():
    """The table was measured with a plain fixed-depth alpha-beta (``repetition_util.fixed_depth``); what does not
    depend on the root order of the iterations is asserted through the restatement as well."""
    g = rp.table_game("kqk_black")
    for d in (1, 2, 3, 4):
        move, score, nodes, flag, done = rp.repeated(g, d, B)
        plain = it.iterdeep(g, d, B)
        assert (uci(move), score, flag, done) == ("g8h8", 0, 0, d) and uci(plain[0]) == "g8h8"
        assert plain[1] == (-900 if d == 1 else -906)
        assert rp.fixed_depth(g, d, True)[:2] == (move, 0) and rp.fixed_depth(g, d, False)[1] == plain[1]
    assert (rp.fixed_depth(g, 4, False)[2], rp.fixed_depth(g, 4, True)[2]) == (617, 19)

    g = rp.table_game("start_knights")                      # the move changes at depth 2 in the fixed-depth search; the
    assert uci(rp.fixed_depth(g, 2, False)[0]) == "e2e4"    # iterations hand e2e4, their depth-1 move, to the front of
    assert uci(rp.fixed_depth(g, 2, True)[0]) == "g1f3"     # the root, where it ties at 0 and stays: fewer nodes only
    on, off = rp.repeated(g, 2, B), it.iterdeep(g, 2, B)
    assert on[:2] == off[:2] == (uci_to_move("e2e4"), 0) and on[2] < off[2]

    g = rp.table_game("kqk_white")                          # the same move and score; 12 hits at depth 3, 28 at depth 4
    for d, hits in ((1, 1), (2, 1), (3, 12), (4, 28)):
        counts = {}
        assert rp.fixed_depth(g, d, True, counts)[:2] == rp.fixed_depth(g, d, False)[:2] and counts["hits"] == hits
        on, off = rp.repeated(g, d, B), it.iterdeep(g, d, B)
        assert on[:2] == off[:2] and on[1] == 906 and on[3:] == off[3:] == (0, d)

    g = rp.table_game("kqk_nohist")                         # no hit at depths 1-3; 24 at depth 4, all on the path, all
    for d in (1, 2, 3, 4):                                  # at the horizon
        counts, c = {}, rp.new_counts()
        fixed = rp.fixed_depth(g, d, True, counts)
        assert counts.get("hits", 0) == (24 if d == 4 else 0) and fixed == rp.fixed_depth(g, d, False)
        on = rp.repeated(g, d, B, counts=c)
        assert on == it.iterdeep(g, d, B)
        assert (c["path_hit"], c["hit_at_horizon"], c["history_hit"], c["hit_at_inner_node"]) == \
            ((24, 24, 0, 0) if d == 4 else (0, 0, 0, 0))

    back = uci_to_move("f6g8")                              # the two en-passant children
    legal, none = rp.table_game("ep_legal"), rp.table_game("ep_none")
    assert ou.child(legal, back).repetitions() == 1 and ou.child(none, back).repetitions() == 2
    c = rp.new_counts()
    assert rp.repeated(legal, 1, B, counts=c) == it.iterdeep(legal, 1, B)
    assert c["ep_legal_is_no_hit"] == 1 and c["history_hit"] == 0
    c = rp.new_counts()
    rp.repeated(none, 1, B, counts=c)
    assert c["ep_legal_is_no_hit"] == 0 and c["history_hit"] == 1


# ---- 2 ---------------------------------------------------------------------------------------------------------
def test_ordering_changes_the_nodes_alone():
    fewer = 0
    for name, g in rp.games():
        for d, q in ((2, 0), (3, 0), (2, 2)):
            if name == od.BIG_ROOT and d + q > 2:
                continue
            off, on = rp.repeated(g, d, B, q), rp.repeated(g, d, B, q, ordering=True)
            assert off[:2] == on[:2] and off[3:] == on[3:] == (0, d), (name, d, q)
            fewer += on[2] < off[2]
    assert fewer >= 10                                      # and the order is a real one


# ---- 3 ---------------------------------------------------------------------------------------------------------
def test_clock_zero_roots_are_searched_as_without_the_rule():
    roots = [(n, g) for n, g in od.games() if rp.clock(g) == 0]
    assert len(od.games()) == 19 and len(roots) >= 12
    for name, g in roots:
        for d, q in ((1, 0), (2, 0), (3, 0), (1, 2), (2, 1)):
            if name == od.BIG_ROOT and d + q > 2:
                continue
            for budget in (B, 150):
                c = rp.new_counts()
                assert rp.repeated(g, d, budget, q, counts=c) == it.iterdeep(g, d, budget, q), (name, d, q)
                assert rp.repeated(g, d, budget, q, ordering=True) == od.ordered(g, d, budget, q), (name, d, q)
                assert not any(c[k] for k in rp.BRANCHES if k != "ep_legal_is_no_hit")


# ---- 4 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,depth,quiescence,ordering", [("kqk_black", 3, 0, False), ("ep_none", 2, 1, True)])
def test_every_budget(name, depth, quiescence, ordering):
    g = rp.table_game(name)
    whole = rp.repeated(g, depth, B, quiescence, ordering)
    total, legal, last = whole[2], g.legal_move_ids(), 0
    assert whole[3:] == (0, depth) and 20 <= total <= 400
    for budget in range(1, total + 2):
        move, score, nodes, flag, done = rp.repeated(g, depth, budget, quiescence, ordering)
        assert move in legal and nodes == min(budget, total)
        assert done >= last and (flag == ou.CUT) == (done < depth) == (budget < total)
        last = done
    assert rp.repeated(g, depth, total, quiescence, ordering) == whole == rp.repeated(g, depth, total + 1, quiescence,
                                                                                     ordering)


# ---- 5 ---------------------------------------------------------------------------------------------------------
REQUIRED = ("history_hit", "path_hit", "hit_at_horizon", "hit_at_inner_node", "ep_legal_is_no_hit", "result_ahead_of_hit")


def test_the_gpu_set_reaches_the_branches():
    total, nodes = rp.new_counts(), 0
    names = [n for n, _ in rp.games()]
    assert names[:19] == [n for n, _ in od.games()] and len(names) == 28
    assert rp.CASES == ((2, 0, 63), (3, 0, 150), (3, 0, 600), (4, 0, 2000), (3, 2, 300), (3, 2, 600), (2, 0, B))
    for L in rp.STRADDLE_L:                                 # the earlier occurrences lie on both sides of the ring wrap
        g = dict(rp.games())["straddle_%d" % L]
        assert len(g) == L + 10 > 256 > L and g.repetitions() == 3 and rp.clock(g) >= 10
    assert len(dict(rp.games())["forced_fifth_cut"]) == 14
    for case in rp.CASES:
        for ordering in (False, True):
            rows, counts = rp.reference(*case, ordering)
            for (name, g), row in zip(rp.games(), rows):
                assert (row is None) == (case[0] == 4 and name not in rp.SMALL)
                if row is not None:
                    move, score, n, flag, done = row
                    assert move in g.legal_move_ids() and n <= case[2] and (flag == ou.CUT) == (done < case[0]), name
            nodes += sum(r[2] for r in rows if r is not None)
            for k, v in counts.items():
                total[k] += v
    print(nodes, "nodes", total)
    assert all(total[k] > 0 for k in REQUIRED), total
    # the two quiescence branches are reached too (a repeated quiescence node, and one that would have stood pat at or
    # above beta): none of BRANCHES is left out
    assert total["hit_in_quiescence"] > 0 and total["hit_ahead_of_stand_pat_cut"] > 0
    assert set(REQUIRED) | {"hit_in_quiescence", "hit_ahead_of_stand_pat_cut"} == set(rp.BRANCHES)
    assert nodes < 100000


# ---- 6 ---------------------------------------------------------------------------------------------------------
def test_six_games_of_depth_two():
    """Both sides play depth 2 after four random opening plies (``gen_data``'s opening words of seed s, one game per
    seed 0 .. 5): four of the six games end by the fifth occurrence without the rule, at plies 47 .. 119, and with the
    rule three of those become decisive and one is still running at the cap; the two decisive games do not change.
    This is a CPU measurement of the FIXED-DEPTH search (``repetition_util.fixed_depth``), as it was first made: by
    consequence (a) and the _id contract the budgeted restatement finds the same minimax VALUE, but where root moves
    tie its move-to-front may keep another of them (``start_knights`` above), so its games are other games -- on
    these seeds five end by the fifth occurrence without the rule and none with it (measured once and not asserted, to keep
    this file quick)."""
    from chessrl_amd import gen_data as gd
    cap = 140

    def play(seed, rule):
        g = OracleGame()
        w = iter(int(x) for x in gd.opening_words(random.Random(seed), 1, 4)[0])
        ru.run_in_slot(g, lambda: next(w), max_moves=4)
        assert len(g) == 4
        while g.get_result() is None and len(g) < cap:
            assert g.move(uci(rp.fixed_depth(g, 2, rule)[0]))
        return len(g), g.get_result(), g.repetitions(), g.get_history()["moves"]

    off = [play(s, False) for s in range(6)]
    on = [play(s, True) for s in range(6)]
    print([x[:3] for x in off], [x[:3] for x in on])
    fifth_off = [s for s in range(6) if off[s][1:3] == (0, 5)]
    fifth_on = [s for s in range(6) if on[s][1:3] == (0, 5)]
    assert len(fifth_off) == 4 and [off[s][0] for s in fifth_off] == [53, 67, 47, 119]
    assert len(fifth_on) < len(fifth_off) and fifth_on == []
    assert [on[s][:2] for s in fifth_off] == [(cap, None), (133, 1), (47, 1), (109, 1)]
    for s in set(range(6)) - set(fifth_off):                # decisive before: unchanged, move for move
        assert off[s][1] in (1, -1) and off[s] == on[s]
    # the budgeted restatement itself, on the two shortest of the four: the fifth occurrence without the rule, a win with it
    for s, ends in ((2, (133, 1)), (3, (47, 1))):
        g = OracleGame()
        for m in off[s][3][:4]:
            assert g.move(m)
        h = g.get_copy()
        while g.get_result() is None and len(g) < cap:
            it.play_ply(g, 2, B)
        while h.get_result() is None and len(h) < cap:
            rp.play_ply(h, 2, B)
        assert (g.get_result(), g.repetitions()) == (0, 5) and (len(h), h.get_result()) == ends and h.repetitions() == 1


# ---- 7 ---------------------------------------------------------------------------------------------------------
def test_host_refusals_the_mode_key_and_the_header():
    from chessrl_amd import _lib
    from chessrl_amd import benchmark as bm
    from chessrl_amd import gen_data as gd
    from chessrl_amd.opponent import GameOpponent, MinimaxPlayer
    from chessrl_amd.searchmode import SearchMode
    p = MinimaxPlayer(False, 3, node_budget=300, repetition=True)
    assert (p.node_budget, p.repetition, p.ordering, MinimaxPlayer(True, node_budget=300).repetition,
            MinimaxPlayer(True).repetition) == (300, True, False, False, False)
    assert MinimaxPlayer(False, 3, ou.NODE_LIMIT, 0, 300, True).repetition is False    # positional calls are unchanged
    with pytest.raises(ValueError, match="repetition needs a node_budget"):
        MinimaxPlayer(True, repetition=True)
    with pytest.raises(ValueError, match="repetition needs a node_budget"):
        bm.benchmark(None, games=4, opponent_repetition=True, model=object())
    with pytest.raises(ValueError, match="repetition needs a node_budget"):
        gd.gen_data("unused.json", num_games=4, repetition=True)
    with pytest.raises(ValueError, match="repetition needs a node_budget"):
        _lib.Context.opponent_moves(None, [1], repetition=True)             # before any device call
    with pytest.raises(ValueError, match="repetition needs a node_budget"):
        _lib.Context.sim_reply_opponent(None, 0, 1000, 0, 0, 0, repetition=True)
    assert "opponent_repetition" in GameOpponent.__init__.__code__.co_varnames
    key = lambda **kw: SearchMode(reply=MinimaxPlayer(False, 3, node_budget=300, **kw)).key
    assert key(repetition=True) == SearchMode(reply=MinimaxPlayer(True, 3, node_budget=300, repetition=True)).key
    assert len({key(), key(repetition=True), key(ordering=True), key(ordering=True, repetition=True)}) == 4
    assert key(repetition=False) == key()
    mode = SearchMode(reply=p)
    assert mode.kind == "opponent" and [name for _, name in mode.plan] == [
        "phase_select_expand", "phase_reply_opponent", "phase_tower_s2"]
    text = open(os.path.join(ROOT, "include", "chessrl_hip.h")).read()
    for name in ("crl_opponent_moves_rep", "crl_sim_reply_opponent_rep"):
        assert name in _lib.SYMBOLS
        decl = re.search(r"int  %s\(.*?\);" % name, text, re.S).group(0)
        assert "int ordering, int repetition" in decl, name
    assert "#define CRL_ABI_VERSION 9" in text and _lib.ABI_VERSION == 9
    header = open(os.path.join(ROOT, "chessrl_amd", "csrc", "opponent.hpp")).read()
    assert "// REPETITION (" in header and "static_assert(ID || !REP" in header
    # the budgeted kernels are two templates over the six flags (REP among them), their legal shapes stated once
    for k in ("k_opponent_moves_id", "k_reply_opponent_id"):
        assert re.search(r"template <bool QS, bool ORD, bool REP, bool POS, bool SEL, bool EXC>\s*"
                         r"__global__ __launch_bounds__\(64\) void %s\(" % k, header), k
    assert re.search(r"constexpr bool opp_shape_legal\(bool QS, bool ORD,", header)
    assert re.search(r"static_assert\(opp_legal_shapes\(\) == 32,", header)
    assert "static_assert(opp_shape_legal(QS, ORD, REP, POS, SEL, EXC)" in header
