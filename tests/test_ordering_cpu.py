"""No GPU: the restatement of the built-in opponent's move ordering (tests/ordering_util.py; csrc/opponent.hpp ORDERING)
and what tests/test_gpu_ordering.py leans on, asserted with the oracle alone.

1. with a budget nothing reaches, move, score, flag and completed depth are those of ``iterdeep_util.iterdeep`` on every
   root (depth 3: the roots the iterdeep test uses there), and the score is the pruning-free minimax value;
2. the order pays: at depth 3 fewer nodes in sum than ``iterdeep``, with and without quiescence, and at most 0.8 of
   them over the 18 roots other than ``218_moves`` (no claim per root);
3. on two small positions every budget from 1 to the whole search and one more: a legal move, ``min(B, total)`` nodes,
   a completed depth that never falls, and no cut exactly from the whole search on;
4. the set the GPU test runs reaches every branch of the rule (this test fixes that set);
5. the host-side refusals, ``SearchMode.key``, the symbol list and the header.
"""
import os
import re

import pytest

from tests import iterdeep_util as it
from tests import opponent_util as ou
from tests import ordering_util as od
from tests import quiescence_util as q
from tests.test_iterdeep_cpu import SMALL3, plain_minimax

BIG = 10 ** 9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def named(name):
    return dict(od.games())[name]


@pytest.mark.parametrize("depth,quiescence", [(2, 0), (3, 0), (2, 2), (3, 2)])
def test_unreached_budget_gives_the_answer_of_the_unordered_search(depth, quiescence):
    fewer = 0
    for name, g in od.games():
        if depth == 3 and name not in SMALL3:
            continue
        move, score, nodes, flag, done = od.ordered(g, depth, BIG, quiescence)
        want = it.iterdeep(g, depth, BIG, quiescence)
        assert (move, score, flag, done) == want[:2] + want[3:] and (flag, done) == (0, depth), name
        if quiescence == 0:
            assert score == ou.minimax(g, depth)[1] and -plain_minimax(ou.child(g, move), 1, depth) == score, name
        elif name in SMALL3:
            assert score == q.minimax_q(g, depth, quiescence)[1], name
        assert od.ordered(g, depth, nodes, quiescence) == (move, score, nodes, 0, depth), name   # its last permitted node
        fewer += nodes < want[2]
    assert fewer > 0                                                       # the order did change the count somewhere


def sums(quiescence, names):
    """(nodes of ``iterdeep``, nodes of ``ordered``) at maximum depth 3 over ``names``, every answer compared."""
    plain = with_order = 0
    for name in names:
        g = named(name)
        a, b = it.iterdeep(g, 3, BIG, quiescence), od.ordered(g, 3, BIG, quiescence)
        assert a[:2] + a[3:] == b[:2] + b[3:] == a[:2] + (0, 3), name
        plain, with_order = plain + a[2], with_order + b[2]
    return plain, with_order


def test_the_order_pays_at_depth_three():
    all_roots = [name for name, _ in od.games()]
    others = [name for name in all_roots if name != od.BIG_ROOT]
    assert len(all_roots) == 19 and len(others) == 18
    plain, with_order = sums(0, others)
    print("depth 3, 18 roots:", plain, "->", with_order)
    assert with_order < plain and with_order <= 0.8 * plain
    big = sums(0, [od.BIG_ROOT])
    print("depth 3,", od.BIG_ROOT, big)
    assert plain + big[0] > with_order + big[1]                            # (3, 0) over all 19
    # (3, 2): the roots the quiescence test searches to depth 3, so the test stays quick
    small = [name for name in all_roots if name in q.DEPTH3 or name.startswith("fen_")]
    plain_q, with_order_q = sums(2, small)
    print("depth 3, quiescence 2,", len(small), "roots:", plain_q, "->", with_order_q)
    assert len(small) >= 8 and with_order_q < plain_q


@pytest.mark.parametrize("name,depth,quiescence", [("fen_1", 3, 0), ("kpk", 2, 2)])
def test_every_budget_of_a_small_position(name, depth, quiescence):
    g = named(name)
    legal = g.legal_move_ids()
    whole = od.ordered(g, depth, BIG, quiescence)
    total, last_done = whole[2], 0
    assert 20 < total < 300 and whole[3:] == (0, depth)
    for budget in range(1, total + 2):
        move, score, nodes, flag, done = od.ordered(g, depth, budget, quiescence)
        assert move in legal and nodes == min(budget, total), budget
        assert last_done <= done <= depth, budget
        assert (flag == ou.CUT) == (done < depth) == (budget < total), budget
        if budget >= total:
            assert (move, score, nodes, flag, done) == whole
        last_done = done
    assert od.ordered(g, depth, 1, quiescence) == (legal[0], -ou.INF, 1, ou.CUT, 0)


def test_the_gpu_set_reaches_every_branch():
    total = od.new_counts()
    nodes = 0
    assert len(od.games()) == 19 and len(od.CASES) <= 9
    for case in od.CASES:
        depth, quiescence, budget = case
        assert depth <= 3 and quiescence in (0, 2) and (budget <= 600 or budget == od.UNREACHED)
        rows, counts = od.reference(*case)
        unordered = it.reference(*case)[0] if budget != od.UNREACHED else None
        differ = 0
        for i, ((name, g), row) in enumerate(zip(od.games(), rows)):
            assert (row is None) == (not od.in_case(name, case)) == (budget == od.UNREACHED and name == od.BIG_ROOT)
            if row is None:
                continue
            move, score, n, flag, done = row
            assert move in g.legal_move_ids() and n <= budget and (flag == ou.CUT) == (done < depth), name
            if budget == od.UNREACHED:
                assert (flag, done) == (0, depth), name
            else:
                differ += row != unordered[i]
        nodes += sum(r[2] for r in rows if r is not None)
        for k, v in counts.items():
            total[k] += v
        print(case, "rows that differ from the unordered search:", differ, counts)
        if budget != od.UNREACHED:
            assert (differ == 0) == (budget == 1), case                    # a real test of the order, except at B = 1
    print(nodes, "nodes", total)
    assert all(total[k] > 0 for k in od.BRANCHES), total
    assert nodes < 50000
    # the in-check quiescence node sets its killers only where there is quiescence
    assert all(od.reference(*c)[1]["killer_set_in_check_quiescence"] == 0 for c in od.CASES if c[1] == 0)


def test_host_refusals_the_mode_key_and_the_header():
    from chessrl_amd import _lib
    from chessrl_amd import benchmark as bm
    from chessrl_amd import gen_data as gd
    from chessrl_amd.opponent import MinimaxPlayer
    from chessrl_amd.searchmode import SearchMode
    p = MinimaxPlayer(False, 3, node_budget=300, ordering=True)
    assert (p.node_budget, p.ordering, MinimaxPlayer(True, node_budget=300).ordering, MinimaxPlayer(True).ordering) \
        == (300, True, False, False)
    assert MinimaxPlayer(False, 3, ou.NODE_LIMIT, 0, 300).ordering is False     # positional calls are unchanged
    with pytest.raises(ValueError, match="ordering needs a node_budget"):
        MinimaxPlayer(True, ordering=True)
    with pytest.raises(ValueError, match="opponent_ordering"):
        bm.benchmark(None, games=4, opponent_ordering=True, model=object())
    with pytest.raises(ValueError, match="ordering"):
        gd.gen_data("unused.json", num_games=4, ordering=True)
    key = lambda **kw: SearchMode(reply=MinimaxPlayer(False, 3, node_budget=300, **kw)).key
    assert key(ordering=True) == SearchMode(reply=MinimaxPlayer(True, 3, node_budget=300, ordering=True)).key
    assert len({key(), key(ordering=True), SearchMode(reply=MinimaxPlayer(False, 3)).key}) == 3
    assert key(ordering=False) == key()
    mode = SearchMode(reply=p)
    assert mode.kind == "opponent" and [name for _, name in mode.plan] == [
        "phase_select_expand", "phase_reply_opponent", "phase_tower_s2"]
    text = open(os.path.join(ROOT, "include", "chessrl_hip.h")).read()
    for name in ("crl_opponent_moves_ord", "crl_sim_reply_opponent_ord"):
        assert name in _lib.SYMBOLS
        decl = re.search(r"int  %s\(.*?\);[^\n]*" % name, text, re.S).group(0)
        assert "int ordering" in decl and "stockfish.py:14-21" in decl, name
    assert "#define CRL_ABI_VERSION 9" in text and _lib.ABI_VERSION == 9
