"""No GPU: the restatement of the built-in opponent's iterative deepening (tests/iterdeep_util.py) and what
tests/test_gpu_iterdeep.py leans on, asserted with the oracle alone.

1. with a budget nothing reaches, maximum depth 1 is ``opponent_util.alphabeta`` at depth 1;
2. with a budget nothing reaches, depths 2 and 3 give the minimax value and a move that attains it, and every iteration
   is the fixed-depth restatement run on the root with the previous best move in front: move, score and node sum;
3. on two small positions every budget from 1 to the whole search and one more: a legal move, ``min(B, total)`` nodes,
   a completed depth that never falls, and no cut exactly from the whole search on;
4. the set the GPU test runs reaches every branch of the rule (this test fixes that set);
5. the host-side refusals and ``SearchMode.key``.
"""
import pytest

from tests import iterdeep_util as it
from tests import opponent_util as ou
from tests import quiescence_util as q

BIG = 10 ** 9
SMALL3 = ("kpk", "kbkn", "kqk", "blocked", "king_shuffle", "fen_1", "fen_2")


def named(name):
    return dict(it.games())[name]


class Fronted(object):
    """``game`` with ``front`` moved to the front of its legal moves: the root of iteration i for the fixed-depth
    restatements (their children are plain copies, so nothing below the root changes)."""

    def __init__(self, game, front):
        self._game, self._front = game, front

    def legal_move_ids(self):
        moves = self._game.legal_move_ids()
        assert self._front in moves
        return [self._front] + [m for m in moves if m != self._front]

    def __getattr__(self, name):
        return getattr(self._game, name)


def plain_minimax(g, k, depth):
    """The value of ``g`` at search ply ``k`` of a depth-``depth`` search without pruning or order."""
    moves = g.legal_move_ids()
    over, mated = ou.terminal(g, len(moves))
    if over:
        return -(ou.MATE - k) if mated else 0
    if k == depth:
        return ou.evaluate(g)
    return max(-plain_minimax(ou.child(g, m), k + 1, depth) for m in moves)


def test_depth_one_is_the_fixed_depth_search():
    for name, g in it.games():
        assert it.iterdeep(g, 1, BIG) == ou.alphabeta(g, 1) + (1,), name


@pytest.mark.parametrize("depth", [2, 3])
def test_unreached_budget_gives_the_minimax_value(depth):
    for name, g in it.games():
        if depth == 3 and name not in SMALL3:
            continue
        move, score, nodes, flag, done = it.iterdeep(g, depth, BIG)
        assert (flag, done) == (0, depth), name
        assert score == ou.alphabeta(g, depth)[1] == ou.minimax(g, depth)[1], name
        assert move in g.legal_move_ids() and -plain_minimax(ou.child(g, move), 1, depth) == score, name


@pytest.mark.parametrize("depth,quiescence", [(2, 0), (3, 0), (2, 2), (3, 2)])
def test_every_iteration_is_the_fixed_depth_search_with_the_previous_best_in_front(depth, quiescence):
    moved = 0
    for name, g in it.games():
        if depth == 3 and name not in SMALL3:
            continue
        move, score, total, flag = q.alphabeta_q(g, 1, quiescence)
        assert flag == 0
        for i in range(2, depth + 1):
            moved += g.legal_move_ids()[0] != move
            move, score, nodes, flag = q.alphabeta_q(Fronted(g, move), i, quiescence)
            assert flag == 0
            total += nodes                                                 # the root is counted in every iteration
        assert it.iterdeep(g, depth, BIG, quiescence) == (move, score, total, 0, depth), name
        assert it.iterdeep(g, depth, total, quiescence) == (move, score, total, 0, depth), name
    assert moved > 0                                                       # the order did change somewhere


@pytest.mark.parametrize("name,depth,quiescence", [("fen_1", 3, 0), ("kpk", 2, 2)])
def test_every_budget_of_a_small_position(name, depth, quiescence):
    g = named(name)
    legal = g.legal_move_ids()
    whole = it.iterdeep(g, depth, BIG, quiescence)
    total, last_done = whole[2], 0
    assert 20 < total < 300 and whole[3:] == (0, depth)
    for budget in range(1, total + 2):
        move, score, nodes, flag, done = it.iterdeep(g, depth, budget, quiescence)
        assert move in legal and nodes == min(budget, total), budget
        assert last_done <= done <= depth, budget
        assert (flag == ou.CUT) == (done < depth) == (budget < total), budget
        if budget >= total:
            assert (move, score, nodes, flag, done) == whole
        last_done = done
    assert it.iterdeep(g, depth, 1, quiescence) == (legal[0], -ou.INF, 1, ou.CUT, 0)


def test_the_gpu_set_reaches_every_branch():
    total = it.new_counts()
    nodes, done_seen = 0, set()
    assert len(it.games()) == 19 and len(it.CASES) <= 9
    for depth, quiescence, budget in it.CASES:
        assert depth <= 3 and quiescence in (0, 2) and budget <= 600
        rows, counts = it.reference(depth, quiescence, budget)
        for (name, g), (move, score, n, flag, done) in zip(it.games(), rows):
            assert move in g.legal_move_ids() and n <= budget and (flag == ou.CUT) == (done < depth), name
            done_seen.add((depth, done))
        nodes += sum(r[2] for r in rows)
        for k, v in counts.items():
            total[k] += v
    print(nodes, "nodes", total)
    assert all(total[k] > 0 for k in it.BRANCHES), total
    assert nodes < 50000
    # (D, depth_done): cuts in iterations 1, 2 and 3 (depth_done 0, 1, 2) and slots that finish every maximum depth
    assert done_seen == {(d, done) for d in (1, 2, 3) for done in range(d + 1)}
    name, depth, quiescence, budget = it.LAST_NODE
    assert (depth, quiescence, budget) in it.CASES
    assert it.iterdeep(named(name), depth, budget, quiescence)[2:] == (budget, 0, depth)
    assert it.iterdeep(named(name), depth, budget - 1, quiescence)[3] == ou.CUT


def test_host_refusals_and_the_mode_key():
    from chessrl_amd import benchmark as bm
    from chessrl_amd import gen_data as gd
    from chessrl_amd.opponent import MinimaxPlayer
    from chessrl_amd.searchmode import SearchMode
    p = MinimaxPlayer(False, 3, node_budget=300)
    assert (p.search_depth, p.node_budget, p.last_depth, MinimaxPlayer(True).node_budget) == (3, 300, None, None)
    for bad in (0, -5):
        with pytest.raises(ValueError, match="node_budget"):
            MinimaxPlayer(True, node_budget=bad)
        with pytest.raises(ValueError, match="opponent_budget"):
            bm.benchmark(None, games=4, opponent_budget=bad, model=object())
        with pytest.raises(ValueError, match="node_budget"):
            gd.gen_data("unused.json", num_games=4, node_budget=bad)
    key = lambda **kw: SearchMode(reply=MinimaxPlayer(False, 3, **kw)).key
    assert key(node_budget=300) == SearchMode(reply=MinimaxPlayer(True, 3, node_budget=300)).key
    assert len({key(), key(node_budget=300), key(node_budget=301)}) == 3
    mode = SearchMode(reply=p)
    assert mode.kind == "opponent" and [name for _, name in mode.plan] == [
        "phase_select_expand", "phase_reply_opponent", "phase_tower_s2"]
