"""GPU: the search against the built-in opponent -- ``LockstepEngine(reply=MinimaxPlayer)``, ``k_reply_opponent`` of
csrc/opponent.hpp -- against its CPU restatement (tests/opponent_reply_util.py; its preconditions are asserted
without a GPU in tests/test_opponent_reply_cpu.py).

1. trees equal the restatement: depth 1 and 2, eager and graph replay, both numpy promotion modes; run to run;
2. the node limit: trees, node counts and cuts per game;
3. mixed depths per slot;
4. no evaluation of S1;
5. the three policy formats give one tree;
6. the stored reply is the move the opponent plays from that board;
7. ``benchmark(sims=N)`` equals the CPU game loop; ``sims=0`` is the greedy benchmark;
8. ``SelfPlayTree(reply=)`` / ``Agent.best_move(reply=)``.
Every comparison is exact: integers, float64 value sums by bit pattern, float32 priors by value.
"""
import numpy as np
import pytest

from oracle import mcts_oracle
from oracle.chess_oracle import OracleGame, move_to_uci
from tests import opponent_reply_util as u
from tests import opponent_util as ou
from tests.test_opponent_reply_cpu import node_limit_for

pytestmark = pytest.mark.gpu

G = 16
NO_MOVE, RESULT_NONE = 0xFFFF, 2
ARRAYS = ("nchild", "visits", "root_visits", "moves", "replies", "values", "priors")


def engine(depth, sims, roots=None, limit=ou.NODE_LIMIT, evaluator=None, **kw):
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.opponent import MinimaxPlayer
    roots = list(range(G)) if roots is None else roots
    reply = MinimaxPlayer(False, search_depth=depth, node_limit=limit) if depth else None
    eng = LockstepEngine(evaluator if evaluator is not None else u.net().to("cuda:0"), n_games=len(roots),
                         max_sims=sims, reply=reply, **kw)
    u.load_games(eng.ctx, [u.roots()[i] for i in roots])
    return eng


def same_arrays(a, b):
    return all(np.array_equal(a[k].view(np.uint64) if k == "values" else a[k], b[k].view(np.uint64) if k == "values" else b[k])
               for k in ARRAYS)


# ---- 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,sims,mode,graph", [(1, 60, "nep50", False), (1, 60, "legacy", True),
                                                   (2, 40, "nep50", True), (2, 40, "nep50", False)])
def test_trees_equal_the_restatement(depth, sims, mode, graph):
    eng = engine(depth, sims, numpy_promotion=mode, use_graph=graph, steps_per_graph=8)
    assert [p for _, p in eng._plan] == ["phase_select_expand", "phase_reply_opponent", "phase_tower_s2"]
    eng.search(sims)
    rc = eng.root_children()
    assert eng.ctx.counters()["sims"] == G * sims
    nodes, cuts = eng.reply_stats()
    for i in range(G):
        r, log = u.tree(i, depth, ou.NODE_LIMIT, sims, mode)
        u.assert_tree_equal(rc, i, r, (depth, mode, graph))
        assert (int(nodes[i]), int(cuts[i])) == (sum(n for _, _, n, _ in log), 0), i
    eng.search(sims)                                        # the same search once more: identical arrays
    assert same_arrays(rc, eng.root_children())
    again = eng.reply_stats()
    assert np.array_equal(nodes, again[0]) and np.array_equal(cuts, again[1])      # (search_begin cleared them)
    eng.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------
def test_node_limit_trees_and_statistics():
    sims, limit = 48, node_limit_for()
    rows = list(range(u.N_PREFIX, G))                       # the two starts and the six set-up roots
    eng = engine(2, sims, roots=rows, limit=limit, numpy_promotion="nep50")
    eng.search(sims)
    rc = eng.root_children()
    nodes, cuts = eng.reply_stats()
    assert nodes.dtype == np.int64 and cuts.dtype == np.int32
    any_cut = 0
    for k, i in enumerate(rows):
        r, log = u.tree(i, 2, limit, sims, "nep50")
        u.assert_tree_equal(rc, k, r, ("limit", limit))
        n_cut = sum(1 for _, _, _, flag in log if flag == ou.CUT)
        print("root", i, "nodes", int(nodes[k]), "cuts", int(cuts[k]), "restated", sum(n for _, _, n, _ in log), n_cut)
        assert (int(nodes[k]), int(cuts[k])) == (sum(n for _, _, n, _ in log), n_cut), i
        any_cut += n_cut
    mid = rows.index(u.MIDDLEGAME)
    assert 0 < cuts[mid] < sims and any_cut >= cuts[mid]
    eng.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------
def test_mixed_depths_per_slot():
    sims = 40
    eng = engine(1, sims, numpy_promotion="nep50")
    depths = np.array([1 + (i & 1) for i in range(G)], np.int32)
    with pytest.raises(ValueError):
        eng.set_reply_depths(depths[:5])
    with pytest.raises(ValueError):
        eng.set_reply_depths(np.where(depths == 2, 6, 1))
    with pytest.raises(ValueError):
        eng.set_reply_depths(depths - 1)
    eng.set_reply_depths(depths)
    eng.search(sims)
    rc = eng.root_children()
    for i in range(G):
        r, _ = u.tree(i, int(depths[i]), ou.NODE_LIMIT, sims, "nep50")
        u.assert_tree_equal(rc, i, r, ("mixed", int(depths[i])))
    eng.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------
class Counting(object):
    """planes -> (policy, value) through the net, counting the calls and remembering what was handed in."""

    def __init__(self, net):
        self.net, self.calls, self.seen = net, 0, set()

    def __call__(self, planes):
        self.calls += 1
        self.seen.add(planes.data_ptr())
        return self.net(planes)


def test_s1_is_never_evaluated():
    sims, out = 30, {}
    for depth in (0, 1):                                    # 0: the net's reply
        ev = Counting(u.net().to("cuda:0"))
        eng = engine(depth, sims, roots=[0, 3, 8, 9], evaluator=ev, use_graph=False)
        eng.search(sims)
        eng.ctx.sync()
        out[depth] = (ev.calls, eng.planes_s1.data_ptr() in ev.seen, eng.planes_s2.data_ptr() in ev.seen)
        eng.close()
    assert out[0] == (1 + 2 * sims, True, True)
    assert out[1] == (1 + sims, False, True)
    assert out[0][0] - out[1][0] == sims


# ---- 5 ---------------------------------------------------------------------------------------------------------
def test_policy_formats_give_one_tree():
    from chessrl_amd.model import ChessModel
    model = ChessModel(blocks=2, filters=64, seed=3)
    sims, out = 40, []
    for legal, raw in ((False, False), (True, False), (True, None)):
        eng = engine(1, sims, evaluator=model, legal_priors=legal, raw_priors=raw, steps_per_graph=8)
        assert eng.legal_priors == legal and eng.raw_priors == (raw is None)
        eng.search(sims)
        first = eng.root_children()
        chosen = np.where(first["nchild"] > 0, np.maximum(first["visits"].argmax(1), 0), -1).astype(np.int32)
        bm, am = eng.advance(chosen)
        eng.search(sims)
        out.append((first, bm, am, eng.root_children(), eng.ctx.counters(), eng.reply_stats()))
        eng.close()
    a = out[0]
    assert a[0]["nchild"].sum() > 100 and (a[2] != NO_MOVE).sum() >= 8
    for b in out[1:]:
        assert same_arrays(a[0], b[0]) and same_arrays(a[3], b[3])
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert {k: int(v) for k, v in a[4].items()} == {k: int(v) for k, v in b[4].items()}
        assert np.array_equal(a[5][0], b[5][0]) and np.array_equal(a[5][1], b[5][1])


# ---- 6 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2])
def test_the_stored_reply_is_the_real_reply(depth):
    from chessrl_amd import _lib
    from chessrl_amd.engine import choose_children
    sims = 40
    eng = engine(depth, sims, numpy_promotion="nep50")
    eng.search(sims)
    rc = eng.root_children()
    plies = eng.ctx.records(with_moves=False)[1]
    chosen = choose_children(rc["visits"], rc["nchild"], rc["root_visits"], plies, noise=False)
    assert (chosen >= 0).all()
    for i in range(G):
        assert chosen[i] == u.tree(i, depth, ou.NODE_LIMIT, sims, "nep50")[0].chosen
    bm, am = eng.advance(chosen)
    after = eng.ctx.results()
    ctx = _lib.Context(G, 1, max_plies=256)
    u.load_games(ctx, list(u.roots()))
    assert ctx.push_moves(bm).all()
    res = ctx.results()
    moves, _, _, flags = ctx.opponent_moves(np.full(G, depth, np.int32), push=True)
    assert np.array_equal(moves, am)
    ended = am == NO_MOVE
    assert ended.any() and not ended.all()
    assert (res[ended] != RESULT_NONE).all() and (flags[ended] == ou.SKIPPED).all() and (res[~ended] == RESULT_NONE).all()
    assert np.array_equal(ctx.results(), after)             # the two-ply advance left the same games behind
    assert np.array_equal(ctx.records()[1], eng.ctx.records()[1])
    ctx.close()
    eng.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------
BENCH_SEED, BENCH_PLIES, BENCH_SIMS = 7, 10, 16


@pytest.mark.parametrize("depth", [1, 2])
def test_benchmark_with_search_equals_the_cpu_loop(depth):
    from chessrl_amd import benchmark as bm
    from chessrl_amd.engine import resolve_numpy_promotion
    colors = bm.game_colors(4, seed=BENCH_SEED)
    assert True in colors and False in colors               # both colours are played
    out = bm.benchmark(None, games=4, opponent_depth=depth, sims=BENCH_SIMS, seed=BENCH_SEED, max_plies=BENCH_PLIES,
                       model=u.net().to("cuda:0"))
    want, results = u.cpu_games(tuple(colors), depth, BENCH_SIMS, BENCH_PLIES, resolve_numpy_promotion("auto"))
    assert out["games"] == want
    assert {k: out[k] for k in ("played", "won", "drawn")} == bm.tally(colors, results)
    assert all(len(g) >= BENCH_PLIES for g in want)


def test_benchmark_without_search_is_the_greedy_benchmark(capsys):
    from chessrl_amd import benchmark as bm
    net = u.net()
    plies = 12
    out = bm.benchmark(None, games=4, opponent_depth=2, seed=BENCH_SEED, max_plies=plies, model=net.to("cuda:0"), sims=0,
                       log=True)
    assert "MCTS" not in capsys.readouterr().out
    colors = bm.game_colors(4, seed=BENCH_SEED)
    agent = mcts_oracle.OracleAgent(net)
    want, results = [], []
    for c in colors:
        g = OracleGame()
        while g.get_result() is None and len(g) < plies:
            if g.turn == c:
                assert g.move(agent.best_move(g, real_game=True))
            else:
                ou.play_ply(g, 2)
        want.append(g.get_history()["moves"])
        results.append(g.get_result())
    assert out["games"] == want
    assert {k: out[k] for k in ("played", "won", "drawn")} == bm.tally(colors, results)
    bm.benchmark(None, games=4, opponent_depth=1, seed=BENCH_SEED, max_plies=2, model=net.to("cuda:0"), sims=4, log=True)
    assert "agent: MCTS, 4 simulations per move" in capsys.readouterr().out


# ---- 8 ---------------------------------------------------------------------------------------------------------
def test_drop_in_tree_and_agent():
    from chessrl_amd.agent import Agent
    from chessrl_amd.engine import resolve_numpy_promotion
    from chessrl_amd.game import Game
    from chessrl_amd.mctree import SelfPlayTree
    from chessrl_amd.opponent import MinimaxPlayer
    sims, mode = 40, resolve_numpy_promotion("auto")
    agent = Agent(True, model=u.net().to("cuda:0"))
    player = MinimaxPlayer(False, 2)
    for i in (3, u.MIDDLEGAME):
        src = u.roots()[i]
        game = Game(board=u.FENS[i - u.FEN0]) if i >= u.FEN0 else Game()
        for k in range(len(src)):
            assert game.move(move_to_uci(src.board.move_stack[k].m))
        r, _ = u.tree(i, 2, ou.NODE_LIMIT, sims, mode)
        tree = SelfPlayTree(game, reply=player)
        assert tree.search_move(agent, sims, noise=False, ai_move=True) == r.moves
        kids = tree.root.children
        assert tree.root.visits == r.root_visits
        assert [c.visits for c in kids] == r.visits and [c.move for c in kids] == r.child_moves
        assert [c.reply or "00000" for c in kids] == r.child_replies
        assert [np.float64(c.value).view(np.uint64) for c in kids] == [np.float64(v).view(np.uint64) for v in r.values]
        assert [c.prior for c in kids] == [np.float32(p) for p in r.priors]
        eng = agent.engine_for(sims, reply=player)
        assert eng is tree._engine and eng.reply is player
        assert agent.engine_for(sims, reply=MinimaxPlayer(True, 2)) is eng          # cached per (sims, depth, limit)
        with pytest.raises(ValueError, match="reply= cannot continue a Node"):
            SelfPlayTree(kids[0]).search_move(agent, sims, noise=False)
        with pytest.raises(ValueError, match="reply= cannot continue a Node"):
            SelfPlayTree(kids[0], reply=player)
        np.random.seed(11)                                  # best_move searches with noise, from the global stream
        first = agent.best_move(game, real_game=False, max_iters=sims, ai_move=False, reply=player)
        want = mcts_oracle.search(src, u.ReplyAgent(u.net(), 2, log_greedy=False), sims, noise=True, mode=mode,
                                  rng=np.random.RandomState(11))
        assert first == want.moves[0]
        game.free()
