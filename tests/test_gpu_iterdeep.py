"""GPU: the built-in opponent's iterative deepening under a node budget (csrc/opponent.hpp ITERATIVE DEEPENING;
the ``k_opponent_moves_id`` / ``k_reply_opponent_id`` kernel templates) against its CPU restatement
(tests/iterdeep_util.py; its preconditions and the case list are asserted without a GPU in tests/test_iterdeep_cpu.py).

1. move, score, node count, flag and completed depth of 16 roots and three set-up positions equal ``iterdeep`` in every
   case of ``iterdeep_util.CASES``; depth 0 and finished games; run to run;
2. ``push`` equals ``crl_push_moves`` of the returned move;
3. the refusals;
4. ``MinimaxPlayer`` / ``GameOpponent``, ``benchmark`` (greedy and searching) and ``gen_data`` against CPU loops;
5. ``LockstepEngine(reply=MinimaxPlayer(node_budget=B))``: trees and reply statistics, graph and eager, and under a
   budget that cuts replies in iteration 1; ``SelfPlayTree(reply=)`` / ``Agent.best_move(reply=)``;
6. ``node_budget=None`` is the fixed-depth kernel: the trees of the existing entry.
Integer work only: every comparison is exact.
"""
import ctypes
import functools
import random

import numpy as np
import pytest

from oracle import mcts_oracle
from oracle.chess_oracle import OracleGame, move_to_uci
from oracle.fakenet import FakeNet
from tests import iterdeep_util as it
from tests import opponent_reply_util as u
from tests import opponent_util as ou
from tests import quiescence_util as q
from tests import rollout_util as ru
from tests import test_gpu_opponent as tg
from tests import test_gpu_quiescence as tq

pytestmark = pytest.mark.gpu

NO_MOVE, RESULT_NONE = 0xFFFF, 2
N_GAMES = tq.N_GAMES                           # slots 0 .. 15 the private roots, 16 .. 18 the set-up positions
TWIN, FIFTH_SLOT = tg.TWIN, tg.FIFTH_SLOT      # slot 37 holds the root of slot 0 once more
MATED = (24, 25)                               # slots that hold roots 8 and 9: the back-rank mates are played there


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def depth_row(depth):
    row = np.zeros(64, np.int32)
    row[:N_GAMES] = depth
    row[TWIN] = depth
    return row


# ---- 1 ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def finished_ctx():
    """The one context of section 1: ``test_gpu_quiescence.slot_games`` with the mates of roots 8 and 9 played in
    slots 24 and 25."""
    ctx = tq.context64()
    mate = np.full(64, NO_MOVE, np.uint16)
    for s in MATED:
        mate[s] = ou.alphabeta(q.games()[s % 16][1], 1)[0]
    ctx.push_moves(mate)
    assert [int(r) for r in ctx.results()[list(MATED)]] == [1, -1]
    yield ctx
    ctx.close()


@pytest.mark.parametrize("depth,quiescence,budget", it.CASES)
def test_search_equals_the_restatement_and_repeats_itself(finished_ctx, depth, quiescence, budget):
    ctx = finished_ctx
    before = tg.state(ctx)
    row = depth_row(depth)
    row[list(MATED)] = depth
    got = ctx.opponent_moves(row, quiescence=quiescence, node_budget=budget)
    moves, scores, nodes, flags, done = got
    for i, ref in enumerate(it.reference(depth, quiescence, budget)[0]):
        name = it.games()[i][0]
        one = (int(moves[i]), int(scores[i]), int(nodes[i]), int(flags[i]), int(done[i]))
        print(name, (depth, quiescence, budget), move_to_uci(one[0]), one[1:], "restated", ref)
        assert one == ref, (name, depth, quiescence, budget)
    assert all(a[TWIN] == a[0] for a in got)
    idle = row == 0
    assert (moves[idle] == NO_MOVE).all() and not any(a[idle].any() for a in (scores, nodes, flags, done))
    for s in MATED:                                             # a finished game: skipped, nothing searched
        assert (moves[s], scores[s], nodes[s], flags[s], done[s]) == (NO_MOVE, 0, 0, ou.SKIPPED, 0)
    assert nodes.max() <= budget
    again = ctx.opponent_moves(row, quiescence=quiescence, node_budget=budget)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    assert tg.same_state(tg.state(ctx), before)    # nothing was pushed, no slot was touched


def test_the_node_limit_caps_the_budget_and_no_budget_is_the_old_entry(finished_ctx):
    ctx = finished_ctx
    row = depth_row(2)
    capped = ctx.opponent_moves(row, node_limit=63, node_budget=10 ** 6)
    assert all(np.array_equal(a, b) for a, b in zip(capped, ctx.opponent_moves(row, node_budget=63)))
    assert all(np.array_equal(a, b) for a, b in zip(ctx.opponent_moves(row, node_budget=None), ctx.opponent_moves(row)))
    assert len(ctx.opponent_moves(row)) == 4


# ---- 2 ---------------------------------------------------------------------------------------------------------
def test_push_equals_push_moves_of_the_returned_move():
    from chessrl_amd import _lib
    games = tq.slot_games()
    games[FIFTH_SLOT] = tg.forced_fifth_game()
    a, b = _lib.Context(64, 1, max_plies=256), _lib.Context(64, 1, max_plies=256)
    tg.load_games(a, games)
    tg.load_games(b, games)
    row = depth_row(2)
    row[19:35] = 3                                              # roots 3 .. 15, 0 .. 2 once more, one ply deeper
    row[FIFTH_SLOT] = 2
    for ply in range(3):
        moves, _, nodes, flags, done = a.opponent_moves(row, push=True, quiescence=2, node_budget=100)
        running = b.results() == RESULT_NONE
        want_skip = (row > 0) & ~running
        assert ((flags == ou.SKIPPED) == want_skip).all() and (moves[want_skip] == NO_MOVE).all()
        assert (moves[(row > 0) & running] != NO_MOVE).all() and (moves[row == 0] == NO_MOVE).all()
        assert nodes.max() <= 100 and (done <= row).all()
        if ply == 0:
            for i in range(N_GAMES):
                assert (int(moves[i]), int(done[i])) == it.reference(2, 2, 100)[0][i][::4]
        ok = b.push_moves(moves)
        assert (ok == (moves != NO_MOVE)).all()
        assert tg.same_state(tg.state(a), tg.state(b))
        # the forced line: running after one ply, drawn by the fifth occurrence after two, skipped in the third
        assert (int(a.results()[FIFTH_SLOT]), int(flags[FIFTH_SLOT])) == ((RESULT_NONE, 0), (0, 0), (0, ou.SKIPPED))[ply]
    res = a.results()
    assert res[8] == 1 and res[9] == -1                         # the back-rank mates were delivered
    assert a.records()[1][FIFTH_SLOT] == len(tg.FORCED_FIFTH) + 2
    a.close()
    b.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from chessrl_amd import _lib
    ctx = tq.context64()
    before = tg.state(ctx)
    L, h = ctx._L, ctx._h
    moves, good = np.zeros(64, np.uint16), np.full(64, 1, np.int32)
    deep, negative = good.copy(), good.copy()
    deep[63], negative[5] = 6, -1
    call = lambda depths, Q, budget, out: L.crl_opponent_moves_id(h, depths, Q, 1, budget, out, None, None, None, None)
    for budget in (0, -1):
        assert call(ptr(good), 0, budget, ptr(moves)) == -1
    assert call(ptr(deep), 0, 100, ptr(moves)) == -1 and call(ptr(negative), 0, 100, ptr(moves)) == -1
    assert call(None, 0, 100, ptr(moves)) == -1 and call(ptr(good), 0, 100, None) == -1
    for bad in (-1, 7):
        assert call(ptr(good), bad, 100, ptr(moves)) == -1
    assert tg.same_state(tg.state(ctx), before)
    with pytest.raises(_lib.HipLibraryError):
        ctx.opponent_moves(good, node_budget=0)
    import torch
    dev = torch.zeros(64, dtype=torch.int64, device="cuda:0").data_ptr()
    for kw in (dict(node_budget=0), dict(node_budget=100, quiescence=7), dict(node_budget=100, dev_depth_sum=None)):
        kw.setdefault("dev_depth_sum", dev)                     # refused before any launch: nothing is read or written
        with pytest.raises(_lib.HipLibraryError):
            ctx.sim_reply_opponent(dev, 1000, dev, dev, dev, **kw)
    # scores, nodes, flags and depths_done may be NULL
    assert L.crl_opponent_moves_id(h, ptr(good), 2, 0, 100, ptr(moves), None, None, None, None) == 0
    assert np.array_equal(moves, ctx.opponent_moves(good, quiescence=2, node_budget=100)[0])
    assert tg.same_state(tg.state(ctx), before)
    ctx.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------
PLIES = 24


def test_minimax_player_reports_the_completed_depth():
    from chessrl_amd.game import Game
    from chessrl_amd.opponent import MinimaxPlayer
    g = Game(board=q.KNOWN_ANSWER)
    for budget, limit in ((80, ou.NODE_LIMIT), (600, ou.NODE_LIMIT), (600, 30)):
        p = MinimaxPlayer(True, search_depth=3, node_limit=limit, quiescence=2, node_budget=budget)
        want = it.iterdeep(q.games()[16][1], 3, min(budget, limit), 2)
        assert p.best_move(g) == move_to_uci(want[0]) and p.last == want[1:4] and p.last_depth == want[4]
    plain = MinimaxPlayer(True, search_depth=1)
    assert plain.best_move(g) == "e2e5" and plain.last_depth is None
    g.free()


def test_game_opponent_one_move_at_a_time():
    from chessrl_amd.opponent import GameOpponent, MinimaxPlayer
    player = MinimaxPlayer(True, search_depth=1)
    g = GameOpponent(player_color=True, opponent_depth=3, opponent_budget=100)
    assert (g.opponent.search_depth, g.opponent.node_budget, player.node_budget) == (3, 100, None)
    depths = set()
    while g.get_result() is None and len(g) < PLIES:
        g.move(player.best_move(g))
        depths.add(g.opponent.last_depth)
    hist = g.get_history()
    g.free()
    c = OracleGame()
    while c.get_result() is None and len(c) < PLIES:
        ou.play_ply(c, 1)
        if c.get_result() is None:
            it.play_ply(c, 3, 100)
    assert (hist["moves"], hist["result"]) == (c.get_history()["moves"], c.get_result())
    assert len(hist["moves"]) >= PLIES and depths <= {1, 2, 3}


def test_benchmark_equals_the_cpu_loop(capsys):
    from chessrl_amd import benchmark as bm
    net = FakeNet(seed=5, prior_shift=29)
    out = bm.benchmark(None, games=4, opponent_depth=3, opponent_quiescence=2, opponent_budget=80, seed=7,
                       max_plies=PLIES, model=net.to("cuda:0"), log=True)
    assert "built-in opponent, depth <= 3 within 80 nodes per move, quiescence 2 (not Stockfish, no Elo)" \
        in capsys.readouterr().out
    colors = bm.game_colors(4, seed=7)
    agent = mcts_oracle.OracleAgent(net)
    want, results = [], []
    for c in colors:
        g = OracleGame()
        while g.get_result() is None and len(g) < PLIES:
            if g.turn == c:
                assert g.move(agent.best_move(g, real_game=True))
            else:
                it.play_ply(g, 3, 80, 2)
        want.append(g.get_history()["moves"])
        results.append(g.get_result())
    assert out["games"] == want
    assert {k: out[k] for k in ("played", "won", "drawn")} == bm.tally(colors, results)
    assert True in colors and False in colors                   # both colours were played


def test_benchmark_with_search_equals_the_cpu_loop():
    from chessrl_amd import benchmark as bm
    from chessrl_amd.engine import resolve_numpy_promotion
    from oracle.chess_oracle import NULL_MOVE
    sims, plies, depth, budget = 12, 8, 3, 60
    mode = resolve_numpy_promotion("auto")
    colors = bm.game_colors(4, seed=7)
    out = bm.benchmark(None, games=4, opponent_depth=depth, opponent_budget=budget, sims=sims, seed=7, max_plies=plies,
                       model=u.net().to("cuda:0"))
    want, results = [], []
    for white in colors:                                        # opponent_reply_util.cpu_games with the budgeted opponent
        g = OracleGame()
        agent = it.ReplyAgentID(u.net(), depth, budget)
        if not white:
            it.play_ply(g, depth, budget)
        while g.get_result() is None and len(g) < plies:
            r = mcts_oracle.search(g, agent, sims, noise=False, mode=mode)
            assert g.move(r.child_moves[r.chosen])
            if r.child_replies[r.chosen] != NULL_MOVE:
                assert g.move(r.child_replies[r.chosen])
        want.append(g.get_history()["moves"])
        results.append(g.get_result())
    assert out["games"] == want
    assert {k: out[k] for k in ("played", "won", "drawn")} == bm.tally(colors, results)


def test_gen_data_equals_the_cpu_loop(tmp_path):
    from chessrl_amd import gen_data as gd
    path = str(tmp_path / "games.json")
    n, opening, seed, max_plies = 4, 4, 0, 120
    d = gd.gen_data(path, num_games=n, depth=2, node_budget=40, opening_plies=opening, seed=seed, max_plies=max_plies)
    draws = gd.draw_games(n, depth=2, random_dep=False, seed=seed)
    words = gd.opening_words(random.Random(seed), n, opening)
    saved = {rec.game_id: rec for rec in d.games}
    assert len(saved) == len(d)
    for i in range(n):
        is_white, game_depth, player_depth = draws[i]
        g = OracleGame()
        w = iter(int(x) for x in words[i])
        ru.run_in_slot(g, lambda: next(w), max_moves=opening)       # (StopIteration if the words did not suffice)
        assert len(g) == opening
        while g.get_result() is None and len(g) < max_plies:
            it.play_ply(g, player_depth if g.turn == is_white else game_depth, 40)
        if g.get_result() is None:                                  # still running after max_plies: dropped
            assert i not in saved
            continue
        hist = saved[i].get_history()
        assert hist["moves"] == g.get_history()["moves"]          # every move replayed legally in the oracle
        assert hist["result"] == g.get_result() and hist["player_color"] == is_white
    print("finished games:", sorted(saved))
    assert len(saved) >= 1


# ---- 5 ---------------------------------------------------------------------------------------------------------
ROWS = (0, 3, 8, 10, 11, 12, u.MIDDLEGAME, 15)
SIMS, REPLY_DEPTH, BUDGET, TINY = 24, 3, 120, 3


@functools.lru_cache(maxsize=None)
def tree(root, budget, quiescence, mode):
    """(SearchResult, log) of root ``root`` against the opponent of maximum depth 3 under ``budget``: computed once,
    never changed."""
    agent = it.ReplyAgentID(u.net(), REPLY_DEPTH, budget, quiescence)
    r = mcts_oracle.search(u.roots()[root], agent, SIMS, noise=False, mode=mode)
    return r, tuple(agent.log)


def engine(budget, quiescence=0, **kw):
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.opponent import MinimaxPlayer
    reply = MinimaxPlayer(False, search_depth=REPLY_DEPTH, quiescence=quiescence, node_budget=budget)
    eng = LockstepEngine(u.net().to("cuda:0"), n_games=len(ROWS), max_sims=SIMS, reply=reply, numpy_promotion="nep50",
                         **kw)
    u.load_games(eng.ctx, [u.roots()[i] for i in ROWS])
    return eng


def check_trees(eng, budget, quiescence, what):
    """The trees and the three per-game accumulators against the restatement; -> the completed depths of all replies."""
    eng.search(SIMS)
    rc = eng.root_children()
    nodes, cuts, depth_sum = eng.reply_stats()
    seen = []
    for k, i in enumerate(ROWS):
        r, log = tree(i, budget, quiescence, "nep50")
        u.assert_tree_equal(rc, k, r, what)
        want = (sum(n for _, _, n, _, _ in log), sum(1 for e in log if e[3] == ou.CUT), sum(e[4] for e in log))
        assert (int(nodes[k]), int(cuts[k]), int(depth_sum[k])) == want, (what, i)
        assert all((e[3] == ou.CUT) == (e[4] < REPLY_DEPTH) and e[2] <= budget for e in log)
        seen += [e[4] for e in log]
    return seen


@pytest.mark.parametrize("graph", [True, False])
def test_reply_trees_equal_the_restatement(graph):
    eng = engine(BUDGET, use_graph=graph, steps_per_graph=8)
    assert [p for _, p in eng._plan] == ["phase_select_expand", "phase_reply_opponent", "phase_tower_s2"]
    seen = check_trees(eng, BUDGET, 0, ("graph", graph))
    eng.close()
    print("completed depths of the replies:", {d: seen.count(d) for d in sorted(set(seen))})
    assert {2, 3} <= set(seen)                                  # some replies finished, some were cut in iteration 3


def test_replies_with_quiescence_and_a_budget_that_cuts_in_iteration_one():
    eng = engine(TINY, quiescence=2)
    seen = check_trees(eng, TINY, 2, ("tiny", TINY))
    eng.close()
    assert 0 in seen                                            # replies cut inside iteration 1: still a legal reply


def test_drop_in_tree_and_agent():
    from chessrl_amd.agent import Agent
    from chessrl_amd.engine import resolve_numpy_promotion
    from chessrl_amd.game import Game
    from chessrl_amd.mctree import SelfPlayTree
    from chessrl_amd.opponent import MinimaxPlayer
    mode = resolve_numpy_promotion("auto")
    agent = Agent(True, model=u.net().to("cuda:0"))
    player = MinimaxPlayer(False, REPLY_DEPTH, node_budget=BUDGET)
    for i in (3, u.MIDDLEGAME):
        src = u.roots()[i]
        game = Game(board=u.FENS[i - u.FEN0]) if i >= u.FEN0 else Game()
        for k in range(len(src)):
            assert game.move(move_to_uci(src.board.move_stack[k].m))
        r, _ = tree(i, BUDGET, 0, mode)
        t = SelfPlayTree(game, reply=player)
        assert t.search_move(agent, SIMS, noise=False, ai_move=True) == r.moves
        kids = t.root.children
        assert t.root.visits == r.root_visits
        assert [c.visits for c in kids] == r.visits and [c.move for c in kids] == r.child_moves
        assert [c.reply or "00000" for c in kids] == r.child_replies
        assert [np.float64(c.value).view(np.uint64) for c in kids] == [np.float64(v).view(np.uint64) for v in r.values]
        np.random.seed(11)                                  # best_move searches with noise, from the global stream
        first = agent.best_move(game, real_game=False, max_iters=SIMS, ai_move=False, reply=player)
        want = mcts_oracle.search(src, it.ReplyAgentID(u.net(), REPLY_DEPTH, BUDGET), SIMS, noise=True, mode=mode,
                                  rng=np.random.RandomState(11))
        assert first == want.moves[0]
        game.free()


def test_agent_engine_cache_keys_on_the_budget():
    from chessrl_amd.agent import Agent
    from chessrl_amd.opponent import MinimaxPlayer
    agent = Agent(True, model=u.net().to("cuda:0"))
    plain = agent.engine_for(8, reply=MinimaxPlayer(False, 2))
    budgeted = agent.engine_for(8, reply=MinimaxPlayer(False, 2, node_budget=50))
    assert budgeted is not plain and (plain.reply.node_budget, budgeted.reply.node_budget) == (None, 50)
    assert agent.engine_for(8, reply=MinimaxPlayer(True, 2, node_budget=50)) is budgeted
    assert agent.engine_for(8, reply=MinimaxPlayer(True, 2, node_budget=51)) is not budgeted


# ---- 6 ---------------------------------------------------------------------------------------------------------
def test_no_budget_launches_the_fixed_depth_kernel():
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.opponent import MinimaxPlayer
    eng = LockstepEngine(u.net().to("cuda:0"), n_games=len(ROWS), max_sims=SIMS,
                         reply=MinimaxPlayer(False, search_depth=1, node_budget=None), numpy_promotion="nep50")
    u.load_games(eng.ctx, [u.roots()[i] for i in ROWS])
    eng.search(SIMS)
    rc = eng.root_children()
    stats = eng.reply_stats()
    assert len(stats) == 2 and not hasattr(eng, "reply_depth_sum")
    for k, i in enumerate(ROWS):
        r, log = u.tree(i, 1, ou.NODE_LIMIT, SIMS, "nep50")
        u.assert_tree_equal(rc, k, r, ("fixed", i))
        assert (int(stats[0][k]), int(stats[1][k])) == (sum(n for _, _, n, _ in log), 0)
    eng.close()
