"""GPU: the built-in opponent's move ordering under a node budget (csrc/opponent.hpp ORDERING; the ORD shapes of the
``k_opponent_moves_id`` / ``k_reply_opponent_id`` kernel templates) against its CPU restatement (tests/ordering_util.py; its
preconditions and the case list are asserted without a GPU in tests/test_ordering_cpu.py).

1. move, score, node count, flag and completed depth of 16 roots and three set-up positions equal ``ordered`` in every
   case of ``ordering_util.CASES``; depth 0 and finished games; run to run;
2. ``ordering = 0`` through the new entry is ``crl_opponent_moves_id``, array for array;
3. ``push`` plays the ordered move: history and result as by ``crl_push_moves``;
4. the refusals;
5. ``MinimaxPlayer`` / ``GameOpponent``, ``benchmark`` (greedy and searching) and ``gen_data`` against CPU loops;
6. ``LockstepEngine(reply=MinimaxPlayer(node_budget=B, ordering=True))``: trees and reply statistics, graph and eager,
   and under a budget that cuts replies in iteration 1; ``ordering=False`` gives the trees of today's entry.
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
from tests import ordering_util as od
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


def depth_row(depth, case=None):
    """``depth`` in the 19 slots of the games (0 where ``case`` leaves the game out) and in the twin of slot 0."""
    row = np.zeros(64, np.int32)
    for i, (name, _) in enumerate(od.games()):
        row[i] = depth if case is None or od.in_case(name, case) else 0
    row[TWIN] = row[0]
    return row


# ---- 1 ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def finished_ctx():
    """The one context of sections 1 and 2: ``test_gpu_quiescence.slot_games`` with the mates of roots 8 and 9 played
    in slots 24 and 25."""
    ctx = tq.context64()
    mate = np.full(64, NO_MOVE, np.uint16)
    for s in MATED:
        mate[s] = ou.alphabeta(q.games()[s % 16][1], 1)[0]
    ctx.push_moves(mate)
    assert [int(r) for r in ctx.results()[list(MATED)]] == [1, -1]
    yield ctx
    ctx.close()


@pytest.mark.parametrize("depth,quiescence,budget", od.CASES)
def test_search_equals_the_restatement_and_repeats_itself(finished_ctx, depth, quiescence, budget):
    ctx = finished_ctx
    before = tg.state(ctx)
    case = (depth, quiescence, budget)
    row = depth_row(depth, case)
    row[list(MATED)] = depth
    got = ctx.opponent_moves(row, quiescence=quiescence, node_budget=budget, ordering=True)
    moves, scores, nodes, flags, done = got
    left_out = 0
    for i, ref in enumerate(od.reference(*case)[0]):
        name = od.games()[i][0]
        one = (int(moves[i]), int(scores[i]), int(nodes[i]), int(flags[i]), int(done[i]))
        print(name, case, move_to_uci(one[0]) if one[0] != NO_MOVE else None, one[1:], "restated", ref)
        if ref is None:                                         # a depth-0 slot among the searched ones
            left_out += 1
            ref = (NO_MOVE, 0, 0, 0, 0)
        assert one == ref, (name, case)
    assert left_out == (budget == od.UNREACHED)
    assert all(a[TWIN] == a[0] for a in got)
    idle = row == 0
    assert (moves[idle] == NO_MOVE).all() and not any(a[idle].any() for a in (scores, nodes, flags, done))
    for s in MATED:                                             # a finished game: skipped, nothing searched
        assert (moves[s], scores[s], nodes[s], flags[s], done[s]) == (NO_MOVE, 0, 0, ou.SKIPPED, 0)
    assert nodes.max() <= budget
    again = ctx.opponent_moves(row, quiescence=quiescence, node_budget=budget, ordering=True)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))   # the killers of one search do not reach the next
    assert tg.same_state(tg.state(ctx), before)    # nothing was pushed, no slot was touched


def test_an_unreached_budget_differs_from_the_unordered_kernel_in_the_nodes_alone(finished_ctx):
    ctx = finished_ctx
    case = od.CASES[-1]
    assert case == (3, 0, od.UNREACHED)
    row = depth_row(3, case)
    plain = ctx.opponent_moves(row, node_budget=od.UNREACHED)
    with_order = ctx.opponent_moves(row, node_budget=od.UNREACHED, ordering=True)
    for j in (0, 1, 3, 4):
        assert np.array_equal(plain[j], with_order[j])
    searched = row > 0
    assert (with_order[4][searched] == 3).all() and not with_order[3].any()
    print("nodes:", int(plain[2][:N_GAMES].sum()), "->", int(with_order[2][:N_GAMES].sum()))
    assert with_order[2][:N_GAMES].sum() <= 0.8 * plain[2][:N_GAMES].sum()


# ---- 2 ---------------------------------------------------------------------------------------------------------
def outputs():
    return (np.zeros(64, np.uint16), np.zeros(64, np.int32), np.zeros(64, np.int64), np.zeros(64, np.uint8),
            np.zeros(64, np.int32))


def test_ordering_zero_is_the_unordered_entry(finished_ctx):
    ctx = finished_ctx
    L, h = ctx._L, ctx._h
    for depth, quiescence, budget in ((3, 0, 150), (3, 2, 300)):
        row = depth_row(depth)
        row[list(MATED)] = depth
        old, new, on = outputs(), outputs(), outputs()
        assert L.crl_opponent_moves_id(h, ptr(row), quiescence, 0, budget, *[ptr(a) for a in old]) == 0
        assert L.crl_opponent_moves_ord(h, ptr(row), quiescence, 0, budget, 0, *[ptr(a) for a in new]) == 0
        assert L.crl_opponent_moves_ord(h, ptr(row), quiescence, 0, budget, 1, *[ptr(a) for a in on]) == 0
        assert all(np.array_equal(a, b) for a, b in zip(old, new))
        for i, ref in enumerate(it.reference(depth, quiescence, budget)[0]):
            assert tuple(int(a[i]) for a in new) == ref
        assert not all(np.array_equal(a, b) for a, b in zip(new, on))      # ordering = 1 is another kernel
        wrapped = ctx.opponent_moves(row, quiescence=quiescence, node_budget=budget, ordering=False)
        assert all(np.array_equal(a, b) for a, b in zip(old, wrapped))
    with pytest.raises(ValueError, match="ordering needs a node_budget"):
        ctx.opponent_moves(depth_row(2), ordering=True)


# ---- 3 ---------------------------------------------------------------------------------------------------------
def test_push_plays_the_ordered_move():
    from chessrl_amd import _lib
    games = tq.slot_games()
    games[FIFTH_SLOT] = tg.forced_fifth_game()
    a, b = _lib.Context(64, 1, max_plies=256), _lib.Context(64, 1, max_plies=256)
    tg.load_games(a, games)
    tg.load_games(b, games)
    row = depth_row(3)
    row[19:35] = 2                                              # roots 3 .. 15, 0 .. 2 once more, one ply shallower
    row[FIFTH_SLOT] = 2
    for ply in range(3):
        moves, _, nodes, flags, done = a.opponent_moves(row, push=True, quiescence=2, node_budget=300, ordering=True)
        running = b.results() == RESULT_NONE
        want_skip = (row > 0) & ~running
        assert ((flags == ou.SKIPPED) == want_skip).all() and (moves[want_skip] == NO_MOVE).all()
        assert (moves[(row > 0) & running] != NO_MOVE).all() and (moves[row == 0] == NO_MOVE).all()
        assert nodes.max() <= 300 and (done <= row).all()
        if ply == 0:
            for i in range(N_GAMES):
                assert (int(moves[i]), int(done[i])) == od.reference(3, 2, 300)[0][i][::4]
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


# ---- 4 ---------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from chessrl_amd import _lib
    ctx = tq.context64()
    before = tg.state(ctx)
    L, h = ctx._L, ctx._h
    moves, good = np.zeros(64, np.uint16), np.full(64, 1, np.int32)
    deep, negative = good.copy(), good.copy()
    deep[63], negative[5] = 6, -1
    call = lambda depths, Q, budget, ordering, out: L.crl_opponent_moves_ord(h, depths, Q, 1, budget, ordering, out,
                                                                             None, None, None, None)
    for ordering in (2, -1):
        assert call(ptr(good), 0, 100, ordering, ptr(moves)) == -1
    for budget in (0, -1):
        assert call(ptr(good), 0, budget, 1, ptr(moves)) == -1
    assert call(ptr(deep), 0, 100, 1, ptr(moves)) == -1 and call(ptr(negative), 0, 100, 1, ptr(moves)) == -1
    assert call(None, 0, 100, 1, ptr(moves)) == -1 and call(ptr(good), 0, 100, 1, None) == -1
    for bad in (-1, 7):
        assert call(ptr(good), bad, 100, 1, ptr(moves)) == -1
    assert tg.same_state(tg.state(ctx), before)                 # push = 1 in every call: nothing was launched
    with pytest.raises(_lib.HipLibraryError):
        ctx.opponent_moves(good, node_budget=0, ordering=True)
    import torch
    dev = torch.zeros(64, dtype=torch.int64, device="cuda:0").data_ptr()
    reply = lambda Q, budget, ordering, acc: L.crl_sim_reply_opponent_ord(h, dev, Q, budget, ordering, dev, dev, dev, acc)
    assert reply(0, 100, 2, dev) == -1 and reply(0, 0, 1, dev) == -1 and reply(7, 100, 1, dev) == -1
    assert reply(0, 100, 1, None) == -1                         # refused before any launch: nothing is read or written
    with pytest.raises(ValueError, match="ordering needs a node_budget"):
        ctx.sim_reply_opponent(dev, 1000, dev, dev, dev, ordering=True)
    # scores, nodes, flags and depths_done may be NULL
    assert L.crl_opponent_moves_ord(h, ptr(good), 2, 0, 100, 1, ptr(moves), None, None, None, None) == 0
    assert np.array_equal(moves, ctx.opponent_moves(good, quiescence=2, node_budget=100, ordering=True)[0])
    assert tg.same_state(tg.state(ctx), before)
    ctx.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------
PLIES = 24


def test_minimax_player_plays_the_ordered_move():
    from chessrl_amd.game import Game
    from chessrl_amd.opponent import MinimaxPlayer
    g = Game(board=q.KNOWN_ANSWER)
    for budget, limit in ((80, ou.NODE_LIMIT), (600, ou.NODE_LIMIT), (600, 30)):
        p = MinimaxPlayer(True, search_depth=3, node_limit=limit, quiescence=2, node_budget=budget, ordering=True)
        want = od.ordered(q.games()[16][1], 3, min(budget, limit), 2)
        assert p.best_move(g) == move_to_uci(want[0]) and p.last == want[1:4] and p.last_depth == want[4]
    g.free()


def test_game_opponent_one_move_at_a_time():
    from chessrl_amd.opponent import GameOpponent, MinimaxPlayer
    player = MinimaxPlayer(True, search_depth=1)
    g = GameOpponent(player_color=True, opponent_depth=3, opponent_budget=100, opponent_ordering=True)
    assert (g.opponent.search_depth, g.opponent.node_budget, g.opponent.ordering, player.ordering) == (3, 100, True, False)
    while g.get_result() is None and len(g) < PLIES:
        g.move(player.best_move(g))
    hist = g.get_history()
    g.free()
    c = OracleGame()
    while c.get_result() is None and len(c) < PLIES:
        ou.play_ply(c, 1)
        if c.get_result() is None:
            od.play_ply(c, 3, 100)
    assert (hist["moves"], hist["result"]) == (c.get_history()["moves"], c.get_result())
    assert len(hist["moves"]) >= PLIES


def test_benchmark_equals_the_cpu_loop(capsys):
    from chessrl_amd import benchmark as bm
    net = FakeNet(seed=5, prior_shift=29)
    out = bm.benchmark(None, games=4, opponent_depth=3, opponent_quiescence=2, opponent_budget=80, seed=7,
                       max_plies=PLIES, model=net.to("cuda:0"), log=True, opponent_ordering=True)
    assert "against the built-in opponent, depth <= 3 within 80 nodes per move, ordered" in capsys.readouterr().out.lower()
    colors = bm.game_colors(4, seed=7)
    agent = mcts_oracle.OracleAgent(net)
    want, results = [], []
    for c in colors:
        g = OracleGame()
        while g.get_result() is None and len(g) < PLIES:
            if g.turn == c:
                assert g.move(agent.best_move(g, real_game=True))
            else:
                od.play_ply(g, 3, 80, 2)
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
                       model=u.net().to("cuda:0"), opponent_ordering=True)
    want, results = [], []
    for white in colors:                                        # opponent_reply_util.cpu_games with the ordered opponent
        g = OracleGame()
        agent = od.ReplyAgentOrd(u.net(), depth, budget)
        if not white:
            od.play_ply(g, depth, budget)
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
    d = gd.gen_data(path, num_games=n, depth=2, node_budget=40, ordering=True, opening_plies=opening, seed=seed,
                    max_plies=max_plies)
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
            od.play_ply(g, player_depth if g.turn == is_white else game_depth, 40)
        if g.get_result() is None:                                  # still running after max_plies: dropped
            assert i not in saved
            continue
        hist = saved[i].get_history()
        assert hist["moves"] == g.get_history()["moves"]          # every move replayed legally in the oracle
        assert hist["result"] == g.get_result() and hist["player_color"] == is_white
    print("finished games:", sorted(saved))
    assert len(saved) >= 1


# ---- 6 ---------------------------------------------------------------------------------------------------------
SIMS, REPLY_DEPTH, BUDGET, TINY = 24, 3, 120, 3


def rows():
    assert len(u.roots()) == 16
    return tuple(range(16))


@functools.lru_cache(maxsize=None)
def tree(root, budget, quiescence, mode, ordering=True):
    """(SearchResult, log) of root ``root`` against the opponent of maximum depth 3 under ``budget``: computed once,
    never changed."""
    agent = (od.ReplyAgentOrd if ordering else it.ReplyAgentID)(u.net(), REPLY_DEPTH, budget, quiescence)
    r = mcts_oracle.search(u.roots()[root], agent, SIMS, noise=False, mode=mode)
    return r, tuple(agent.log)


def engine(budget, quiescence=0, ordering=True, **kw):
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.opponent import MinimaxPlayer
    reply = MinimaxPlayer(False, REPLY_DEPTH, quiescence=quiescence, node_budget=budget, ordering=ordering)
    eng = LockstepEngine(u.net().to("cuda:0"), n_games=len(rows()), max_sims=SIMS, reply=reply, numpy_promotion="nep50",
                         **kw)
    u.load_games(eng.ctx, [u.roots()[i] for i in rows()])
    return eng


def check_trees(eng, budget, quiescence, what, ordering=True):
    """The trees and the three per-game accumulators against the restatement; -> the logs of all replies."""
    eng.search(SIMS)
    rc = eng.root_children()
    stats = eng.reply_stats()
    assert len(stats) == 3                                      # unchanged in shape
    nodes, cuts, depth_sum = stats
    seen = []
    for k, i in enumerate(rows()):
        r, log = tree(i, budget, quiescence, "nep50", ordering)
        u.assert_tree_equal(rc, k, r, what)
        want = (sum(n for _, _, n, _, _ in log), sum(1 for e in log if e[3] == ou.CUT), sum(e[4] for e in log))
        assert (int(nodes[k]), int(cuts[k]), int(depth_sum[k])) == want, (what, i)
        assert all((e[3] == ou.CUT) == (e[4] < REPLY_DEPTH) and e[2] <= budget for e in log)
        seen += list(log)
    return seen


@pytest.mark.parametrize("graph", [True, False])
def test_reply_trees_equal_the_restatement(graph):
    eng = engine(BUDGET, use_graph=graph, steps_per_graph=8)
    assert [p for _, p in eng._plan] == ["phase_select_expand", "phase_reply_opponent", "phase_tower_s2"]
    seen = check_trees(eng, BUDGET, 0, ("graph", graph))
    eng.close()
    depths = [e[4] for e in seen]
    print("completed depths of the replies:", {d: depths.count(d) for d in sorted(set(depths))})
    assert {2, 3} <= set(depths)                                # some replies finished, some were cut in iteration 3
    # the order matters in these trees: the unordered opponent's replies cost other node counts
    plain = [e for i in rows() for e in tree(i, BUDGET, 0, "nep50", False)[1]]
    assert [e[2] for e in plain] != [e[2] for e in seen]


def test_replies_with_quiescence_and_a_budget_that_cuts_in_iteration_one():
    eng = engine(TINY, quiescence=2)
    seen = check_trees(eng, TINY, 2, ("tiny", TINY))
    eng.close()
    assert 0 in [e[4] for e in seen]                            # replies cut inside iteration 1: still a legal reply


def test_ordering_off_gives_the_trees_of_the_unordered_entry():
    eng = engine(BUDGET, ordering=False)
    assert eng.reply.ordering is False
    check_trees(eng, BUDGET, 0, ("unordered", BUDGET), ordering=False)
    eng.close()
