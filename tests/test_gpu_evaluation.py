"""GPU: the built-in opponent's positional evaluation (csrc/opponent.hpp EVALUATION; ``opp_evaluate_positional``, the
POS shapes of the ``k_opponent_moves_id`` / ``k_reply_opponent_id`` kernel templates and ``k_opponent_evaluate``) against its CPU restatement
(tests/evaluation_util.py; the restatement itself is held to the header's table without a GPU in
tests/test_evaluation_cpu.py).

1. ``opponent_evaluate`` of both kinds equals the restatement on the 28 roots of ``repetition_util`` and on the set-up
   positions (pawn structure, rook files, the bishop pair, shelter, every king attacker, nine queens, black to move,
   bare kings), and on the colour flip of each;
2. ``opponent_moves(evaluation="positional")``: move, score, node count, flag and completed depth equal the
   restatement in every case of ``evaluation_util.CASES`` (every kernel shape; budgets that cut and one nothing
   reaches); depth 0 and finished games; run to run; ``push``;
3. ``evaluation = 0`` through the new entries is the ``_rep`` entry, array for array; the refusals change nothing;
4. ``LockstepEngine(reply=MinimaxPlayer(False, 2, node_budget=120, evaluation="positional"))``: trees and reply
   statistics against ``oracle.mcts_oracle.search``, graph and eager;
5. ``MinimaxPlayer`` / ``GameOpponent``, ``benchmark`` and ``gen_data`` against CPU loops;
6. the loop of ``tools/opponent_match.py`` against a CPU loop with the two evaluations on their sides.
Integer work only: every comparison is exact.
"""
import ctypes
import functools
import importlib
import random

import numpy as np
import pytest

from oracle import mcts_oracle
from oracle.chess_oracle import OracleGame, move_to_uci
from oracle.fakenet import FakeNet
from tests import evaluation_util as ev
from tests import opponent_reply_util as u
from tests import opponent_util as ou
from tests import repetition_util as rp
from tests import rollout_util as ru
from tests import test_gpu_opponent as tg
from tests import test_gpu_repetition as tr

pytestmark = pytest.mark.gpu

NO_MOVE, RESULT_NONE = 0xFFFF, 2
N_GAMES = tr.N_GAMES                           # slots 0 .. 27: the roots, as in test_gpu_repetition
TWIN, MATED, MAX_PLIES = tr.TWIN, tr.MATED, tr.MAX_PLIES


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---- 1 ---------------------------------------------------------------------------------------------------------
def test_static_evaluation_equals_the_restatement():
    from chessrl_amd import _lib
    games = [g for _, g in ev.static_games()]
    games += [ev.flip_game(g) for g in games]
    n = len(games)
    assert n == 2 * (28 + len(ev.SETUPS)) and n <= 128
    ctx = _lib.Context(128, 1, max_plies=MAX_PLIES)
    tg.load_games(ctx, games + [games[i % 16] for i in range(128 - n)])
    before = tg.state(ctx)
    names = [name for name, _ in ev.static_games()]
    names += [name + " flipped" for name in names]
    for kind, restated in sorted(ev.EVALUATIONS.items()):
        got = ctx.opponent_evaluate(kind)
        for i, g in enumerate(games):
            print(kind, names[i], int(got[i]), "restated", restated(g))
            assert int(got[i]) == restated(g), (kind, names[i])
        assert np.array_equal(got[:n // 2], got[n // 2:n])                  # a colour flip keeps the score
        assert np.array_equal(got, ctx.opponent_evaluate(kind))
    assert np.array_equal(ctx.opponent_evaluate(), ctx.opponent_evaluate("material"))
    assert not np.array_equal(ctx.opponent_evaluate("positional"), ctx.opponent_evaluate("material"))
    nine = names.index("nine_queens")
    assert 9 * 900 < abs(int(ctx.opponent_evaluate("positional")[nine])) <= ev.BOUND
    assert tg.same_state(tg.state(ctx), before)
    # a window: the scores are window-relative
    ctx.set_window(28, 16)
    assert np.array_equal(ctx.opponent_evaluate("positional"), [ev.positional(g) for g in games[28:44]])
    ctx.set_window(0, 128)
    # the refusals
    scores = np.zeros(128, np.int32)
    L, h = ctx._L, ctx._h
    assert L.crl_opponent_evaluate(h, 2, ptr(scores)) == -1 and L.crl_opponent_evaluate(h, -1, ptr(scores)) == -1
    assert L.crl_opponent_evaluate(h, 1, None) == -1
    assert L.crl_opponent_evaluate(h, 1, ptr(scores)) == 0
    assert np.array_equal(scores, ctx.opponent_evaluate("positional"))
    with pytest.raises(ValueError, match="evaluation must be one of"):
        ctx.opponent_evaluate("pst")
    ctx.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------
def depth_row(depth, case=None):
    """``depth`` in the 28 slots of the games (0 where ``case`` leaves the game out) and in the twin of slot 0."""
    row = np.zeros(64, np.int32)
    for i, (name, _) in enumerate(ev.games()):
        row[i] = depth if case is None or ev.in_case(name, case) else 0
    row[TWIN] = row[0]
    return row


@pytest.fixture(scope="module")
def finished_ctx():
    """``test_gpu_repetition.slot_games`` with the mates of roots 8 and 9 played in MATED."""
    ctx = tr.context64()
    mate = np.full(64, NO_MOVE, np.uint16)
    for s, i in zip(MATED, (8, 9)):
        mate[s] = ou.alphabeta(ev.games()[i][1], 1)[0]
    ctx.push_moves(mate)
    assert [int(r) for r in ctx.results()[list(MATED)]] == [1, -1]
    yield ctx
    ctx.close()


@pytest.mark.parametrize("depth,quiescence,budget,ordering,repetition", ev.CASES)
def test_search_equals_the_restatement_and_repeats_itself(finished_ctx, depth, quiescence, budget, ordering, repetition):
    ctx = finished_ctx
    assert [n for n, _ in ev.games()] == [n for n, _ in rp.games()]
    before = tg.state(ctx)
    case = (depth, quiescence, budget, ordering, repetition)
    row = depth_row(depth, case)
    row[list(MATED)] = depth
    kw = dict(quiescence=quiescence, node_budget=budget, ordering=ordering, repetition=repetition)
    got = ctx.opponent_moves(row, evaluation="positional", **kw)
    moves, scores, nodes, flags, done = got
    left_out = other = 0
    material = ev.reference(*case, evaluation="material")
    for i, ref in enumerate(ev.reference(*case)):
        name = ev.games()[i][0]
        one = (int(moves[i]), int(scores[i]), int(nodes[i]), int(flags[i]), int(done[i]))
        print(name, case, move_to_uci(one[0]) if one[0] != NO_MOVE else None, one[1:], "restated", ref)
        if ref is None:                                         # a depth-0 slot among the searched ones
            left_out += 1
            ref = (NO_MOVE, 0, 0, 0, 0)
        elif ref != material[i]:
            other += 1
        assert one == ref, (name, case)
        assert abs(one[1]) <= ev.BOUND or abs(one[1]) >= ou.MATE - 11 or one[1] == -ou.INF    # the header's bound
    assert left_out == (1 if budget == ev.UNREACHED else 0)
    assert other >= 14                                          # the evaluation matters in these searches
    assert all(a[TWIN] == a[0] for a in got)
    idle = row == 0
    assert (moves[idle] == NO_MOVE).all() and not any(a[idle].any() for a in (scores, nodes, flags, done))
    for s in MATED:                                             # a finished game: skipped, nothing searched
        assert (moves[s], scores[s], nodes[s], flags[s], done[s]) == (NO_MOVE, 0, 0, ou.SKIPPED, 0)
    assert nodes.max() <= budget
    again = ctx.opponent_moves(row, evaluation="positional", **kw)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))   # nothing of one search reaches the next
    assert tg.same_state(tg.state(ctx), before)                 # nothing was pushed, no slot was touched


def test_push_plays_the_move():
    from chessrl_amd import _lib
    games = tr.slot_games()
    a, b = _lib.Context(64, 1, max_plies=MAX_PLIES), _lib.Context(64, 1, max_plies=MAX_PLIES)
    tg.load_games(a, games)
    tg.load_games(b, games)
    row = depth_row(3)
    row[28:37] = 2
    case = (3, 2, 200, True, True)
    assert case in ev.CASES
    for ply in range(3):
        moves, _, nodes, flags, done = a.opponent_moves(row, push=True, quiescence=2, node_budget=200, ordering=True,
                                                        repetition=True, evaluation="positional")
        running = b.results() == RESULT_NONE
        want_skip = (row > 0) & ~running
        assert ((flags == ou.SKIPPED) == want_skip).all() and (moves[want_skip] == NO_MOVE).all()
        assert (moves[(row > 0) & running] != NO_MOVE).all() and (moves[row == 0] == NO_MOVE).all()
        assert nodes.max() <= 200 and (done <= row).all()
        if ply == 0:
            for i in range(N_GAMES):
                assert (int(moves[i]), int(done[i])) == ev.reference(*case)[i][::4]
        ok = b.push_moves(moves)
        assert (ok == (moves != NO_MOVE)).all()
        assert tg.same_state(tg.state(a), tg.state(b))
    a.close()
    b.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------
def test_material_through_the_new_entry_is_the_rep_entry(finished_ctx):
    ctx = finished_ctx
    L, h = ctx._L, ctx._h
    for depth, quiescence, budget, ordering, repetition in ((3, 0, 300, 0, 0), (3, 0, 300, 1, 1), (2, 0, 63, 0, 1),
                                                            (3, 2, 200, 1, 0)):
        row = depth_row(depth)
        row[list(MATED)] = depth
        old, new, on = tr.outputs(), tr.outputs(), tr.outputs()
        assert L.crl_opponent_moves_rep(h, ptr(row), quiescence, 0, budget, ordering, repetition,
                                        *[ptr(a) for a in old]) == 0
        assert L.crl_opponent_moves_ev(h, ptr(row), quiescence, 0, budget, ordering, repetition, 0,
                                       *[ptr(a) for a in new]) == 0
        assert L.crl_opponent_moves_ev(h, ptr(row), quiescence, 0, budget, ordering, repetition, 1,
                                       *[ptr(a) for a in on]) == 0
        assert all(np.array_equal(a, b) for a, b in zip(old, new))
        assert not all(np.array_equal(a, b) for a, b in zip(old, on))
        wrapped = ctx.opponent_moves(row, quiescence=quiescence, node_budget=budget, ordering=bool(ordering),
                                     repetition=bool(repetition), evaluation="material")
        assert all(np.array_equal(a, b) for a, b in zip(old, wrapped))
        default = ctx.opponent_moves(row, quiescence=quiescence, node_budget=budget, ordering=bool(ordering),
                                     repetition=bool(repetition))
        assert all(np.array_equal(a, b) for a, b in zip(old, default))
    with pytest.raises(ValueError, match="evaluation needs a node_budget"):
        ctx.opponent_moves(depth_row(2), evaluation="positional")


def test_refusals_change_nothing():
    from chessrl_amd import _lib
    ctx = tr.context64()
    before = tg.state(ctx)
    L, h = ctx._L, ctx._h
    moves, good = np.zeros(64, np.uint16), np.full(64, 1, np.int32)
    deep, negative = good.copy(), good.copy()
    deep[63], negative[5] = 6, -1
    call = lambda depths, Q, budget, ordering, rep, kind, out: L.crl_opponent_moves_ev(
        h, depths, Q, 1, budget, ordering, rep, kind, out, None, None, None, None)
    for kind in (2, -1):
        assert call(ptr(good), 0, 100, 0, 0, kind, ptr(moves)) == -1
    for rep in (2, -1):
        assert call(ptr(good), 0, 100, 0, rep, 1, ptr(moves)) == -1
    for ordering in (2, -1):
        assert call(ptr(good), 0, 100, ordering, 1, 1, ptr(moves)) == -1
    for budget in (0, -1):
        assert call(ptr(good), 0, budget, 1, 1, 1, ptr(moves)) == -1
    assert call(ptr(deep), 0, 100, 0, 0, 1, ptr(moves)) == -1 and call(ptr(negative), 0, 100, 0, 0, 1, ptr(moves)) == -1
    assert call(None, 0, 100, 0, 0, 1, ptr(moves)) == -1 and call(ptr(good), 0, 100, 0, 0, 1, None) == -1
    for bad in (-1, 7):
        assert call(ptr(good), bad, 100, 0, 0, 1, ptr(moves)) == -1
    assert tg.same_state(tg.state(ctx), before)                 # push = 1 in every call: nothing was launched
    with pytest.raises(_lib.HipLibraryError):
        ctx.opponent_moves(good, node_budget=0, evaluation="positional")
    import torch
    dev = torch.zeros(64, dtype=torch.int64, device="cuda:0").data_ptr()
    reply = lambda Q, budget, ordering, rep, kind, acc: L.crl_sim_reply_opponent_ev(h, dev, Q, budget, ordering, rep,
                                                                                    kind, dev, dev, dev, acc)
    assert reply(0, 100, 0, 0, 2, dev) == -1 and reply(0, 100, 0, 0, -1, dev) == -1
    assert reply(0, 100, 0, 2, 1, dev) == -1 and reply(0, 100, 2, 1, 1, dev) == -1 and reply(0, 0, 0, 1, 1, dev) == -1
    assert reply(7, 100, 0, 1, 1, dev) == -1
    assert reply(0, 100, 0, 1, 1, None) == -1                   # refused before any launch: nothing is read or written
    with pytest.raises(ValueError, match="evaluation needs a node_budget"):
        ctx.sim_reply_opponent(dev, 1000, dev, dev, dev, evaluation="positional")
    # scores, nodes, flags and depths_done may be NULL
    assert L.crl_opponent_moves_ev(h, ptr(good), 2, 0, 100, 1, 1, 1, ptr(moves), None, None, None, None) == 0
    assert np.array_equal(moves, ctx.opponent_moves(good, quiescence=2, node_budget=100, ordering=True, repetition=True,
                                                    evaluation="positional")[0])
    assert tg.same_state(tg.state(ctx), before)
    ctx.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------
SIMS, REPLY_DEPTH, BUDGET = 10, 2, 120


@functools.lru_cache(maxsize=None)
def reply_roots():
    """Four roots: a random prefix, the start position, the middlegame and a root with a shuffle behind it."""
    roots = u.roots()
    return (roots[5], roots[u.N_PREFIX], roots[u.MIDDLEGAME], rp.table_game("start_knights"))


@functools.lru_cache(maxsize=None)
def tree(root, evaluation, mode="nep50"):
    """(SearchResult, log) of root ``root`` against the opponent of maximum depth 2 under BUDGET: computed once."""
    agent = ev.ReplyAgentEv(u.net(), REPLY_DEPTH, BUDGET, evaluation=evaluation)
    r = mcts_oracle.search(reply_roots()[root], agent, SIMS, noise=False, mode=mode)
    return r, tuple(agent.log)


@pytest.mark.parametrize("graph", [True, False])
def test_reply_trees_equal_the_restatement(graph):
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.opponent import MinimaxPlayer
    reply = MinimaxPlayer(False, REPLY_DEPTH, node_budget=BUDGET, evaluation="positional")
    eng = LockstepEngine(u.net().to("cuda:0"), n_games=len(reply_roots()), max_sims=SIMS, reply=reply,
                         numpy_promotion="nep50", use_graph=graph, steps_per_graph=5)
    u.load_games(eng.ctx, list(reply_roots()))
    assert eng.reply.evaluation == "positional"
    assert [p for _, p in eng._plan] == ["phase_select_expand", "phase_reply_opponent", "phase_tower_s2"]
    eng.search(SIMS)
    rc = eng.root_children()
    nodes, cuts, depth_sum = eng.reply_stats()
    for i in range(len(reply_roots())):
        r, log = tree(i, "positional")
        u.assert_tree_equal(rc, i, r, ("graph", graph))
        want = (sum(n for _, _, n, _, _ in log), sum(1 for e in log if e[3] == ou.CUT), sum(e[4] for e in log))
        assert (int(nodes[i]), int(cuts[i]), int(depth_sum[i])) == want, (graph, i)
        assert all((e[3] == ou.CUT) == (e[4] < REPLY_DEPTH) and e[2] <= BUDGET for e in log)
    eng.close()
    changed = [i for i in range(len(reply_roots())) if tree(i, "positional")[1] != tree(i, "material")[1]]
    print("roots whose reply logs differ from the material opponent's:", changed)
    assert changed                                              # the evaluation reaches the trees


# ---- 5 ---------------------------------------------------------------------------------------------------------
PLIES = 16


def test_minimax_player_plays_the_move_of_the_evaluation():
    from chessrl_amd.game import Game
    from chessrl_amd.opponent import MinimaxPlayer
    fen = dict(ev.SETUPS)["middlegame"]
    g = Game(board=fen)
    root = ev.from_fen(fen)
    for budget, limit, ordering, repetition in ((80, ou.NODE_LIMIT, False, False), (300, ou.NODE_LIMIT, True, True),
                                                (300, 30, False, True)):
        p = MinimaxPlayer(True, search_depth=3, node_limit=limit, quiescence=2, node_budget=budget, ordering=ordering,
                          repetition=repetition, evaluation="positional")
        want = ev.search(root, 3, min(budget, limit), 2, ordering, repetition)
        assert p.best_move(g) == move_to_uci(want[0]) and p.last == want[1:4] and p.last_depth == want[4]
    g.free()


def test_game_opponent_one_move_at_a_time():
    from chessrl_amd.opponent import GameOpponent, MinimaxPlayer
    player = MinimaxPlayer(True, search_depth=1)
    g = GameOpponent(player_color=True, opponent_depth=2, opponent_budget=100, opponent_evaluation="positional")
    assert (g.opponent.search_depth, g.opponent.node_budget, g.opponent.evaluation, player.evaluation) == (
        2, 100, "positional", "material")
    while g.get_result() is None and len(g) < PLIES:
        g.move(player.best_move(g))
    hist = g.get_history()
    g.free()
    c = OracleGame()
    while c.get_result() is None and len(c) < PLIES:
        ou.play_ply(c, 1)
        if c.get_result() is None:
            ev.play_ply(c, 2, 100)
    assert (hist["moves"], hist["result"]) == (c.get_history()["moves"], c.get_result())
    assert len(hist["moves"]) >= PLIES


def test_benchmark_equals_the_cpu_loop(capsys):
    from chessrl_amd import benchmark as bm
    net = FakeNet(seed=5, prior_shift=29)
    out = bm.benchmark(None, games=4, opponent_depth=2, opponent_quiescence=2, opponent_budget=80, seed=7,
                       max_plies=PLIES, model=net.to("cuda:0"), log=True, opponent_ordering=True,
                       opponent_repetition=True, opponent_evaluation="positional")
    said = capsys.readouterr().out.lower()
    assert ("against the built-in opponent, depth <= 2 within 80 nodes per move, ordered, repetition-aware, "
            "quiescence 2, positional evaluation (not stockfish, no elo)" in said)
    colors = bm.game_colors(4, seed=7)
    agent = mcts_oracle.OracleAgent(net)
    want, results = [], []
    for c in colors:
        g = OracleGame()
        while g.get_result() is None and len(g) < PLIES:
            if g.turn == c:
                assert g.move(agent.best_move(g, real_game=True))
            else:
                ev.play_ply(g, 2, 80, 2, ordering=True, repetition=True)
        want.append(g.get_history()["moves"])
        results.append(g.get_result())
    assert out["games"] == want
    assert {k: out[k] for k in ("played", "won", "drawn")} == bm.tally(colors, results)
    assert True in colors and False in colors                   # both colours were played
    # the line of a run without the evaluation is what it was
    bm.benchmark(None, games=2, opponent_depth=2, opponent_budget=20, seed=7, max_plies=2, model=net.to("cuda:0"),
                 log=True)
    assert "within 20 nodes per move (not stockfish, no elo)" in capsys.readouterr().out.lower()


def test_gen_data_equals_the_cpu_loop(tmp_path):
    from chessrl_amd import gen_data as gd
    path = str(tmp_path / "games.json")
    n, opening, seed, max_plies, budget = 4, 4, 0, 24, 60
    d = gd.gen_data(path, num_games=n, depth=2, node_budget=budget, evaluation="positional", opening_plies=opening,
                    seed=seed, max_plies=max_plies)
    draws = gd.draw_games(n, depth=2, random_dep=False, seed=seed)
    words = gd.opening_words(random.Random(seed), n, opening)
    saved = {rec.game_id: rec for rec in d.games}
    for i in range(n):
        is_white, game_depth, player_depth = draws[i]
        g = OracleGame()
        w = iter(int(x) for x in words[i])
        ru.run_in_slot(g, lambda: next(w), max_moves=opening)
        assert len(g) == opening
        while g.get_result() is None and len(g) < max_plies:
            ev.play_ply(g, player_depth if g.turn == is_white else game_depth, budget)
        if g.get_result() is None:                                  # still running after max_plies: dropped
            assert i not in saved
            continue
        hist = saved[i].get_history()
        assert hist["moves"] == g.get_history()["moves"]
        assert hist["result"] == g.get_result() and hist["player_color"] == is_white


# ---- 6 ---------------------------------------------------------------------------------------------------------
def test_match_tool_equals_the_cpu_loop():
    from chessrl_amd import gen_data as gd
    match = importlib.import_module("tools.opponent_match")
    pairs, opening, max_plies, seed = 2, 4, 40, 3
    common = dict(depth=2, node_budget=50, quiescence=0, ordering=True, repetition=True)
    a, b = dict(common, evaluation="positional"), dict(common, evaluation="material")
    a_white, moves, plies, results = match.play(pairs, a, b, opening, max_plies, seed)
    out, games = match.summary(a_white, moves, plies, results)
    assert list(a_white) == [True, False, True, False]
    words = gd.opening_words(random.Random(seed), pairs, opening)
    want, points = [], []
    for i in range(2 * pairs):
        g = OracleGame()
        w = iter(int(x) for x in words[i // 2])                     # games 2i and 2i + 1 share their opening
        ru.run_in_slot(g, lambda: next(w), max_moves=opening)
        assert len(g) == opening
        while g.get_result() is None and len(g) < max_plies:
            side = a if g.turn == bool(a_white[i]) else b
            ev.play_ply(g, 2, 50, 0, True, True, evaluation=side["evaluation"])
        want.append(g.get_history()["moves"])
        r = g.get_result()
        points.append(0.5 if r in (None, 0) else 1.0 if (r == 1) == bool(a_white[i]) else 0.0)
    assert games == want
    assert games[0][:opening] == games[1][:opening] and games[2][:opening] == games[3][:opening]
    assert games[0] != games[1]                                     # the colours are exchanged, the games differ
    assert (out["won"], out["drawn"], out["lost"]) == (points.count(1.0), points.count(0.5), points.count(0.0))
    assert out["score"] == sum(points) / 4 and sum(out["endings"].values()) == 4
    assert out["running_at_max_plies"] == out["endings"]["running"] == sum(1 for m in want if len(m) == max_plies)
