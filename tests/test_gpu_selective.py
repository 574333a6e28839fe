"""GPU: the built-in opponent's selective search (csrc/opponent.hpp SELECTIVE; the SEL shapes of the
``k_opponent_moves_id`` / ``k_reply_opponent_id`` kernel templates) against its CPU restatement (tests/selective_util.py; the restatement itself is held
to the ordered search and to its own branch counts without a GPU in tests/test_selective_cpu.py).

1. ``opponent_moves(selective=True)``: move, score, node count, flag and completed depth equal the restatement in every
   case of ``selective_util.CASES`` (depths 3 to 5, every kernel shape, budgets that cut inside a null child, a reduced
   search and a re-search); depth 0 and finished games; run to run; ``push``;
2. ``selective = 0`` through the new entry is the ``_ev`` entry, array for array, and so is ``selective = 1`` with
   maximum depths <= 2, nodes included; the refusals change nothing;
3. ``LockstepEngine(reply=MinimaxPlayer(False, 4, node_budget=400, ordering=True, selective=True))``: trees and the
   three accumulators against ``oracle.mcts_oracle.search`` on 16 roots, graph and eager;
4. ``MinimaxPlayer`` / ``GameOpponent``, ``benchmark`` (greedy and with ``sims``) and ``gen_data`` against CPU loops.
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
from tests import opponent_reply_util as u
from tests import opponent_util as ou
from tests import rollout_util as ru
from tests import selective_util as su
from tests import test_gpu_opponent as tg

pytestmark = pytest.mark.gpu

NO_MOVE, RESULT_NONE = 0xFFFF, 2
N_GAMES = len(su.games())                      # slots 0 .. N_GAMES - 1: the roots
TWIN = tg.TWIN                                 # slot 37 holds the root of slot 0 once more
MATED = (40, 41)                               # slots that hold roots 8 and 9: the back-rank mates are played there
MAX_PLIES = 320                                # the straddling games are 260 and 265 plies long


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def slot_games():
    """64 slots: slot s < N_GAMES holds game s, slot TWIN game 0, the slots of MATED games 8 and 9, every other slot
    game s % 16."""
    gs = [g for _, g in su.games()]
    assert 28 < N_GAMES <= TWIN and [n for n, _ in su.games()][8:10] == ["back_rank_white", "back_rank_black"]
    out = [gs[s] if s < N_GAMES else gs[s % 16] for s in range(64)]
    out[TWIN] = gs[0]
    for s, i in zip(MATED, (8, 9)):
        out[s] = gs[i]
    return out


def depth_row(depth, case=None):
    """``depth`` in the slots of the games (0 where ``case`` leaves the game out) and in the twin of slot 0."""
    row = np.zeros(64, np.int32)
    for i, (name, _) in enumerate(su.games()):
        row[i] = depth if case is None or su.in_case(name, case) else 0
    row[TWIN] = row[0]
    return row


def outputs():
    return (np.zeros(64, np.uint16), np.zeros(64, np.int32), np.zeros(64, np.int64), np.zeros(64, np.uint8),
            np.zeros(64, np.int32))


@pytest.fixture(scope="module")
def finished_ctx():
    """``slot_games`` with the mates of roots 8 and 9 played in MATED."""
    from chessrl_amd import _lib
    ctx = _lib.Context(64, 1, max_plies=MAX_PLIES)
    tg.load_games(ctx, slot_games())
    mate = np.full(64, NO_MOVE, np.uint16)
    for s, i in zip(MATED, (8, 9)):
        mate[s] = ou.alphabeta(su.games()[i][1], 1)[0]
    ctx.push_moves(mate)
    assert [int(r) for r in ctx.results()[list(MATED)]] == [1, -1]
    yield ctx
    ctx.close()


# ---- 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,quiescence,budget,repetition,evaluation", su.CASES)
def test_search_equals_the_restatement_and_repeats_itself(finished_ctx, depth, quiescence, budget, repetition,
                                                          evaluation):
    ctx = finished_ctx
    before = tg.state(ctx)
    case = (depth, quiescence, budget, repetition, evaluation)
    row = depth_row(depth, case)
    row[list(MATED)] = depth
    kw = dict(quiescence=quiescence, node_budget=budget, ordering=True, repetition=repetition, evaluation=evaluation)
    got = ctx.opponent_moves(row, selective=True, **kw)
    moves, scores, nodes, flags, done = got
    rows, _ = su.reference(*case)
    left_out = 0
    for i, ref in enumerate(rows):
        name = su.games()[i][0]
        one = (int(moves[i]), int(scores[i]), int(nodes[i]), int(flags[i]), int(done[i]))
        print(name, case, move_to_uci(one[0]) if one[0] != NO_MOVE else None, one[1:], "restated", ref)
        if ref is None:                                         # a depth-0 slot among the searched ones
            left_out += 1
            ref = (NO_MOVE, 0, 0, 0, 0)
        assert one == ref, (name, case)
    assert (left_out > 0) == (depth >= 4)
    if case == su.CAPPED_CASE:                                  # the search with the null-move cut capped to beta
        i = [n for n, _ in su.games()].index("capped_cut")
        assert int(flags[i]) == 0 and int(done[i]) == depth and su.reference(*case)[1]["null_cut_capped"] == 1
    assert all(a[TWIN] == a[0] for a in got)
    idle = row == 0
    assert (moves[idle] == NO_MOVE).all() and not any(a[idle].any() for a in (scores, nodes, flags, done))
    for s in MATED:                                             # a finished game: skipped, nothing searched
        assert (moves[s], scores[s], nodes[s], flags[s], done[s]) == (NO_MOVE, 0, 0, ou.SKIPPED, 0)
    assert nodes.max() <= budget
    full = ctx.opponent_moves(row, **kw)
    if budget >= 300:                                           # (a small budget ends before a node has r >= 3)
        assert not all(np.array_equal(a, b) for a, b in zip(got, full))    # the rules reach the searches of the case
    again = ctx.opponent_moves(row, selective=True, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))   # nothing of one search reaches the next
    assert tg.same_state(tg.state(ctx), before)                 # nothing was pushed, no slot was touched


def test_the_cases_are_the_cases_of_the_cpu_test():
    assert len(su.CASES) >= 8 and {c[0] for c in su.CASES} == {3, 4, 5}
    shapes = {(q > 0, rep, kind) for _, q, _, rep, kind in su.CASES}
    assert len(shapes) == 8                                     # every kernel shape
    total = su.new_counts()
    for case in su.CASES:
        for k, v in su.reference(*case)[1].items():
            total[k] += v
    for k in ("budget_cut_in_null_child", "budget_cut_in_reduced_search", "budget_cut_in_research", "null_cut_capped"):
        assert total[k] > 0, k
    assert sum(r[2] for case in su.CASES for r in su.reference(*case)[0] if r is not None) < 60000


def test_push_plays_the_move():
    from chessrl_amd import _lib
    games = slot_games()
    a, b = _lib.Context(64, 1, max_plies=MAX_PLIES), _lib.Context(64, 1, max_plies=MAX_PLIES)
    tg.load_games(a, games)
    tg.load_games(b, games)
    case = su.CASES[1]
    depth, quiescence, budget, repetition, evaluation = case
    row = depth_row(depth)
    row[N_GAMES:TWIN] = 2
    for ply in range(3):
        moves, _, nodes, flags, done = a.opponent_moves(row, push=True, quiescence=quiescence, node_budget=budget,
                                                        ordering=True, repetition=repetition, evaluation=evaluation,
                                                        selective=True)
        running = b.results() == RESULT_NONE
        want_skip = (row > 0) & ~running
        assert ((flags == ou.SKIPPED) == want_skip).all() and (moves[want_skip] == NO_MOVE).all()
        assert (moves[(row > 0) & running] != NO_MOVE).all() and (moves[row == 0] == NO_MOVE).all()
        assert nodes.max() <= budget and (done <= row).all()
        if ply == 0:
            for i in range(N_GAMES):
                assert (int(moves[i]), int(done[i])) == su.reference(*case)[0][i][::4]
        ok = b.push_moves(moves)
        assert (ok == (moves != NO_MOVE)).all()
        assert tg.same_state(tg.state(a), tg.state(b))
    a.close()
    b.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------
def test_selective_zero_and_shallow_depths_are_the_ev_entry(finished_ctx):
    ctx = finished_ctx
    L, h = ctx._L, ctx._h
    # selective = 0: whatever the other settings, ordering off included
    for depth, quiescence, budget, ordering, repetition, kind in ((3, 0, 300, 0, 0, 0), (3, 0, 300, 1, 1, 1),
                                                                 (2, 0, 63, 0, 1, 1), (3, 2, 200, 1, 0, 0),
                                                                 (4, 2, 300, 1, 1, 1)):
        row = depth_row(depth)
        row[list(MATED)] = depth
        old, new = outputs(), outputs()
        assert L.crl_opponent_moves_ev(h, ptr(row), quiescence, 0, budget, ordering, repetition, kind,
                                       *[ptr(a) for a in old]) == 0
        assert L.crl_opponent_moves_sel(h, ptr(row), quiescence, 0, budget, ordering, repetition, kind, 0,
                                        *[ptr(a) for a in new]) == 0
        assert all(np.array_equal(a, b) for a, b in zip(old, new))
        evaluation = "positional" if kind else "material"
        wrapped = ctx.opponent_moves(row, quiescence=quiescence, node_budget=budget, ordering=bool(ordering),
                                     repetition=bool(repetition), evaluation=evaluation, selective=False)
        assert all(np.array_equal(a, b) for a, b in zip(old, wrapped))
        if ordering:
            on = outputs()
            assert L.crl_opponent_moves_sel(h, ptr(row), quiescence, 0, budget, 1, repetition, kind, 1,
                                            *[ptr(a) for a in on]) == 0
            assert not all(np.array_equal(a, b) for a, b in zip(old, on))
    # selective = 1 with maximum depths <= 2: no node has r >= 3, none below the root r >= 2
    for quiescence, budget, repetition, kind in ((0, 63, 0, 0), (2, 200, 1, 1), (0, su.UNREACHED, 1, 0),
                                                 (2, su.UNREACHED, 0, 1)):
        row = depth_row(2)
        row[1::2] = np.minimum(row[1::2], 1)                    # depths 1 and 2 side by side
        row[list(MATED)] = 2
        old, new = outputs(), outputs()
        assert L.crl_opponent_moves_ev(h, ptr(row), quiescence, 0, budget, 1, repetition, kind,
                                       *[ptr(a) for a in old]) == 0
        assert L.crl_opponent_moves_sel(h, ptr(row), quiescence, 0, budget, 1, repetition, kind, 1,
                                        *[ptr(a) for a in new]) == 0
        assert all(np.array_equal(a, b) for a, b in zip(old, new)), (quiescence, budget, repetition, kind)
        assert old[2].max() > 20
    with pytest.raises(ValueError, match="selective needs ordering"):
        ctx.opponent_moves(depth_row(2), node_budget=100, selective=True)
    with pytest.raises(ValueError, match="ordering needs a node_budget"):
        ctx.opponent_moves(depth_row(2), ordering=True, selective=True)


def test_refusals_change_nothing():
    from chessrl_amd import _lib
    from chessrl_amd.opponent import GameOpponent, MinimaxPlayer
    ctx = _lib.Context(64, 1, max_plies=MAX_PLIES)
    tg.load_games(ctx, slot_games())
    before = tg.state(ctx)
    L, h = ctx._L, ctx._h
    moves, good = np.zeros(64, np.uint16), np.full(64, 1, np.int32)
    deep = good.copy()
    deep[63] = 6
    call = lambda depths, Q, budget, ordering, rep, kind, sel, out: L.crl_opponent_moves_sel(
        h, depths, Q, 1, budget, ordering, rep, kind, sel, out, None, None, None, None)
    for sel in (2, -1):
        assert call(ptr(good), 0, 100, 1, 0, 0, sel, ptr(moves)) == -1
    assert call(ptr(good), 0, 100, 0, 0, 0, 1, ptr(moves)) == -1            # selective without ordering
    assert call(ptr(good), 0, 100, 0, 1, 1, 1, ptr(moves)) == -1
    for kind in (2, -1):
        assert call(ptr(good), 0, 100, 1, 0, kind, 1, ptr(moves)) == -1
    for rep in (2, -1):
        assert call(ptr(good), 0, 100, 1, rep, 1, 1, ptr(moves)) == -1
    for ordering in (2, -1):
        assert call(ptr(good), 0, 100, ordering, 1, 1, 1, ptr(moves)) == -1
    for budget in (0, -1):
        assert call(ptr(good), 0, budget, 1, 1, 1, 1, ptr(moves)) == -1
    assert call(ptr(deep), 0, 100, 1, 0, 1, 1, ptr(moves)) == -1
    assert call(None, 0, 100, 1, 0, 1, 1, ptr(moves)) == -1 and call(ptr(good), 0, 100, 1, 0, 1, 1, None) == -1
    for bad in (-1, 7):
        assert call(ptr(good), bad, 100, 1, 0, 1, 1, ptr(moves)) == -1
    assert tg.same_state(tg.state(ctx), before)                 # push = 1 in every call: nothing was launched
    import torch
    dev = torch.zeros(64, dtype=torch.int64, device="cuda:0").data_ptr()
    reply = lambda Q, budget, ordering, rep, kind, sel, acc: L.crl_sim_reply_opponent_sel(
        h, dev, Q, budget, ordering, rep, kind, sel, dev, dev, dev, acc)
    assert reply(0, 100, 1, 0, 0, 2, dev) == -1 and reply(0, 100, 1, 0, 0, -1, dev) == -1
    assert reply(0, 100, 0, 0, 0, 1, dev) == -1                 # selective without ordering
    assert reply(0, 100, 1, 2, 1, 1, dev) == -1 and reply(0, 100, 1, 0, 2, 1, dev) == -1
    assert reply(0, 0, 1, 1, 1, 1, dev) == -1 and reply(7, 100, 1, 1, 1, 1, dev) == -1
    assert reply(0, 100, 1, 1, 1, 1, None) == -1                # refused before any launch: nothing is read or written
    with pytest.raises(ValueError, match="selective needs ordering"):
        ctx.sim_reply_opponent(dev, 1000, dev, dev, dev, node_budget=100, dev_depth_sum=dev, selective=True)
    with pytest.raises(ValueError, match="selective needs ordering"):
        MinimaxPlayer(True, 3, node_budget=100, selective=True)
    with pytest.raises(ValueError, match="selective needs ordering"):
        GameOpponent(opponent_budget=100, opponent_selective=True)
    with pytest.raises(ValueError, match="ordering needs a node_budget"):
        MinimaxPlayer(True, 3, ordering=True, selective=True)
    # scores, nodes, flags and depths_done may be NULL
    assert L.crl_opponent_moves_sel(h, ptr(good), 2, 0, 100, 1, 1, 1, 1, ptr(moves), None, None, None, None) == 0
    assert np.array_equal(moves, ctx.opponent_moves(good, quiescence=2, node_budget=100, ordering=True, repetition=True,
                                                    evaluation="positional", selective=True)[0])
    assert tg.same_state(tg.state(ctx), before)
    ctx.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------
SIMS, REPLY_DEPTH, BUDGET = 6, 4, 400


@functools.lru_cache(maxsize=None)
def tree(root, selective, mode="nep50"):
    """(SearchResult, log) of root ``root`` against the ordered opponent of maximum depth 4 under BUDGET: computed
    once."""
    agent = su.ReplyAgentSel(u.net(), REPLY_DEPTH, BUDGET, selective=selective)
    r = mcts_oracle.search(u.roots()[root], agent, SIMS, noise=False, mode=mode)
    return r, tuple(agent.log)


@pytest.mark.parametrize("graph", [True, False])
def test_reply_trees_equal_the_restatement(graph):
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.opponent import MinimaxPlayer
    from chessrl_amd.searchmode import SearchMode
    roots = u.roots()
    assert len(roots) == 16
    reply = MinimaxPlayer(False, REPLY_DEPTH, node_budget=BUDGET, ordering=True, selective=True)
    eng = LockstepEngine(u.net().to("cuda:0"), n_games=len(roots), max_sims=SIMS, reply=reply,
                         numpy_promotion="nep50", use_graph=graph, steps_per_graph=3)
    u.load_games(eng.ctx, list(roots))
    assert eng.reply.selective is True
    assert [p for _, p in eng._plan] == ["phase_select_expand", "phase_reply_opponent", "phase_tower_s2"]
    plain = MinimaxPlayer(False, REPLY_DEPTH, node_budget=BUDGET, ordering=True)
    assert SearchMode(reply=reply).key != SearchMode(reply=plain).key
    assert SearchMode(reply=plain).key[2][:7] == SearchMode(reply=reply).key[2][:7]    # appended to the tuple
    eng.search(SIMS)
    rc = eng.root_children()
    nodes, cuts, depth_sum = eng.reply_stats()
    for i in range(len(roots)):
        r, log = tree(i, True)
        u.assert_tree_equal(rc, i, r, ("graph", graph))
        want = (sum(n for _, _, n, _, _ in log), sum(1 for e in log if e[3] == ou.CUT), sum(e[4] for e in log))
        assert (int(nodes[i]), int(cuts[i]), int(depth_sum[i])) == want, (graph, i)
        assert all((e[3] == ou.CUT) == (e[4] < REPLY_DEPTH) and e[2] <= BUDGET for e in log)
    eng.close()
    changed = [i for i in (5, u.N_PREFIX, u.MIDDLEGAME) if tree(i, True)[1] != tree(i, False)[1]]
    print("roots whose reply logs differ from the full-width opponent's:", changed)
    assert changed                                              # the rules reach the trees


# ---- 4 ---------------------------------------------------------------------------------------------------------
PLIES = 12
MIDDLEGAME_FEN = "r2q1rk1/pp2bppp/2n1bn2/3p4/3P4/2NBPN2/PP3PPP/R1BQ1RK1 w - - 0 10"


def test_minimax_player_plays_the_selective_move():
    from chessrl_amd.game import Game
    from chessrl_amd.opponent import MinimaxPlayer
    from oracle.chess_oracle import board_from_fen
    g = Game(board=MIDDLEGAME_FEN)
    root = OracleGame(board=board_from_fen(MIDDLEGAME_FEN))
    for budget, limit, quiescence, repetition, evaluation in ((400, ou.NODE_LIMIT, 0, False, "material"),
                                                              (500, ou.NODE_LIMIT, 2, True, "positional"),
                                                              (500, 90, 0, True, "material")):
        p = MinimaxPlayer(True, search_depth=4, node_limit=limit, quiescence=quiescence, node_budget=budget,
                          ordering=True, repetition=repetition, evaluation=evaluation, selective=True)
        want = su.search(root, 4, min(budget, limit), quiescence, repetition, evaluation)
        assert p.best_move(g) == move_to_uci(want[0]) and p.last == want[1:4] and p.last_depth == want[4]
    g.free()


def test_game_opponent_one_move_at_a_time():
    from chessrl_amd.opponent import GameOpponent, MinimaxPlayer
    player = MinimaxPlayer(True, search_depth=1)
    g = GameOpponent(player_color=True, opponent_depth=3, opponent_budget=200, opponent_ordering=True,
                     opponent_selective=True)
    assert (g.opponent.search_depth, g.opponent.node_budget, g.opponent.selective, player.selective) == (
        3, 200, True, False)
    while g.get_result() is None and len(g) < PLIES:
        g.move(player.best_move(g))
    hist = g.get_history()
    g.free()
    c = OracleGame()
    while c.get_result() is None and len(c) < PLIES:
        ou.play_ply(c, 1)
        if c.get_result() is None:
            su.play_ply(c, 3, 200)
    assert (hist["moves"], hist["result"]) == (c.get_history()["moves"], c.get_result())
    assert len(hist["moves"]) >= PLIES


def test_benchmark_equals_the_cpu_loop(capsys):
    from chessrl_amd import benchmark as bm
    net = FakeNet(seed=5, prior_shift=29)
    out = bm.benchmark(None, games=4, opponent_depth=3, opponent_quiescence=2, opponent_budget=150, seed=7,
                       max_plies=PLIES, model=net.to("cuda:0"), log=True, opponent_ordering=True,
                       opponent_repetition=True, opponent_evaluation="positional", opponent_selective=True)
    said = capsys.readouterr().out.lower()
    assert ("against the built-in opponent, depth <= 3 within 150 nodes per move, ordered, repetition-aware, "
            "quiescence 2, positional evaluation, selective (not stockfish, no elo)" in said)
    colors = bm.game_colors(4, seed=7)
    agent = mcts_oracle.OracleAgent(net)
    want, results = [], []
    for c in colors:
        g = OracleGame()
        while g.get_result() is None and len(g) < PLIES:
            if g.turn == c:
                assert g.move(agent.best_move(g, real_game=True))
            else:
                su.play_ply(g, 3, 150, 2, True, "positional")
        want.append(g.get_history()["moves"])
        results.append(g.get_result())
    assert out["games"] == want
    assert {k: out[k] for k in ("played", "won", "drawn")} == bm.tally(colors, results)
    assert True in colors and False in colors                   # both colours were played
    with pytest.raises(ValueError, match="selective needs ordering"):
        bm.benchmark(None, games=2, opponent_budget=20, model=net.to("cuda:0"), opponent_selective=True)
    # the line of a run without the option is what it was
    bm.benchmark(None, games=2, opponent_depth=2, opponent_budget=20, seed=7, max_plies=2, model=net.to("cuda:0"),
                 log=True, opponent_ordering=True)
    assert "within 20 nodes per move, ordered (not stockfish, no elo)" in capsys.readouterr().out.lower()


def test_benchmark_with_sims_equals_the_cpu_loop():
    from chessrl_amd import benchmark as bm
    from chessrl_amd.engine import resolve_numpy_promotion
    from oracle.chess_oracle import NULL_MOVE
    games, sims, max_plies, depth, budget = 4, 8, 6, 3, 150
    mode = resolve_numpy_promotion("auto")
    out = bm.benchmark(None, games=games, opponent_depth=depth, opponent_budget=budget, seed=7, max_plies=max_plies,
                       model=u.net().to("cuda:0"), sims=sims, opponent_ordering=True, opponent_selective=True)
    colors = bm.game_colors(games, seed=7)
    want, results = [], []
    for white in colors:                                        # opponent_reply_util.cpu_games with this opponent
        g = OracleGame()
        agent = su.ReplyAgentSel(u.net(), depth, budget)
        if not white:                                           # the opponent opens as white
            su.play_ply(g, depth, budget)
        while g.get_result() is None and len(g) < max_plies:
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
    n, opening, seed, max_plies, budget = 4, 4, 0, 16, 150
    d = gd.gen_data(path, num_games=n, depth=3, node_budget=budget, ordering=True, selective=True,
                    opening_plies=opening, seed=seed, max_plies=max_plies)
    draws = gd.draw_games(n, depth=3, random_dep=False, seed=seed)
    words = gd.opening_words(random.Random(seed), n, opening)
    saved = {rec.game_id: rec for rec in d.games}
    for i in range(n):
        is_white, game_depth, player_depth = draws[i]
        g = OracleGame()
        w = iter(int(x) for x in words[i])
        ru.run_in_slot(g, lambda: next(w), max_moves=opening)
        assert len(g) == opening
        while g.get_result() is None and len(g) < max_plies:
            su.play_ply(g, player_depth if g.turn == is_white else game_depth, budget)
        if g.get_result() is None:                                  # still running after max_plies: dropped
            assert i not in saved
            continue
        hist = saved[i].get_history()
        assert hist["moves"] == g.get_history()["moves"]
        assert hist["result"] == g.get_result() and hist["player_color"] == is_white
    with pytest.raises(ValueError, match="selective needs ordering"):
        gd.gen_data(path, num_games=1, node_budget=50, selective=True)
