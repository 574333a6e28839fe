"""GPU: the built-in opponent's repetition rule under a node budget (csrc/opponent.hpp REPETITION;
the REP shapes of the ``k_opponent_moves_id`` / ``k_reply_opponent_id`` kernel templates) against its CPU
restatement (tests/repetition_util.py; its preconditions and the case list are asserted without a GPU in
tests/test_repetition_cpu.py).

1. move, score, node count, flag and completed depth of the 19 set-up roots and nine roots with a history equal
   ``repeated`` in every case of ``repetition_util.CASES``, ordering off and on; depth 0 and finished games; run to run;
2. ``repetition = 0`` through the new entry is ``crl_opponent_moves_ord``, array for array; ``repetition = 1`` differs
   on the history roots and, D + Q <= 3, not on the roots with clock 0, nodes included;
3. ``push`` plays the move: history and result as by ``crl_push_moves``, the forced fifth occurrence and two games
   whose history ring has wrapped included;
4. the refusals;
5. ``MinimaxPlayer`` / ``GameOpponent``, ``benchmark`` (greedy and searching) and ``gen_data`` against CPU loops;
6. ``LockstepEngine(reply=MinimaxPlayer(node_budget=B, repetition=True))``: trees and reply statistics, graph and
   eager, on roots with a shuffle behind S1; ``repetition=False`` gives today's trees.
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
from tests import repetition_util as rp
from tests import rollout_util as ru
from tests import test_gpu_opponent as tg

pytestmark = pytest.mark.gpu

NO_MOVE, RESULT_NONE = 0xFFFF, 2
N_GAMES = len(rp.games())                      # slots 0 .. 18 the set-up roots, 19 .. 27 the roots with a history
TWIN, FIFTH_SLOT = tg.TWIN, tg.FIFTH_SLOT      # slot 37 holds the root of slot 0 once more
MATED = (40, 41)                               # slots that hold roots 8 and 9: the back-rank mates are played there
MAX_PLIES = 320                                # the straddling games are 260 and 265 plies long


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def slot_games():
    """64 slots: slot s < 28 holds game s, slot TWIN game 0, the slots of MATED games 8 and 9, every other slot game
    s % 16."""
    gs = [g for _, g in rp.games()]
    assert N_GAMES == 28 and [n for n, _ in rp.games()][8:10] == ["back_rank_white", "back_rank_black"]
    out = [gs[s] if s < N_GAMES else gs[s % 16] for s in range(64)]
    out[TWIN] = gs[0]
    for s, i in zip(MATED, (8, 9)):
        out[s] = gs[i]
    return out


def context64():
    from chessrl_amd import _lib
    ctx = _lib.Context(64, 1, max_plies=MAX_PLIES)
    tg.load_games(ctx, slot_games())
    return ctx


def depth_row(depth, case=None):
    """``depth`` in the 28 slots of the games (0 where ``case`` leaves the game out) and in the twin of slot 0."""
    row = np.zeros(64, np.int32)
    for i, (name, _) in enumerate(rp.games()):
        row[i] = depth if case is None or rp.in_case(name, case) else 0
    row[TWIN] = row[0]
    return row


# ---- 1 ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def finished_ctx():
    """The one context of sections 1 and 2: ``slot_games`` with the mates of roots 8 and 9 played in MATED."""
    ctx = context64()
    mate = np.full(64, NO_MOVE, np.uint16)
    for s, i in zip(MATED, (8, 9)):
        mate[s] = ou.alphabeta(rp.games()[i][1], 1)[0]
    ctx.push_moves(mate)
    assert [int(r) for r in ctx.results()[list(MATED)]] == [1, -1]
    yield ctx
    ctx.close()


@pytest.mark.parametrize("ordering", [False, True])
@pytest.mark.parametrize("depth,quiescence,budget", rp.CASES)
def test_search_equals_the_restatement_and_repeats_itself(finished_ctx, depth, quiescence, budget, ordering):
    ctx = finished_ctx
    before = tg.state(ctx)
    case = (depth, quiescence, budget)
    row = depth_row(depth, case)
    row[list(MATED)] = depth
    got = ctx.opponent_moves(row, quiescence=quiescence, node_budget=budget, ordering=ordering, repetition=True)
    moves, scores, nodes, flags, done = got
    left_out = 0
    for i, ref in enumerate(rp.reference(depth, quiescence, budget, ordering)[0]):
        name = rp.games()[i][0]
        one = (int(moves[i]), int(scores[i]), int(nodes[i]), int(flags[i]), int(done[i]))
        print(name, case, ordering, move_to_uci(one[0]) if one[0] != NO_MOVE else None, one[1:], "restated", ref)
        if ref is None:                                         # a depth-0 slot among the searched ones
            left_out += 1
            ref = (NO_MOVE, 0, 0, 0, 0)
        assert one == ref, (name, case, ordering)
    assert left_out == (N_GAMES - len(rp.SMALL) if depth == 4 else 0)
    assert all(a[TWIN] == a[0] for a in got)
    idle = row == 0
    assert (moves[idle] == NO_MOVE).all() and not any(a[idle].any() for a in (scores, nodes, flags, done))
    for s in MATED:                                             # a finished game: skipped, nothing searched
        assert (moves[s], scores[s], nodes[s], flags[s], done[s]) == (NO_MOVE, 0, 0, ou.SKIPPED, 0)
    assert nodes.max() <= budget
    again = ctx.opponent_moves(row, quiescence=quiescence, node_budget=budget, ordering=ordering, repetition=True)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))   # nothing of one search reaches the next
    assert tg.same_state(tg.state(ctx), before)    # nothing was pushed, no slot was touched


# ---- 2 ---------------------------------------------------------------------------------------------------------
def outputs():
    return (np.zeros(64, np.uint16), np.zeros(64, np.int32), np.zeros(64, np.int64), np.zeros(64, np.uint8),
            np.zeros(64, np.int32))


def test_repetition_zero_is_the_ord_entry_and_clock_zero_roots_do_not_change(finished_ctx):
    ctx = finished_ctx
    L, h = ctx._L, ctx._h
    names = [n for n, _ in rp.games()]
    clock0 = [i for i, (_, g) in enumerate(rp.games()) if rp.clock(g) == 0]
    hist = [names.index(n) for n in ("kqk_black", "ep_none", "forced_fifth_cut", "king_shuffle")]
    assert len(clock0) >= 12 and not set(clock0) & set(hist)
    for depth, quiescence, budget, ordering in ((3, 0, 600, 0), (3, 0, 600, 1), (2, 0, 63, 0), (3, 2, 300, 1)):
        row = depth_row(depth)
        row[list(MATED)] = depth
        old, new, on = outputs(), outputs(), outputs()
        assert L.crl_opponent_moves_ord(h, ptr(row), quiescence, 0, budget, ordering, *[ptr(a) for a in old]) == 0
        assert L.crl_opponent_moves_rep(h, ptr(row), quiescence, 0, budget, ordering, 0, *[ptr(a) for a in new]) == 0
        assert L.crl_opponent_moves_rep(h, ptr(row), quiescence, 0, budget, ordering, 1, *[ptr(a) for a in on]) == 0
        assert all(np.array_equal(a, b) for a, b in zip(old, new))
        ref = (od.reference if ordering else it.reference)(depth, quiescence, budget)[0]
        for i in range(19):
            if ref[i] is not None:
                assert tuple(int(a[i]) for a in new) == ref[i]
        for i in hist:                                              # repetition = 1 is another search there
            assert tuple(int(a[i]) for a in on) != tuple(int(a[i]) for a in new), names[i]
        if depth + quiescence <= 3:                                 # consequence (b), nodes included
            for i in clock0:
                assert tuple(int(a[i]) for a in on) == tuple(int(a[i]) for a in new), names[i]
        wrapped = ctx.opponent_moves(row, quiescence=quiescence, node_budget=budget, ordering=bool(ordering),
                                     repetition=False)
        assert all(np.array_equal(a, b) for a, b in zip(old, wrapped))
    with pytest.raises(ValueError, match="repetition needs a node_budget"):
        ctx.opponent_moves(depth_row(2), repetition=True)


# ---- 3 ---------------------------------------------------------------------------------------------------------
def test_push_plays_the_move():
    from chessrl_amd import _lib
    games = slot_games()
    games[FIFTH_SLOT] = tg.forced_fifth_game()
    a, b = _lib.Context(64, 1, max_plies=MAX_PLIES), _lib.Context(64, 1, max_plies=MAX_PLIES)
    tg.load_games(a, games)
    tg.load_games(b, games)
    names = [n for n, _ in rp.games()]
    straddlers = [names.index("straddle_%d" % L) for L in rp.STRADDLE_L]
    assert all(len(games[s]) > 256 for s in straddlers)         # their history ring has wrapped
    row = depth_row(3)
    row[28:37] = 2                                              # roots 12 .. 15, 0 .. 4 once more, one ply shallower
    row[FIFTH_SLOT] = 2
    for ply in range(3):
        moves, _, nodes, flags, done = a.opponent_moves(row, push=True, quiescence=2, node_budget=300, repetition=True)
        running = b.results() == RESULT_NONE
        want_skip = (row > 0) & ~running
        assert ((flags == ou.SKIPPED) == want_skip).all() and (moves[want_skip] == NO_MOVE).all()
        assert (moves[(row > 0) & running] != NO_MOVE).all() and (moves[row == 0] == NO_MOVE).all()
        assert nodes.max() <= 300 and (done <= row).all()
        if ply == 0:
            for i in range(N_GAMES):
                assert (int(moves[i]), int(done[i])) == rp.reference(3, 2, 300)[0][i][::4]
        ok = b.push_moves(moves)
        assert (ok == (moves != NO_MOVE)).all()
        assert tg.same_state(tg.state(a), tg.state(b))
        # the forced line: running after one ply, drawn by the REAL fifth occurrence after two, skipped in the third
        assert (int(a.results()[FIFTH_SLOT]), int(flags[FIFTH_SLOT])) == ((RESULT_NONE, 0), (0, 0), (0, ou.SKIPPED))[ply]
    res = a.results()
    assert res[8] == 1 and res[9] == -1                         # the back-rank mates were delivered
    assert a.records()[1][FIFTH_SLOT] == len(tg.FORCED_FIFTH) + 2
    for s, L in zip(straddlers, rp.STRADDLE_L):                 # three plies past ply L + 10, in the wrapped ring
        assert a.records()[1][s] == L + 13
    a.close()
    b.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from chessrl_amd import _lib
    ctx = context64()
    before = tg.state(ctx)
    L, h = ctx._L, ctx._h
    moves, good = np.zeros(64, np.uint16), np.full(64, 1, np.int32)
    deep, negative = good.copy(), good.copy()
    deep[63], negative[5] = 6, -1
    call = lambda depths, Q, budget, ordering, rep, out: L.crl_opponent_moves_rep(h, depths, Q, 1, budget, ordering, rep,
                                                                                  out, None, None, None, None)
    for rep in (2, -1):
        assert call(ptr(good), 0, 100, 0, rep, ptr(moves)) == -1
    for ordering in (2, -1):
        assert call(ptr(good), 0, 100, ordering, 1, ptr(moves)) == -1
    for budget in (0, -1):
        assert call(ptr(good), 0, budget, 1, 1, ptr(moves)) == -1
    assert call(ptr(deep), 0, 100, 0, 1, ptr(moves)) == -1 and call(ptr(negative), 0, 100, 0, 1, ptr(moves)) == -1
    assert call(None, 0, 100, 0, 1, ptr(moves)) == -1 and call(ptr(good), 0, 100, 0, 1, None) == -1
    for bad in (-1, 7):
        assert call(ptr(good), bad, 100, 0, 1, ptr(moves)) == -1
    assert tg.same_state(tg.state(ctx), before)                 # push = 1 in every call: nothing was launched
    with pytest.raises(_lib.HipLibraryError):
        ctx.opponent_moves(good, node_budget=0, repetition=True)
    import torch
    dev = torch.zeros(64, dtype=torch.int64, device="cuda:0").data_ptr()
    reply = lambda Q, budget, ordering, rep, acc: L.crl_sim_reply_opponent_rep(h, dev, Q, budget, ordering, rep, dev, dev,
                                                                               dev, acc)
    assert reply(0, 100, 0, 2, dev) == -1 and reply(0, 100, 2, 1, dev) == -1 and reply(0, 0, 0, 1, dev) == -1
    assert reply(7, 100, 0, 1, dev) == -1
    assert reply(0, 100, 0, 1, None) == -1                      # refused before any launch: nothing is read or written
    with pytest.raises(ValueError, match="repetition needs a node_budget"):
        ctx.sim_reply_opponent(dev, 1000, dev, dev, dev, repetition=True)
    # scores, nodes, flags and depths_done may be NULL
    assert L.crl_opponent_moves_rep(h, ptr(good), 2, 0, 100, 1, 1, ptr(moves), None, None, None, None) == 0
    assert np.array_equal(moves, ctx.opponent_moves(good, quiescence=2, node_budget=100, ordering=True, repetition=True)[0])
    assert tg.same_state(tg.state(ctx), before)
    ctx.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------
PLIES = 24


def test_minimax_player_plays_the_move_of_the_rule():
    from chessrl_amd.game import Game
    from chessrl_amd.opponent import MinimaxPlayer
    g = Game(board=rp.KQK)
    for uci in dict((n, m) for n, _, m in rp.TABLE)["kqk_black"]:
        assert g.move(uci)
    root = rp.table_game("kqk_black")
    for budget, limit, ordering in ((80, ou.NODE_LIMIT, False), (600, ou.NODE_LIMIT, True), (600, 30, False)):
        p = MinimaxPlayer(False, search_depth=3, node_limit=limit, quiescence=2, node_budget=budget, ordering=ordering,
                          repetition=True)
        want = rp.repeated(root, 3, min(budget, limit), 2, ordering)
        assert p.best_move(g) == move_to_uci(want[0]) and p.last == want[1:4] and p.last_depth == want[4]
    p = MinimaxPlayer(False, search_depth=3, node_budget=600, repetition=True)
    assert (p.best_move(g), p.last[0]) == ("g8h8", 0)           # the issue's table: a draw, not -906
    g.free()


def test_game_opponent_one_move_at_a_time():
    from chessrl_amd.opponent import GameOpponent, MinimaxPlayer
    player = MinimaxPlayer(True, search_depth=1)
    g = GameOpponent(player_color=True, opponent_depth=3, opponent_budget=100, opponent_repetition=True)
    assert (g.opponent.search_depth, g.opponent.node_budget, g.opponent.repetition, g.opponent.ordering,
            player.repetition) == (3, 100, True, False, False)
    while g.get_result() is None and len(g) < PLIES:
        g.move(player.best_move(g))
    hist = g.get_history()
    g.free()
    c = OracleGame()
    while c.get_result() is None and len(c) < PLIES:
        ou.play_ply(c, 1)
        if c.get_result() is None:
            rp.play_ply(c, 3, 100)
    assert (hist["moves"], hist["result"]) == (c.get_history()["moves"], c.get_result())
    assert len(hist["moves"]) >= PLIES


def test_benchmark_equals_the_cpu_loop(capsys):
    from chessrl_amd import benchmark as bm
    net = FakeNet(seed=5, prior_shift=29)
    out = bm.benchmark(None, games=4, opponent_depth=3, opponent_quiescence=2, opponent_budget=80, seed=7,
                       max_plies=PLIES, model=net.to("cuda:0"), log=True, opponent_ordering=True,
                       opponent_repetition=True)
    said = capsys.readouterr().out.lower()
    assert ("against the built-in opponent, depth <= 3 within 80 nodes per move, ordered, repetition-aware" in said
            and "(not stockfish, no elo)" in said)
    colors = bm.game_colors(4, seed=7)
    agent = mcts_oracle.OracleAgent(net)
    want, results = [], []
    for c in colors:
        g = OracleGame()
        while g.get_result() is None and len(g) < PLIES:
            if g.turn == c:
                assert g.move(agent.best_move(g, real_game=True))
            else:
                rp.play_ply(g, 3, 80, 2, ordering=True)
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
                       model=u.net().to("cuda:0"), opponent_repetition=True)
    want, results = [], []
    for white in colors:                                        # opponent_reply_util.cpu_games with this opponent
        g = OracleGame()
        agent = rp.ReplyAgentRep(u.net(), depth, budget)
        if not white:
            rp.play_ply(g, depth, budget)
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
    n, opening, seed, max_plies, budget = 4, 4, 0, 120, 200
    d = gd.gen_data(path, num_games=n, depth=2, node_budget=budget, repetition=True, opening_plies=opening, seed=seed,
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
            rp.play_ply(g, player_depth if g.turn == is_white else game_depth, budget)
        if g.get_result() is None:                                  # still running after max_plies: dropped
            assert i not in saved
            continue
        hist = saved[i].get_history()
        assert hist["moves"] == g.get_history()["moves"]          # every move replayed legally in the oracle
        assert hist["result"] == g.get_result() and hist["player_color"] == is_white
    print("finished games:", sorted(saved))
    assert len(saved) >= 1


# ---- 6 ---------------------------------------------------------------------------------------------------------
SIMS, REPLY_DEPTH, BUDGET = 24, 3, 120
SHUFFLED = ("start_knights", "kqk_white")      # the two roots with a shuffle in their history: S1 has history behind it


@functools.lru_cache(maxsize=None)
def reply_roots():
    assert len(u.roots()) == 16
    return tuple(u.roots()) + tuple(rp.table_game(n) for n in SHUFFLED)


@functools.lru_cache(maxsize=None)
def tree(root, repetition, mode="nep50"):
    """(SearchResult, log) of root ``root`` against the opponent of maximum depth 3 under BUDGET: computed once, never
    changed."""
    agent = (rp.ReplyAgentRep if repetition else it.ReplyAgentID)(u.net(), REPLY_DEPTH, BUDGET, 0)
    r = mcts_oracle.search(reply_roots()[root], agent, SIMS, noise=False, mode=mode)
    return r, tuple(agent.log)


def engine(repetition, **kw):
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.opponent import MinimaxPlayer
    reply = MinimaxPlayer(False, REPLY_DEPTH, node_budget=BUDGET, repetition=repetition)
    eng = LockstepEngine(u.net().to("cuda:0"), n_games=len(reply_roots()), max_sims=SIMS, reply=reply,
                         numpy_promotion="nep50", **kw)
    u.load_games(eng.ctx, list(reply_roots()))
    return eng


def check_trees(eng, repetition, what):
    """The trees and the three per-game accumulators against the restatement; -> the logs of all replies."""
    eng.search(SIMS)
    rc = eng.root_children()
    nodes, cuts, depth_sum = eng.reply_stats()
    seen = []
    for i in range(len(reply_roots())):
        r, log = tree(i, repetition)
        u.assert_tree_equal(rc, i, r, what)
        want = (sum(n for _, _, n, _, _ in log), sum(1 for e in log if e[3] == ou.CUT), sum(e[4] for e in log))
        assert (int(nodes[i]), int(cuts[i]), int(depth_sum[i])) == want, (what, i)
        assert all((e[3] == ou.CUT) == (e[4] < REPLY_DEPTH) and e[2] <= BUDGET for e in log)
        seen += list(log)
    return seen


@pytest.mark.parametrize("graph", [True, False])
def test_reply_trees_equal_the_restatement(graph):
    eng = engine(True, use_graph=graph, steps_per_graph=8)
    assert eng.reply.repetition is True
    assert [p for _, p in eng._plan] == ["phase_select_expand", "phase_reply_opponent", "phase_tower_s2"]
    check_trees(eng, True, ("graph", graph))
    eng.close()
    # the rule matters in these trees: root 5, a random prefix with reversible plies behind it, gets another reply in
    # one of its nodes; on the two shuffled roots the replies stay and their node counts change
    differ = [i for i in range(len(reply_roots()))
              if [e[0] for e in tree(i, True)[1]] != [e[0] for e in tree(i, False)[1]]]
    print("roots whose replies differ from the rule-off tree:", differ)
    assert 5 in differ
    changed = [i for i in range(len(reply_roots())) if tree(i, True)[1] != tree(i, False)[1]]
    assert {16, 17} <= set(changed)


def test_repetition_off_gives_todays_trees():
    eng = engine(False)
    assert eng.reply.repetition is False
    check_trees(eng, False, ("rule off", BUDGET))
    eng.close()
