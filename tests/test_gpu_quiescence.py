"""GPU: the built-in opponent's quiescence search (csrc/opponent.hpp QUIESCENCE; ``k_opponent_moves_q``,
``k_reply_opponent_q``) against its CPU restatement (tests/quiescence_util.py; its preconditions are asserted without
a GPU in tests/test_quiescence_cpu.py).

1. move, score, node count and flag of 16 roots and three set-up positions equal ``alphabeta_q``; run to run;
2. ``quiescence=0`` equals the entry point without the argument;
3. the cut through the C-ABI;
4. ``push`` equals ``crl_push_moves`` of the returned move;
5. the refusals;
6. ``MinimaxPlayer`` / ``GameOpponent``, ``benchmark`` and ``gen_data`` against CPU loops;
7. ``LockstepEngine(reply=MinimaxPlayer(quiescence=Q))``: trees and reply statistics, graph and eager, and under a
   node limit that cuts.
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
from tests import quiescence_util as q
from tests import rollout_util as ru
from tests import test_gpu_opponent as tg

pytestmark = pytest.mark.gpu

NO_MOVE, RESULT_NONE = 0xFFFF, 2
N_GAMES = 19                                   # slots 0 .. 15 the private roots, 16 .. 18 the set-up positions
TWIN, FIFTH_SLOT = tg.TWIN, tg.FIFTH_SLOT      # slot 37 holds the root of slot 0 once more


def slot_games():
    """64 slots: slot s < 19 holds game s of ``quiescence_util.games()``, slot TWIN game 0, the others root s % 16."""
    gs = [g for _, g in q.games()]
    return [gs[0] if s == TWIN else gs[s] if s < N_GAMES else gs[s % 16] for s in range(64)]


def context64():
    from chessrl_amd import _lib
    ctx = _lib.Context(64, 1, max_plies=256)
    tg.load_games(ctx, slot_games())
    return ctx


def depth_row(depth, quiescence):
    row = np.zeros(64, np.int32)
    for i, ref in enumerate(q.reference(depth, quiescence)[0]):
        if ref is not None:
            row[i] = depth
    row[TWIN] = row[0]
    return row


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---- 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,quiescence", q.CASES)
def test_search_equals_the_restatement_and_repeats_itself(depth, quiescence):
    ctx = context64()
    before = tg.state(ctx)
    row = depth_row(depth, quiescence)
    assert row[16:19].all() and (row[19:TWIN] == 0).all()
    moves, scores, nodes, flags = ctx.opponent_moves(row, quiescence=quiescence)
    for i, ref in enumerate(q.reference(depth, quiescence)[0]):
        name = q.games()[i][0]
        if ref is None:
            assert row[i] == 0
            continue
        got = (int(moves[i]), int(scores[i]), int(nodes[i]), int(flags[i]))
        print(name, depth, quiescence, move_to_uci(got[0]), got[1:], "restated", ref)
        assert got == ref, (name, depth, quiescence)
    assert (moves[TWIN], scores[TWIN], nodes[TWIN], flags[TWIN]) == (moves[0], scores[0], nodes[0], flags[0])
    idle = row == 0
    assert (moves[idle] == NO_MOVE).all() and not scores[idle].any() and not nodes[idle].any() and not flags[idle].any()
    again = ctx.opponent_moves(row, quiescence=quiescence)
    assert all(np.array_equal(a, b) for a, b in zip((moves, scores, nodes, flags), again))
    assert tg.same_state(tg.state(ctx), before)    # nothing was pushed, no slot was touched
    ctx.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------
def test_quiescence_zero_equals_the_old_entry_point():
    ctx = context64()
    L, h = ctx._L, ctx._h
    for depth in (1, 2):
        row = np.full(64, depth, np.int32)
        moves, scores = np.zeros(64, np.uint16), np.zeros(64, np.int32)
        nodes, flags = np.zeros(64, np.int64), np.zeros(64, np.uint8)
        assert L.crl_opponent_moves(h, ptr(row), 0, ou.NODE_LIMIT, ptr(moves), ptr(scores), ptr(nodes), ptr(flags)) == 0
        new = ctx.opponent_moves(row, quiescence=0)
        assert all(np.array_equal(a, b) for a, b in zip((moves, scores, nodes, flags), new))
        for i in range(16):
            assert (int(moves[i]), int(scores[i]), int(nodes[i]), int(flags[i])) == ou.alphabeta(q.games()[i][1], depth)
        # and quiescence is not ignored: some row differs in its node count
        assert not np.array_equal(ctx.opponent_moves(row, quiescence=1)[2], nodes)
    ctx.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------
def test_the_cut_through_the_c_abi():
    ctx = context64()
    L, h = ctx._L, ctx._h
    slot = [n for n, _ in q.games()].index("midgame_40")
    game = q.games()[slot][1]
    legal = game.legal_move_ids()
    only = np.zeros(64, np.int32)
    only[slot] = 2
    full = q.reference(2, 6)[0][slot][2]
    for limit in (full + 1, full, full - 1, full // 2, 1):
        moves, scores = np.zeros(64, np.uint16), np.zeros(64, np.int32)
        nodes, flags = np.zeros(64, np.int64), np.zeros(64, np.uint8)
        assert L.crl_opponent_moves_q(h, ptr(only), 6, 0, limit, ptr(moves), ptr(scores), ptr(nodes), ptr(flags)) == 0
        got = (int(moves[slot]), int(scores[slot]), int(nodes[slot]), int(flags[slot]))
        want = q.alphabeta_q(game, 2, 6, node_limit=limit)
        print("limit", limit, got, "restated", want)
        assert got == want
        assert (got[3] == ou.CUT) == (limit < full) and got[0] in legal
    ctx.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------
def test_push_equals_push_moves_of_the_returned_move():
    from chessrl_amd import _lib
    games = slot_games()
    games[FIFTH_SLOT] = tg.forced_fifth_game()
    a, b = _lib.Context(64, 1, max_plies=256), _lib.Context(64, 1, max_plies=256)
    tg.load_games(a, games)
    tg.load_games(b, games)
    row = depth_row(1, 2)
    row[19:35] = 2                                              # roots 3 .. 15, 0 .. 2 once more, one ply deeper
    row[FIFTH_SLOT] = 1
    for ply in range(3):
        moves, _, _, flags = a.opponent_moves(row, push=True, quiescence=2)
        running = b.results() == RESULT_NONE
        want_skip = (row > 0) & ~running
        assert ((flags == ou.SKIPPED) == want_skip).all() and (moves[want_skip] == NO_MOVE).all()
        assert (moves[(row > 0) & running] != NO_MOVE).all() and (moves[row == 0] == NO_MOVE).all()
        if ply == 0:
            for i in range(N_GAMES):
                assert int(moves[i]) == q.reference(1, 2)[0][i][0]
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


# ---- 5 ---------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from chessrl_amd import _lib
    from chessrl_amd.opponent import MinimaxPlayer
    ctx = context64()
    before = tg.state(ctx)
    L, h = ctx._L, ctx._h
    moves, good = np.zeros(64, np.uint16), np.full(64, 1, np.int32)
    for bad in (-1, 7):
        assert L.crl_opponent_moves_q(h, ptr(good), bad, 1, 1000, ptr(moves), None, None, None) == -1
    assert tg.same_state(tg.state(ctx), before)
    with pytest.raises(_lib.HipLibraryError):
        ctx.opponent_moves(good, quiescence=7)
    import torch
    dev = torch.zeros(64, dtype=torch.int64, device="cuda:0").data_ptr()
    for bad in (-1, 7):                                         # refused before any launch: nothing is read or written
        with pytest.raises(_lib.HipLibraryError):
            ctx.sim_reply_opponent(dev, 1000, dev, dev, dev, quiescence=bad)
    with pytest.raises(ValueError):
        MinimaxPlayer(True, quiescence=7)
    # scores, nodes and flags may be NULL
    assert L.crl_opponent_moves_q(h, ptr(good), 6, 0, 1000, ptr(moves), None, None, None) == 0
    assert np.array_equal(moves, ctx.opponent_moves(good, node_limit=1000, quiescence=6)[0])
    assert tg.same_state(tg.state(ctx), before)
    ctx.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------
PLIES = 24


def test_minimax_player_on_the_known_answer():
    from chessrl_amd.game import Game
    from chessrl_amd.opponent import MinimaxPlayer
    g = Game(board=q.KNOWN_ANSWER)
    assert MinimaxPlayer(True, search_depth=1).best_move(g) == "e2e5"
    p = MinimaxPlayer(True, search_depth=1, quiescence=4)
    want = q.alphabeta_q(q.games()[16][1], 1, 4)
    assert p.best_move(g) == move_to_uci(want[0]) != "e2e5" and p.last == want[1:]
    g.free()


def test_game_opponent_one_move_at_a_time():
    from chessrl_amd.opponent import GameOpponent, MinimaxPlayer
    player = MinimaxPlayer(True, search_depth=1)
    g = GameOpponent(player_color=True, opponent_depth=2, opponent_quiescence=2)
    assert (g.opponent.search_depth, g.opponent.quiescence, player.quiescence) == (2, 2, 0)
    while g.get_result() is None and len(g) < PLIES:
        g.move(player.best_move(g))
    hist = g.get_history()
    g.free()
    c = OracleGame()
    while c.get_result() is None and len(c) < PLIES:
        ou.play_ply(c, 1)
        if c.get_result() is None:
            q.play_ply_q(c, 2, 2)
    assert (hist["moves"], hist["result"]) == (c.get_history()["moves"], c.get_result())
    assert len(hist["moves"]) >= PLIES


def test_benchmark_equals_the_cpu_loop(capsys):
    from chessrl_amd import benchmark as bm
    net = FakeNet(seed=5, prior_shift=29)
    out = bm.benchmark(None, games=4, opponent_depth=1, opponent_quiescence=2, seed=7, max_plies=PLIES,
                       model=net.to("cuda:0"), log=True)
    assert "built-in depth-1 opponent, quiescence 2" in capsys.readouterr().out
    colors = bm.game_colors(4, seed=7)
    agent = mcts_oracle.OracleAgent(net)
    want, results = [], []
    for c in colors:
        g = OracleGame()
        while g.get_result() is None and len(g) < PLIES:
            if g.turn == c:
                assert g.move(agent.best_move(g, real_game=True))
            else:
                q.play_ply_q(g, 1, 2)
        want.append(g.get_history()["moves"])
        results.append(g.get_result())
    assert out["games"] == want
    assert {k: out[k] for k in ("played", "won", "drawn")} == bm.tally(colors, results)
    assert True in colors and False in colors                   # both colours were played


def test_gen_data_equals_the_cpu_loop(tmp_path):
    from chessrl_amd import gen_data as gd
    path = str(tmp_path / "games.json")
    n, opening, seed = 4, 4, 0
    d = gd.gen_data(path, num_games=n, depth=1, quiescence=2, opening_plies=opening, seed=seed, max_plies=256)
    draws = gd.draw_games(n, depth=1, random_dep=False, seed=seed)
    words = gd.opening_words(random.Random(seed), n, opening)
    saved = {rec.game_id: rec for rec in d.games}
    assert len(saved) == len(d) >= 1
    for i in range(n):
        is_white, game_depth, player_depth = draws[i]
        g = OracleGame()
        it = iter(int(w) for w in words[i])
        ru.run_in_slot(g, lambda: next(it), max_moves=opening)     # (StopIteration if the words did not suffice)
        assert len(g) == opening
        while g.get_result() is None and len(g) < 256:
            q.play_ply_q(g, player_depth if g.turn == is_white else game_depth, 2)
        if g.get_result() is None:                                  # still running after 256 plies: dropped
            assert i not in saved
            continue
        hist = saved[i].get_history()
        assert hist["moves"] == g.get_history()["moves"]          # every move replayed legally in the oracle
        assert hist["result"] == g.get_result()
        assert hist["player_color"] == is_white


# ---- 7 ---------------------------------------------------------------------------------------------------------
G, SIMS, REPLY_DEPTH, REPLY_Q = 16, 48, 1, 2


@functools.lru_cache(maxsize=None)
def tree(root, limit, mode):
    """(SearchResult, log) of root ``root`` against the depth-1, quiescence-2 opponent: computed once, never changed."""
    agent = q.ReplyAgentQ(u.net(), REPLY_DEPTH, REPLY_Q, limit)
    r = mcts_oracle.search(u.roots()[root], agent, SIMS, noise=False, mode=mode)
    return r, tuple(agent.log)


def engine(limit, rows, **kw):
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.opponent import MinimaxPlayer
    reply = MinimaxPlayer(False, search_depth=REPLY_DEPTH, node_limit=limit, quiescence=REPLY_Q)
    eng = LockstepEngine(u.net().to("cuda:0"), n_games=len(rows), max_sims=SIMS, reply=reply, numpy_promotion="nep50",
                         **kw)
    u.load_games(eng.ctx, [u.roots()[i] for i in rows])
    return eng


def check_trees(eng, rows, limit, what):
    eng.search(SIMS)
    rc = eng.root_children()
    nodes, cuts = eng.reply_stats()
    n_cut = 0
    for k, i in enumerate(rows):
        r, log = tree(i, limit, "nep50")
        u.assert_tree_equal(rc, k, r, what)
        cut = sum(1 for _, _, _, flag in log if flag == ou.CUT)
        assert (int(nodes[k]), int(cuts[k])) == (sum(n for _, _, n, _ in log), cut), (what, i)
        n_cut += cut
    return n_cut


@pytest.mark.parametrize("graph", [True, False])
def test_reply_trees_equal_the_restatement(graph):
    rows = list(range(G))
    eng = engine(ou.NODE_LIMIT, rows, use_graph=graph, steps_per_graph=8)
    assert [p for _, p in eng._plan] == ["phase_select_expand", "phase_reply_opponent", "phase_tower_s2"]
    assert check_trees(eng, rows, ou.NODE_LIMIT, ("graph", graph)) == 0
    eng.close()
    # the quiescence changed replies: the trees are not those of the depth-1 opponent without it
    differ = sum(1 for i in rows if u.reply_ids(tree(i, ou.NODE_LIMIT, "nep50")[0])
                 != u.reply_ids(u.tree(i, REPLY_DEPTH, ou.NODE_LIMIT, SIMS, "nep50")[0]))
    print("roots whose replies differ from quiescence 0:", differ)
    assert differ > 0


def test_agent_engine_cache_keys_on_quiescence():
    from chessrl_amd.agent import Agent
    from chessrl_amd.opponent import MinimaxPlayer
    agent = Agent(True, model=u.net().to("cuda:0"))
    plain = agent.engine_for(8, reply=MinimaxPlayer(False, 1))
    deep = agent.engine_for(8, reply=MinimaxPlayer(False, 1, quiescence=2))
    assert deep is not plain and (plain.reply.quiescence, deep.reply.quiescence) == (0, 2)
    assert agent.engine_for(8, reply=MinimaxPlayer(True, 1, quiescence=2)) is deep


def test_reply_under_a_node_limit_that_cuts():
    _, log = tree(u.MIDDLEGAME, ou.NODE_LIMIT, "nep50")
    counts = sorted(n for _, _, n, _ in log)
    limit = counts[len(counts) // 2]                           # the median: about half of that root's replies are cut
    rows = list(range(u.N_PREFIX, G))
    eng = engine(limit, rows)
    n_cut = check_trees(eng, rows, limit, ("limit", limit))
    print("limit", limit, "cut replies", n_cut)
    assert n_cut >= 1
    eng.close()
