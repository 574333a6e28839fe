"""GPU: the built-in opponent (csrc/opponent.hpp; stockfish.py:23-31, gamestockfish.py:27-41) against its CPU
restatement (tests/opponent_util.py).

1. move, score, node count and flag of 16 roots at depths 1, 2 (and 3 on the small ones) equal ``alphabeta``;
2. known answers through the C-ABI: mate in 1, stalemate avoidance, the fifty-move claim, the cut;
3. ``push`` equals ``crl_push_moves`` of the returned move; finished games; the window;
4. the refusals;
5. ``GameOpponent`` + ``MinimaxPlayer`` one move at a time, and ``benchmark`` in lockstep, against CPU loops;
6. ``gen_data`` against ``run_in_slot`` + ``alphabeta``;
7. two runs give identical node counts.
Integer work only: every comparison is exact.
"""
import ctypes
import functools
import random

import numpy as np
import pytest

from oracle import mcts_oracle
from oracle.chess_oracle import OracleGame, board_from_fen, board_to_array, move_to_uci
from oracle.fakenet import FakeNet
from tests import opponent_util as ou
from tests import rollout_util as ru

pytestmark = pytest.mark.gpu

NO_MOVE, RESULT_NONE = 0xFFFF, 2
DEPTH3 = ("kpk", "kbkn", "clock_96", "kqk", "blocked", "stalemate_near", "knight_shuffle", "king_shuffle")
CLOCK_98 = "7k/8/4K3/8/6Q1/8/8/8 w - - 98 80"
TWIN = 37                                      # slot 37 holds the root of slot 0 once more


@functools.lru_cache(maxsize=None)
def roots():
    return ru.private_roots()


@functools.lru_cache(maxsize=None)
def reference(depth):
    """``alphabeta`` of every root at ``depth`` (None where the depth-3 set leaves the root out), computed once."""
    return tuple(ou.alphabeta(g, depth) if depth < 3 or name in DEPTH3 else None for name, g in roots())


def load_games(ctx, games):
    """Slot i of the context becomes games[i]: its first position, then its move list."""
    ctx.set_positions(np.stack([board_to_array(g.board_at(len(g))) for g in games]))
    n = max(max(len(g) for g in games), 1)
    tbl = np.full((len(games), n), NO_MOVE, np.uint16)
    cnt = np.array([len(g) for g in games], np.int32)
    for i, g in enumerate(games):
        tbl[i, :len(g)] = [g.board.move_stack[k].m for k in range(len(g))]
    assert list(ctx.push_sequences(tbl, cnt)) == list(cnt)


def slot_games():
    """64 slots: slot s holds root s % 16, slot TWIN holds root 0."""
    gs = [g for _, g in roots()]
    return [gs[0] if s == TWIN else gs[s % 16] for s in range(64)]


def context64():
    from chessrl_amd import _lib
    ctx = _lib.Context(64, 1, max_plies=256)
    load_games(ctx, slot_games())
    return ctx


def depth_row(depth):
    row = np.zeros(64, np.int32)
    for i, ref in enumerate(reference(depth)):
        if ref is not None:
            row[i] = depth
    row[TWIN] = row[0]
    return row


def state(ctx):
    return [ctx.get_positions().copy()] + [a.copy() for a in ctx.records()]


def same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. restatement equality, 7. run to run ----------------------------------------------------------------
def test_search_equals_the_restatement_and_repeats_itself():
    ctx = context64()
    before = state(ctx)
    for depth in (1, 2, 3):
        row = depth_row(depth)
        moves, scores, nodes, flags = ctx.opponent_moves(row)
        for i, ref in enumerate(reference(depth)):
            name = roots()[i][0]
            if ref is None:
                assert row[i] == 0
                continue
            got = (int(moves[i]), int(scores[i]), int(nodes[i]), int(flags[i]))
            print(name, depth, move_to_uci(got[0]), got[1:], "restated", ref)
            assert got == ref, (name, depth)
        assert (moves[TWIN], scores[TWIN], nodes[TWIN], flags[TWIN]) == (moves[0], scores[0], nodes[0], flags[0])
        idle = row == 0
        assert (moves[idle] == NO_MOVE).all() and not scores[idle].any() and not nodes[idle].any() and not flags[idle].any()
        again = ctx.opponent_moves(row)
        assert all(np.array_equal(a, b) for a, b in zip((moves, scores, nodes, flags), again))
    assert same_state(state(ctx), before)          # nothing was pushed, no slot was touched
    ctx.close()


# ---- 2. known answers through the C-ABI --------------------------------------------------------------------
def test_known_answers():
    from chessrl_amd import _lib
    names = [n for n, _ in roots()]
    games = [dict(roots())[n] for n in ("back_rank_white", "back_rank_black", "stalemate_near", "clock_96", "218_moves")]
    games.append(OracleGame(board=board_from_fen(CLOCK_98)))
    ctx = _lib.Context(len(games), 1, max_plies=16)
    load_games(ctx, games)
    m1, s1, n1, f1 = ctx.opponent_moves([1, 1, 1, 1, 0, 0])
    assert [move_to_uci(m) for m in m1[:2]] == ["a1a8", "a8a1"] and list(s1[:2]) == [29999, 29999]
    assert list(n1[:2]) == [1 + len(g.legal_move_ids()) for g in games[:2]]
    m2, s2, n2, f2 = ctx.opponent_moves([0, 0, 2, 2, 2, 2])
    for m in (m1[2], m2[2]):                                   # neither depth stalemates
        after = ou.child(games[2], int(m))
        assert after.get_result() is None and move_to_uci(m) not in ("g5g6", "g5h6")
    assert s1[2] > 800 and s2[2] > 800
    assert s2[3] > 800 and s2[5] == 0                          # clock 98 at the horizon; clock 100: the claim
    assert not f1.any() and not f2.any()
    # the cut, on the 218-move root
    legal = games[4].legal_move_ids()
    full = int(n2[4])
    only = np.array([0, 0, 0, 0, 2, 0], np.int32)
    for limit in (full + 1, full, full - 1, full // 2, 1):
        got = ctx.opponent_moves(only, node_limit=limit)
        got = (int(got[0][4]), int(got[1][4]), int(got[2][4]), int(got[3][4]))
        want = ou.alphabeta(games[4], 2, node_limit=limit)
        print("limit", limit, got, "restated", want)
        assert got == want
        assert (got[3] == ou.CUT) == (limit < full) and got[0] in legal
    assert names.index("218_moves") == 13
    ctx.close()


# ---- 3. push -------------------------------------------------------------------------------------------------
# both kings shuffle behind locked pawns (rollout_util.BLOCKED): from a1 only Kb1 is legal, from a8 only Kb8.  After
# these 16 plies the position (Kb1, kb8, white to move) has occurred four times, the two positions on the way to
# it twice and once: the next two plies are forced and the second makes the fifth occurrence.
FORCED_FIFTH = ["a1b1", "a8b8"] + ["b1a1", "b8c8", "a1b1", "c8b8"] * 3 + ["b1a1", "b8a8"]
FIFTH_SLOT = 38


def forced_fifth_game():
    g = OracleGame(board=board_from_fen(ru.BLOCKED))
    for u in FORCED_FIFTH:
        assert g.move(u), u
    assert g.get_result() is None and [move_to_uci(m) for m in g.legal_move_ids()] == ["a1b1"]
    return g


def test_push_equals_push_moves_of_the_returned_move():
    from chessrl_amd import _lib
    games = slot_games()
    games[FIFTH_SLOT] = forced_fifth_game()
    a, b = _lib.Context(64, 1, max_plies=256), _lib.Context(64, 1, max_plies=256)
    load_games(a, games)
    load_games(b, games)
    row = depth_row(1)
    row[16:32] = 2                                              # the same roots once more, one ply deeper
    row[FIFTH_SLOT] = 1
    for ply in range(3):
        moves, _, _, flags = a.opponent_moves(row, push=True)
        running = b.results() == RESULT_NONE
        want_skip = (row > 0) & ~running
        assert ((flags == ou.SKIPPED) == want_skip).all() and (moves[want_skip] == NO_MOVE).all()
        assert (moves[(row > 0) & running] != NO_MOVE).all() and (moves[row == 0] == NO_MOVE).all()
        ok = b.push_moves(moves)
        assert (ok == (moves != NO_MOVE)).all()
        assert same_state(state(a), state(b))
        # the forced line: running after one ply, drawn by the fifth occurrence after two, skipped in the third
        assert (int(a.results()[FIFTH_SLOT]), int(flags[FIFTH_SLOT])) == ((RESULT_NONE, 0), (0, 0), (0, ou.SKIPPED))[ply]
    res = a.results()
    assert res[8] == 1 and res[9] == -1                         # the back-rank mates were delivered
    plies = a.records()[1]
    assert plies[FIFTH_SLOT] == len(FORCED_FIFTH) + 2
    idle = row == 0
    assert (plies[idle] == np.array([len(g) for g in games])[idle]).all()          # depth 0: untouched
    a.close()
    b.close()


def test_finished_games_and_the_window():
    ctx = context64()
    mate = np.full(64, NO_MOVE, np.uint16)
    mate[8], mate[9] = ou.alphabeta(roots()[8][1], 1)[0], ou.alphabeta(roots()[9][1], 1)[0]
    ctx.push_moves(mate)
    assert list(ctx.results()[8:10]) == [1, -1]
    before = state(ctx)
    moves, scores, nodes, flags = ctx.opponent_moves(np.full(64, 1, np.int32), push=True)
    assert list(moves[8:10]) == [NO_MOVE, NO_MOVE] and list(flags[8:10]) == [ou.SKIPPED, ou.SKIPPED]
    assert not nodes[8:10].any() and not scores[8:10].any()
    assert (flags == ou.SKIPPED).sum() == 2
    after = state(ctx)
    assert all(np.array_equal(x[8:10], y[8:10]) for x, y in zip(before, after))
    assert (after[2] == before[2] + (flags != ou.SKIPPED)).all()
    # the window: rows are window-relative, slots outside it are left alone
    depths = np.array([2, 0, 2, 2], np.int32)
    expect = (depths > 0) & (after[3][32:36] == RESULT_NONE)
    assert expect.sum() >= 2
    ctx.set_window(32, 4)
    m, s, n, f = ctx.opponent_moves(depths, push=True)
    ctx.set_window(0, 64)
    final = state(ctx)
    changed = np.zeros(64, bool)
    changed[32:36] = expect
    assert (final[2] == after[2] + changed).all()
    assert all(np.array_equal(x[~changed], y[~changed]) for x, y in zip(after, final))
    assert ((m != NO_MOVE) == expect).all()
    assert all(final[1][32 + i, final[2][32 + i] - 1] == m[i] for i in range(4) if expect[i])
    ctx.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from chessrl_amd import _lib
    ctx = context64()
    before = state(ctx)
    L, h = ctx._L, ctx._h
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    moves, good = np.zeros(64, np.uint16), np.full(64, 1, np.int32)
    deep, negative = good.copy(), good.copy()
    deep[63], negative[5] = 6, -1
    assert L.crl_opponent_moves(h, ptr(deep), 1, 1000, ptr(moves), None, None, None) == -1
    assert L.crl_opponent_moves(h, ptr(negative), 1, 1000, ptr(moves), None, None, None) == -1
    assert L.crl_opponent_moves(h, ptr(good), 1, 0, ptr(moves), None, None, None) == -1
    assert L.crl_opponent_moves(h, None, 1, 1000, ptr(moves), None, None, None) == -1
    assert L.crl_opponent_moves(h, ptr(good), 1, 1000, None, None, None, None) == -1
    assert same_state(state(ctx), before)
    with pytest.raises(_lib.HipLibraryError):
        ctx.opponent_moves(deep)
    # scores, nodes and flags may be NULL
    assert L.crl_opponent_moves(h, ptr(good), 0, 1000, ptr(moves), None, None, None) == 0
    assert np.array_equal(moves, ctx.opponent_moves(good, node_limit=1000)[0])
    assert same_state(state(ctx), before)
    ctx.close()


# ---- 5. drop-in and batched play -----------------------------------------------------------------------------
PLIES = 24


def cpu_game_against_opponent(player_white, player_depth, opponent_depth):
    """gen_data_stockfish.play_game's loop on the oracle: ``bm = player.best_move(g); g.move(bm)``."""
    g = OracleGame()
    while g.get_result() is None and len(g) < PLIES:
        if not player_white and len(g) == 0:
            ou.play_ply(g, opponent_depth)
        else:
            ou.play_ply(g, player_depth)
            if g.get_result() is None:
                ou.play_ply(g, opponent_depth)
    return g.get_history()["moves"], g.get_result()


@pytest.mark.parametrize("player_white", [True, False])
def test_game_opponent_one_move_at_a_time(player_white):
    from chessrl_amd.opponent import GameOpponent, MinimaxPlayer
    player = MinimaxPlayer(player_white, search_depth=1)
    g = GameOpponent(player_color=player_white, opponent_depth=2) if player_white else \
        GameOpponent(opponent=MinimaxPlayer(True, search_depth=2), player_color=False)
    assert g.opponent.color is (not player_white) and g.opponent.search_depth == 2
    while g.get_result() is None and len(g) < PLIES:
        g.move(player.best_move(g))
    hist = g.get_history()
    copy = g.get_copy()
    assert copy.opponent is g.opponent and copy.get_history()["moves"] == hist["moves"]
    copy.free()
    g.tearup()
    g.free()
    assert g.opponent is None
    assert (hist["moves"], hist["result"]) == cpu_game_against_opponent(player_white, 1, 2)
    assert len(hist["moves"]) >= PLIES


def test_minimax_player_on_a_finished_game():
    from chessrl_amd.game import Game
    from chessrl_amd.opponent import MinimaxPlayer
    g = Game(board="6k1/5ppp/8/8/8/8/8/R5K1 w - - 0 1")
    p = MinimaxPlayer(True, search_depth=1)
    assert p.best_move(g) == "a1a8" and p.last == (29999, 1 + len(g.get_legal_moves()), 0)
    assert g.move("a1a8") and g.get_result() == 1
    assert p.best_move(g) == "00000" and p.last[2] == ou.SKIPPED
    assert p.kill() is None
    g.free()
    with pytest.raises(ValueError):
        MinimaxPlayer(True, search_depth=6)


def test_benchmark_equals_the_cpu_loop():
    from chessrl_amd import benchmark as bm
    net = FakeNet(seed=5, prior_shift=29)
    out = bm.benchmark(None, games=4, opponent_depth=2, seed=7, max_plies=PLIES, model=net.to("cuda:0"))
    colors = bm.game_colors(4, seed=7)
    agent = mcts_oracle.OracleAgent(net)
    want, results = [], []
    for c in colors:
        g = OracleGame()
        while g.get_result() is None and len(g) < PLIES:
            if g.turn == c:
                assert g.move(agent.best_move(g, real_game=True))
            else:
                ou.play_ply(g, 2)
        want.append(g.get_history()["moves"])
        results.append(g.get_result())
    assert out["games"] == want
    assert {k: out[k] for k in ("played", "won", "drawn")} == bm.tally(colors, results)
    assert True in colors and False in colors                   # both colours were played


# ---- 6. gen_data -----------------------------------------------------------------------------------------------
def test_gen_data_equals_the_cpu_loop(tmp_path):
    from chessrl_amd import gen_data as gd
    from chessrl_amd.dataset import DatasetGame
    path = str(tmp_path / "games.json")
    n, opening, seed = 4, 4, 0
    d = gd.gen_data(path, num_games=n, depth=1, opening_plies=opening, seed=seed, max_plies=256)
    draws = gd.draw_games(n, depth=1, random_dep=False, seed=seed)
    words = gd.opening_words(random.Random(seed), n, opening)
    assert len(d) == n
    for rec in d.games:
        i = rec.game_id
        is_white, game_depth, player_depth = draws[i]
        g = OracleGame()
        it = iter(int(w) for w in words[i])
        ru.run_in_slot(g, lambda: next(it), max_moves=opening)     # (StopIteration if the words did not suffice)
        assert len(g) == opening
        while g.get_result() is None and len(g) < 256:
            ou.play_ply(g, player_depth if g.turn == is_white else game_depth)
        hist = rec.get_history()
        assert hist["moves"] == g.get_history()["moves"]          # every move replayed legally in the oracle
        assert hist["result"] == g.get_result() and hist["result"] is not None
        assert hist["player_color"] == is_white
    back = DatasetGame()
    back.load(path)
    assert [g.get_history()["moves"] for g in back.games] == [r.get_history()["moves"] for r in d.games]
    assert [g.get_history()["result"] for g in back.games] == [r.get_history()["result"] for r in d.games]
    for g in back.games:
        g.free()
