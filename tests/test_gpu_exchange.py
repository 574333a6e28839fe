"""GPU: the built-in opponent's delta and exchange pruning in quiescence (csrc/opponent.hpp EXCHANGE; the
EXC shapes of the ``k_opponent_moves_id`` / ``k_reply_opponent_id`` kernel templates and ``k_opponent_exchange``) against its CPU restatement
(tests/exchange_util.py; the restatement itself is held to its definition, to the existing restatements and to the
preconditions of these roots without a GPU in tests/test_exchange_cpu.py).

1. ``opponent_moves(exchange=True)``: move, score, node count, flag and completed depth equal the restatement on the
   roots of ``exchange_util.games()`` in every case of ``exchange_util.CASES`` (all eight kernel shapes, maximum depths
   2 to 4, Q in {1, 2, 4}, budgets that are reached and budgets that are not);
2. ``Context.opponent_exchange()``: the two bits of every legal move of 64 positions -- random games, the hand-made
   positions and one with 218 legal moves, so that all four passes of the kernel run;
3. off is the parent: ``exchange=False`` gives what the call without the keyword gives, and ``exchange = 0`` through
   the new entry what the ``_sel`` entry gives; the refusals change nothing;
4. ``LockstepEngine(reply=MinimaxPlayer(..., exchange=True))``: the trees and the three accumulators against
   ``oracle.mcts_oracle.search`` whose mover is the restatement.
Integer work only: every comparison is exact.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import mcts_oracle
from oracle.chess_oracle import move_to_uci
from tests import exchange_util as xu
from tests import opponent_reply_util as u
from tests import opponent_util as ou
from tests import ordering_util as od
from tests import test_gpu_opponent as tg

pytestmark = pytest.mark.gpu

NO_MOVE = 0xFFFF
SLOTS = 16                                     # at most 16 slots per launch
N_GAMES = len(xu.games())


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def slot_games():
    """16 slots: slot s < N_GAMES holds root s, the others root s % N_GAMES once more."""
    gs = [g for _, g in xu.games()]
    assert N_GAMES <= SLOTS
    return [gs[s % N_GAMES] for s in range(SLOTS)]


@pytest.fixture(scope="module")
def ctx16():
    from chessrl_amd import _lib
    ctx = _lib.Context(SLOTS, 1, max_plies=64)
    tg.load_games(ctx, slot_games())
    yield ctx
    ctx.close()


def settings(case):
    depth, quiescence, budget, repetition, evaluation, selective = case
    return depth, dict(quiescence=quiescence, node_budget=budget, ordering=True, repetition=repetition,
                       evaluation=evaluation, selective=selective)


# ---- 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", xu.CASES, ids=lambda c: "D%d-Q%d-B%d-%s-%s-%s" % (
    c[0], c[1], c[2], "rep" if c[3] else "norep", c[4], "sel" if c[5] else "full"))
def test_search_equals_the_restatement(ctx16, case):
    ctx = ctx16
    before = tg.state(ctx)
    depth, kw = settings(case)
    row = np.full(SLOTS, depth, np.int32)
    got = ctx.opponent_moves(row, exchange=True, **kw)
    moves, scores, nodes, flags, done = got
    rows = xu.reference(*case)[0]
    for i, ref in enumerate(rows):
        name = xu.games()[i][0]
        one = (int(moves[i]), int(scores[i]), int(nodes[i]), int(flags[i]), int(done[i]))
        print(name, case, move_to_uci(one[0]), one[1:], "restated", ref)
        assert one == ref, (name, case)
    for s in range(N_GAMES, SLOTS):                             # the same root once more: the same answer
        assert all(a[s] == a[s % N_GAMES] for a in got)
    assert nodes.max() <= case[2]
    full = ctx.opponent_moves(row, **kw)
    assert not all(np.array_equal(a, b) for a, b in zip(got, full))        # the filter reaches the searches of the case
    off = xu.reference(*case, exchange=False)[0]
    for i, ref in enumerate(off):                               # ... and without it the kernels are their siblings
        assert (int(full[0][i]), int(full[1][i]), int(full[2][i]), int(full[3][i]), int(full[4][i])) == ref
    again = ctx.opponent_moves(row, exchange=True, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))           # nothing of one search reaches the next
    assert tg.same_state(tg.state(ctx), before)                 # nothing was pushed, no slot was touched


def test_the_cases_reach_and_do_not_reach_their_budgets():
    cut = whole = 0
    for case in xu.CASES:
        for r in xu.reference(*case)[0]:
            cut += r[3] == ou.CUT
            whole += r[3] == 0
    assert cut > 0 and whole > 0


def test_push_plays_the_move():
    from chessrl_amd import _lib
    a, b = _lib.Context(SLOTS, 1, max_plies=64), _lib.Context(SLOTS, 1, max_plies=64)
    tg.load_games(a, slot_games())
    tg.load_games(b, slot_games())
    case = xu.CASES[1]
    depth, kw = settings(case)
    moves = a.opponent_moves(np.full(SLOTS, depth, np.int32), push=True, exchange=True, **kw)[0]
    assert [int(m) for m in moves[:N_GAMES]] == [r[0] for r in xu.reference(*case)[0]]
    assert (b.push_moves(moves) == (moves != NO_MOVE)).all()
    assert tg.same_state(tg.state(a), tg.state(b))
    a.close()
    b.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------
def exchange_positions():
    """64 positions: the hand-made ones, the root with 218 legal moves and 57 from random games."""
    big = dict(od.games())[xu.BIG_ROOT]
    assert len(big.legal_move_ids()) == 218                     # more than 64, more than 192: all four passes
    rnd = xu.random_positions()
    picked = [rnd[i] for i in range(5, len(rnd), max(1, (len(rnd) - 5) // 57))][:57]
    out = [g for _, g in xu.hand_made_games()] + [big] + picked
    assert len(out) == 64
    return out


def test_exchange_bits_of_every_legal_move():
    from chessrl_amd import _lib
    games = exchange_positions()
    ctx = _lib.Context(64, 1, max_plies=64)
    tg.load_games(ctx, games)
    before = tg.state(ctx)
    bits, counts = ctx.opponent_exchange()
    moves, legal_counts = ctx.legal_moves()
    assert np.array_equal(counts, legal_counts) and bits.shape == (64, _lib.MAX_MOVES) and bits.dtype == np.uint8
    tactical = removed = 0
    for s, g in enumerate(games):
        ids = g.legal_move_ids()
        assert int(counts[s]) == len(ids) and [int(m) for m in moves[s, :len(ids)]] == ids, s
        for i, m in enumerate(ids):
            t, kept = xu.judge(g, m)
            assert int(bits[s, i]) == (1 if t else 0) | (2 if kept else 0), (s, g.get_fen(), move_to_uci(m))
            tactical += t
            removed += not kept
        assert not bits[s, len(ids):].any()
    print("tactical moves:", tactical, "removed by the exchange test:", removed)
    assert tactical > 100 and 20 < removed < tactical
    assert counts.max() == 218 and (counts > 64).sum() == 1
    again = ctx.opponent_exchange()
    assert np.array_equal(again[0], bits) and np.array_equal(again[1], counts)
    assert tg.same_state(tg.state(ctx), before)
    assert ctx._L.crl_opponent_exchange(ctx._h, None, ptr(counts)) == -1
    assert ctx._L.crl_opponent_exchange(ctx._h, ptr(bits), None) == -1
    ctx.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------
def outputs():
    return (np.zeros(SLOTS, np.uint16), np.zeros(SLOTS, np.int32), np.zeros(SLOTS, np.int64),
            np.zeros(SLOTS, np.uint8), np.zeros(SLOTS, np.int32))


def test_off_is_the_parent(ctx16):
    ctx = ctx16
    L, h = ctx._L, ctx._h
    for case in xu.CASES[1:6]:
        depth, kw = settings(case)
        row = np.full(SLOTS, depth, np.int32)
        without = ctx.opponent_moves(row, **kw)
        off = ctx.opponent_moves(row, exchange=False, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(without, off))
        old, new = outputs(), outputs()
        args = (kw["quiescence"], 0, kw["node_budget"], 1, int(kw["repetition"]),
                int(kw["evaluation"] == "positional"), int(kw["selective"]))
        assert L.crl_opponent_moves_sel(h, ptr(row), *args, *[ptr(a) for a in old]) == 0
        assert L.crl_opponent_moves_exc(h, ptr(row), *args, 0, *[ptr(a) for a in new]) == 0
        assert all(np.array_equal(a, b) for a, b in zip(old, new))
        assert all(np.array_equal(a, b) for a, b in zip(old, without))
    # exchange = 0 whatever the other settings: ordering off and no quiescence plies included
    row = np.full(SLOTS, 2, np.int32)
    for quiescence, ordering in ((0, 0), (0, 1), (2, 0)):
        old, new = outputs(), outputs()
        assert L.crl_opponent_moves_sel(h, ptr(row), quiescence, 0, 100, ordering, 0, 0, 0, *[ptr(a) for a in old]) == 0
        assert L.crl_opponent_moves_exc(h, ptr(row), quiescence, 0, 100, ordering, 0, 0, 0, 0,
                                        *[ptr(a) for a in new]) == 0
        assert all(np.array_equal(a, b) for a, b in zip(old, new))


def test_refusals_change_nothing(ctx16):
    from chessrl_amd.opponent import GameOpponent
    import torch
    ctx = ctx16
    before = tg.state(ctx)
    L, h = ctx._L, ctx._h
    moves, good = np.zeros(SLOTS, np.uint16), np.full(SLOTS, 1, np.int32)
    call = lambda Q, budget, ordering, sel, exc: L.crl_opponent_moves_exc(
        h, ptr(good), Q, 1, budget, ordering, 0, 0, sel, exc, ptr(moves), None, None, None, None)
    for exc in (2, -1):
        assert call(2, 100, 1, 0, exc) == -1
    assert call(2, 100, 0, 0, 1) == -1                          # exchange without ordering
    assert call(0, 100, 1, 0, 1) == -1                          # ... without quiescence plies
    assert call(2, 0, 1, 0, 1) == -1 and call(7, 100, 1, 0, 1) == -1 and call(2, 100, 0, 1, 1) == -1
    assert tg.same_state(tg.state(ctx), before)                 # push = 1 in every call: nothing was launched
    dev = torch.zeros(SLOTS, dtype=torch.int64, device="cuda:0").data_ptr()
    reply = lambda Q, budget, ordering, exc, acc: L.crl_sim_reply_opponent_exc(
        h, dev, Q, budget, ordering, 0, 0, 0, exc, dev, dev, dev, acc)
    assert reply(2, 100, 1, 2, dev) == -1 and reply(2, 100, 0, 1, dev) == -1 and reply(0, 100, 1, 1, dev) == -1
    assert reply(2, 100, 1, 1, None) == -1 and reply(2, 0, 1, 1, dev) == -1
    row = np.full(SLOTS, 2, np.int32)
    with pytest.raises(ValueError, match="exchange needs ordering"):
        ctx.opponent_moves(row, node_budget=100, quiescence=2, exchange=True)
    with pytest.raises(ValueError, match="ordering needs a node_budget"):
        ctx.opponent_moves(row, ordering=True, quiescence=2, exchange=True)
    with pytest.raises(ValueError, match="exchange needs quiescence"):
        ctx.opponent_moves(row, node_budget=100, ordering=True, exchange=True)
    with pytest.raises(ValueError, match="exchange needs quiescence"):
        ctx.sim_reply_opponent(dev, 1000, dev, dev, dev, node_budget=100, dev_depth_sum=dev, ordering=True,
                               exchange=True)
    with pytest.raises(ValueError, match="exchange needs ordering"):
        GameOpponent(opponent_budget=100, opponent_quiescence=2, opponent_exchange=True)
    assert tg.same_state(tg.state(ctx), before)


# ---- 4 ---------------------------------------------------------------------------------------------------------
SIMS, REPLY_DEPTH, REPLY_Q, BUDGET = 16, 3, 2, 150
REPLY_ROOTS = (5, u.N_PREFIX, u.MIDDLEGAME, u.FEN0 + 2)        # a random prefix, the start, a middlegame, promotions


@functools.lru_cache(maxsize=None)
def tree(root, exchange, mode="nep50"):
    """(SearchResult, log) of root ``root`` against the ordered opponent of maximum depth 3, Q = 2 under BUDGET."""
    agent = xu.ReplyAgentExc(u.net(), REPLY_DEPTH, BUDGET, REPLY_Q, exchange=exchange)
    r = mcts_oracle.search(u.roots()[root], agent, SIMS, noise=False, mode=mode)
    return r, tuple(agent.log)


@pytest.mark.parametrize("graph", [True, False])
def test_reply_trees_equal_the_restatement(graph):
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.opponent import MinimaxPlayer
    from chessrl_amd.searchmode import SearchMode
    roots = [u.roots()[i] for i in REPLY_ROOTS]
    reply = MinimaxPlayer(False, REPLY_DEPTH, quiescence=REPLY_Q, node_budget=BUDGET, ordering=True, exchange=True)
    eng = LockstepEngine(u.net().to("cuda:0"), n_games=len(roots), max_sims=SIMS, reply=reply,
                         numpy_promotion="nep50", use_graph=graph, steps_per_graph=3)
    u.load_games(eng.ctx, roots)
    assert eng.reply.exchange is True
    plain = MinimaxPlayer(False, REPLY_DEPTH, quiescence=REPLY_Q, node_budget=BUDGET, ordering=True)
    assert SearchMode(reply=reply).key != SearchMode(reply=plain).key
    assert SearchMode(reply=plain).key[2][:8] == SearchMode(reply=reply).key[2][:8]    # appended to the tuple
    eng.search(SIMS)
    rc = eng.root_children()
    nodes, cuts, depth_sum = eng.reply_stats()
    for i, root in enumerate(REPLY_ROOTS):
        r, log = tree(root, True)
        u.assert_tree_equal(rc, i, r, ("graph", graph))
        want = (sum(n for _, _, n, _, _ in log), sum(1 for e in log if e[3] == ou.CUT), sum(e[4] for e in log))
        assert (int(nodes[i]), int(cuts[i]), int(depth_sum[i])) == want, (graph, i)
        assert all((e[3] == ou.CUT) == (e[4] < REPLY_DEPTH) and e[2] <= BUDGET for e in log)
    eng.close()
    changed = [i for i in REPLY_ROOTS if tree(i, True)[1] != tree(i, False)[1]]
    print("roots whose reply logs differ from the unpruned opponent's:", changed)
    assert changed                                              # the filter reaches the trees


def test_minimax_player_and_benchmark_line(capsys):
    from chessrl_amd import benchmark as bm
    from chessrl_amd.game import Game
    from chessrl_amd.opponent import MinimaxPlayer
    from oracle.fakenet import FakeNet
    g = Game(board=xu.MIDDLEGAME_FEN)
    root = xu.from_fen(xu.MIDDLEGAME_FEN)
    p = MinimaxPlayer(True, search_depth=3, quiescence=2, node_budget=400, ordering=True, repetition=True,
                      evaluation="positional", selective=True, exchange=True)
    want = xu.search(root, 3, 400, 2, True, "positional", True)
    assert p.best_move(g) == move_to_uci(want[0]) and p.last == want[1:4] and p.last_depth == want[4]
    g.free()
    net = FakeNet(seed=5, prior_shift=29)
    bm.benchmark(None, games=2, opponent_depth=2, opponent_quiescence=1, opponent_budget=40, seed=7, max_plies=2,
                 model=net.to("cuda:0"), log=True, opponent_ordering=True, opponent_exchange=True)
    assert ("within 40 nodes per move, ordered, quiescence 1, exchange-pruned (not stockfish, no elo)"
            in capsys.readouterr().out.lower())
    with pytest.raises(ValueError, match="exchange needs quiescence"):
        bm.benchmark(None, games=2, opponent_budget=20, model=net.to("cuda:0"), opponent_ordering=True,
                     opponent_exchange=True)
