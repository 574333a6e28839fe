"""GPU: the one-ply move boundary (crl_advance_one) and the arena built on it.

The weight sets are FakeNets -- exact integer functions of the planes -- so the device's games are compared with the
CPU restatement (tests/arena_util.py over oracle.mcts_oracle and OracleGame) move for move and result for result;
tests/test_arena_cpu.py checks with the oracle alone that the set is worth comparing.
"""
import numpy as np
import pytest

from oracle import mcts_oracle
from oracle.chess_oracle import OracleGame, board_from_fen, board_to_array, move_to_uci, uci_to_move
from oracle.fakenet import FakeNet
from tests import arena_util as au
from tests import rollout_util as ru
from tests.util import oracle_row

pytestmark = pytest.mark.gpu

NO_MOVE, RESULT_NONE = 0xFFFF, 2
START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
SIMS = 24


def device_nets():
    a, b = au.nets()
    return a.to("cuda:0"), b.to("cuda:0")


def load(ctx, games):
    """slot i of the window becomes OracleGame ``games[i]``: its root position, then its move stack"""
    rows, lists = [], []
    for g in games:
        n = len(g)
        rows.append(board_to_array(g.board_at(n)))
        lists.append([g.board.move_stack[i].m for i in range(n)])
    ctx.set_positions(np.stack(rows))
    width = max(1, max(len(m) for m in lists))
    table = np.full((len(games), width), NO_MOVE, np.uint16)
    for i, m in enumerate(lists):
        table[i, :len(m)] = m
    counts = np.array([len(m) for m in lists], np.int32)
    assert list(ctx.push_sequences(table, counts)) == list(counts)


def result_of(game):
    r = game.get_result()
    return RESULT_NONE if r is None else r


def same_game(ctx, slot, game):
    """position (every bit), ply, result and record of one slot against an OracleGame"""
    moves, plies, results = ctx.records()
    assert plies[slot] == len(game)
    assert list(ctx.get_positions()[slot]) == list(oracle_row(game))
    assert results[slot] == result_of(game)
    assert list(moves[slot, :plies[slot]]) == [game.board.move_stack[i].m for i in range(len(game))]


# ---- the one-ply advance ---------------------------------------------------------------------------------------------
def one_ply_roots():
    def from_ids(ids):
        g = OracleGame()
        for m in ids:
            assert g.move(move_to_uci(m))
        return g
    return [("start", OracleGame(), "first"),
            ("midgame_20", from_ids(ru.random_prefix(20, seed=20)), "last"),
            ("midgame_34", from_ids(ru.random_prefix(34, seed=34)), "first"),
            ("black_1", from_ids(ru.random_prefix(1, seed=1)), "last"),
            ("black_27", from_ids(ru.random_prefix(27, seed=27)), "first"),
            ("untouched_black_9", from_ids(ru.random_prefix(9, seed=9)), "none"),
            ("mate_queen", OracleGame(board=board_from_fen(au.FENS[0])), "mate"),
            ("mate_back_rank", OracleGame(board=board_from_fen(au.FENS[1])), "mate")]


def test_one_ply_advance_equals_one_move_of_the_oracle_game():
    from chessrl_amd.engine import LockstepEngine
    roots = one_ply_roots()
    G = len(roots)
    net = FakeNet(seed=3, prior_shift=30)
    eng = LockstepEngine(net.to("cuda:0"), n_games=G, max_sims=SIMS)
    games = [g for _, g, _ in roots]
    load(eng.ctx, games)
    for i, g in enumerate(games):
        same_game(eng.ctx, i, g)
    assert [g.turn for g in games] == [True, True, True, False, False, False, True, True]
    eng.search(SIMS)
    rc = eng.root_children()
    chosen = np.zeros(G, np.int32)
    for i, (name, g, which) in enumerate(roots):
        r = mcts_oracle.search(g, mcts_oracle.OracleAgent(net), SIMS, noise=False, mode=au.float_mode())
        n = int(rc["nchild"][i])
        assert [move_to_uci(m) for m in rc["moves"][i, :n]] == r.child_moves, name
        if which == "mate":
            mates = [k for k, mv in enumerate(r.child_moves) if _result_after(g, mv) == 1]
            assert mates, name
            chosen[i] = mates[0]
        else:
            chosen[i] = {"first": 0, "last": n - 1, "none": -1}[which]
    before = (eng.ctx.get_positions().copy(), [x.copy() for x in eng.ctx.records()])
    bm = eng.advance(chosen, plies=1)
    assert bm.dtype == np.uint16 and bm.shape == (G,)
    for i, (name, g, which) in enumerate(roots):
        if which == "none":
            assert bm[i] == NO_MOVE
            continue
        mv = move_to_uci(rc["moves"][i, chosen[i]])
        assert move_to_uci(bm[i]) == mv, name
        n0 = len(g)
        assert g.move(mv)
        assert len(g) == n0 + 1                                    # ONE ply: the stored reply is not played
    for i, (name, g, which) in enumerate(roots):
        same_game(eng.ctx, i, g)
        if which == "mate":
            assert g.get_result() == 1
    # the slot given -1: nothing of it changed, and its tree is still there
    u = [w for _, _, w in roots].index("none")
    assert list(before[0][u]) == list(eng.ctx.get_positions()[u])
    moves, plies, results = eng.ctx.records()
    assert plies[u] == before[1][1][u] and results[u] == before[1][2][u] and list(moves[u]) == list(before[1][0][u])
    assert eng.ctx.fetch_tree(u)[2]["root_visits"] == SIMS + 1
    for i, (_, _, which) in enumerate(roots):
        if which != "none":
            assert eng.ctx.fetch_tree(i)[2]["n_nodes"] == 0         # the tree is consumed
    # the next search starts a fresh tree in every running game, from the position one ply on
    eng.search(SIMS)
    rc = eng.root_children()
    for i, (name, g, which) in enumerate(roots):
        if g.get_result() is not None:
            assert rc["root_visits"][i] == 0 and rc["nchild"][i] == 0, name
            continue
        assert rc["root_visits"][i] == SIMS + 1, name
        r = mcts_oracle.search(g, mcts_oracle.OracleAgent(net), SIMS, noise=False, mode=au.float_mode())
        n = int(rc["nchild"][i])
        assert list(rc["visits"][i, :n]) == r.visits, name
        assert [move_to_uci(m) for m in rc["moves"][i, :n]] == r.child_moves, name
    eng.close()


def _result_after(game, mv):
    c = game.get_copy()
    assert c.move(mv)
    return c.get_result()


def test_fivefold_repetition_reached_by_one_ply_advances():
    """One cycle of the knight shuffle is loaded (the start position has occurred twice); twelve one-ply advances play
    three more, so occurrences three and four are history entries that crl_advance_one wrote (S1 of a child with a
    reply) and the fifth ends the game on the mover's ply (a child without one).  A mirror follows by crl_push_moves."""
    from chessrl_amd import _lib
    from chessrl_amd.engine import LockstepEngine
    cycle = ru.KNIGHT_SHUFFLE[:4]
    net = FakeNet(seed=7, prior_shift=30)
    eng = LockstepEngine(net.to("cuda:0"), n_games=1, max_sims=SIMS, max_plies=32)
    mirror = _lib.Context(1, 1, max_plies=32)
    g = OracleGame()
    for u in cycle:
        assert g.move(u)
    load(eng.ctx, [g])
    load(mirror, [g])
    for u in cycle * 3:
        assert g.get_result() is None
        eng.search(SIMS)
        rc = eng.root_children()
        n = int(rc["nchild"][0])
        assert rc["root_visits"][0] == SIMS + 1
        k = [move_to_uci(m) for m in rc["moves"][0, :n]].index(u)
        bm = eng.advance(np.array([k], np.int32), plies=1)
        assert move_to_uci(bm[0]) == u and mirror.push_moves(bm)[0] == 1
        assert g.move(u)
        same_game(eng.ctx, 0, g)
        same_game(mirror, 0, g)
    assert g.get_result() == 0 and g.repetitions() >= 5 and len(g) == 16
    assert eng.ctx.results()[0] == 0 and mirror.results()[0] == 0
    eng.search(SIMS)
    assert eng.root_children()["nchild"][0] == 0                   # a finished game is not searched
    mirror.close()
    eng.close()


def test_two_ply_advance_is_what_it_was():
    """``advance(chosen)`` and ``advance(chosen, plies=2)`` give what ``ctx.advance`` gives, array for array."""
    from chessrl_amd.engine import LockstepEngine
    roots = one_ply_roots()
    games = [g for _, g, _ in roots]
    G = len(games)
    net = FakeNet(seed=3, prior_shift=30).to("cuda:0")
    outs = []
    for how in ("default", "plies=2", "ctx"):
        eng = LockstepEngine(net, n_games=G, max_sims=SIMS)
        load(eng.ctx, games)
        eng.search(SIMS)
        rc = eng.root_children()
        chosen = np.where(np.arange(G) % 3 == 2, -1, (rc["nchild"] - 1) // (1 + np.arange(G) % 2)).astype(np.int32)
        chosen[6] = 21                                              # f7g7: mate, the game ends on our move
        if how == "default":
            bm, am = eng.advance(chosen)
        elif how == "plies=2":
            bm, am = eng.advance(chosen, plies=2)
        else:
            bm, am = eng.ctx.advance(chosen)
        outs.append([bm, am, eng.ctx.get_positions()] + list(eng.ctx.records()))
        eng.close()
    assert outs[2][0][6] == uci_to_move("f7g7") and outs[2][1][6] == NO_MOVE and outs[2][5][6] == 1
    assert (outs[2][0][[0, 1, 3, 4, 7]] != NO_MOVE).all() and (outs[2][1] != NO_MOVE).any()
    assert (outs[2][0][[2, 5]] == NO_MOVE).all() and (outs[2][1][[2, 5]] == NO_MOVE).all()
    for other in outs[:2]:
        for x, y in zip(other, outs[2]):
            assert x.dtype == y.dtype and np.array_equal(x, y)


def test_one_ply_advance_is_refused_where_it_does_not_apply():
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.opponent import MinimaxPlayer
    net = FakeNet(seed=3, prior_shift=30).to("cuda:0")
    chosen = np.zeros(4, np.int32)
    for kw in (dict(reply=MinimaxPlayer(False, search_depth=1)), dict(max_nodes=3 * SIMS + 1), dict(threads=2)):
        eng = LockstepEngine(net, n_games=4, max_sims=SIMS, **kw)
        eng.reset()
        eng.search(SIMS)
        with pytest.raises(ValueError):
            eng.advance(chosen, plies=1)
        with pytest.raises(ValueError):
            eng.advance(chosen, plies=3)
        _, plies, _ = eng.ctx.records(with_moves=False)
        assert list(plies) == [0] * 4                               # refused before the device was touched
        bm, am = eng.advance(chosen)                                # ... and the two-ply boundary still works
        assert (bm != NO_MOVE).all() and (am != NO_MOVE).all()
        eng.close()


# ---- whole arenas ----------------------------------------------------------------------------------------------------
def assert_same_arena(got, want):
    assert len(got["games"]) == len(want["games"])
    for i, (g, w) in enumerate(zip(got["games"], want["games"])):
        assert g == w, "game %d" % i
    for k in ("played", "a_won", "b_won", "drawn", "unfinished", "score_a", "as_white"):
        assert got[k] == want[k], k


def assert_mirrors_agree(arena):
    for s in arena.sets:
        a, b = s.engines["a"].ctx, s.engines["b"].ctx
        assert np.array_equal(a.get_positions(), b.get_positions())
        for x, y in zip(a.records(), b.records()):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("name", ["random", "fen"])
def test_arena_equals_the_cpu_restatement(name, graph):
    from chessrl_amd.arena import Arena
    a, b = device_nets()
    ar = Arena(a, b, use_graph=graph, **(au.RANDOM_SET if name == "random" else au.FEN_SET))
    try:
        got = ar.play()
        assert_mirrors_agree(ar)
        assert [s.a_white for s in ar.sets] == [True, False]
    finally:
        ar.close()
    assert_same_arena(got, au.reference(name))


def test_arena_function_and_uci_openings():
    """``arena`` itself, with openings given as UCI move lists (the random set's own) beside a FEN"""
    from chessrl_amd.arena import arena
    a, b = device_nets()
    want = au.reference("random")
    openings = [want["games"][0]["opening"], au.FENS[1], want["games"][6]["opening"]]
    got = arena(a, b, games=6, sims=au.RANDOM_SET["sims"], openings=openings, max_plies=au.RANDOM_SET["max_plies"])
    assert got["games"][0:2] == want["games"][0:2] and got["games"][4:6] == want["games"][6:8]
    assert [g["result"] for g in got["games"][2:4]] == [1, 1] and got["games"][2]["opening"] == au.FENS[1]
    assert (got["played"], got["a_won"], got["b_won"], got["unfinished"]) == (6, 1, 1, 4)


def test_a_net_against_itself_plays_each_pair_twice():
    from chessrl_amd.arena import arena
    a, _ = device_nets()
    got = arena(a, a, **au.RANDOM_SET)
    for i in range(0, got["played"], 2):
        w, k = got["games"][i], got["games"][i + 1]
        assert w["moves"] == k["moves"] and w["result"] == k["result"] and w["opening"] == k["opening"]
        assert len(w["moves"]) == au.RANDOM_SET["max_plies"]
    assert got["games"][0] == au.reference("random", same=True, games=2)["games"][0]


def test_exchanging_the_nets_exchanges_the_colours():
    from chessrl_amd.arena import arena
    a, b = device_nets()
    for name, args in (("random", au.RANDOM_SET), ("fen", au.FEN_SET)):
        ab, ba = au.reference(name), arena(b, a, **args)
        for i in range(0, ab["played"], 2):
            for x, y in ((i, i + 1), (i + 1, i)):
                assert ba["games"][x]["moves"] == ab["games"][y]["moves"]
                assert ba["games"][x]["result"] == ab["games"][y]["result"]
                assert ba["games"][x]["a_white"] != ab["games"][y]["a_white"]
        assert (ba["a_won"], ba["b_won"], ba["drawn"], ba["unfinished"]) == \
            (ab["b_won"], ab["a_won"], ab["drawn"], ab["unfinished"])


@pytest.mark.parametrize("name", ["random", "fen"])
def test_greedy_arena_equals_best_move_on_both_sides(name):
    from chessrl_amd.arena import arena
    a, b = device_nets()
    args = dict(au.RANDOM_SET if name == "random" else au.FEN_SET, sims=0)
    got = arena(a, b, **args)
    assert_same_arena(got, au.reference(name, sims=0))
    if name == "random":
        assert all(len(g["moves"]) == args["max_plies"] for g in got["games"])


def test_noise_draws_from_one_generator_per_game():
    from chessrl_amd.arena import arena
    a, b = device_nets()
    kw = dict(games=4, max_plies=8, noise=True)
    want = au.reference("random", **kw)
    got = arena(a, b, **dict(au.RANDOM_SET, **kw))
    assert_same_arena(got, want)
    quiet = au.reference("random")
    assert any(w["moves"] != q["moves"][:8] for w, q in zip(want["games"], quiet["games"]))     # the noise chose


def test_two_real_small_nets_play_legal_moves():
    from chessrl_amd import _lib
    from chessrl_amd.arena import arena
    from chessrl_amd.model import ChessModel
    a, b = ChessModel(blocks=2, filters=32, seed=1), ChessModel(blocks=2, filters=32, seed=2)
    got = arena(a, b, games=4, sims=16, seed=3, opening_plies=4, max_plies=8)
    assert got["played"] == 4 and [g["a_white"] for g in got["games"]] == [True, False, True, False]
    ctx = _lib.Context(4, 1, max_plies=16)
    try:
        table = np.full((4, 12), NO_MOVE, np.uint16)
        counts = np.zeros(4, np.int32)
        for i, g in enumerate(got["games"]):
            ids = [uci_to_move(u) for u in g["opening"] + g["moves"]]
            assert len(g["opening"]) == 4 and (len(g["moves"]) == 8 or g["result"] is not None)
            table[i, :len(ids)] = ids
            counts[i] = len(ids)
        ctx.reset_games()
        assert list(ctx.push_sequences(table, counts)) == list(counts)         # every move was legal where it was played
        results = ctx.results()
        assert [None if r == RESULT_NONE else int(r) for r in results] == [g["result"] for g in got["games"]]
    finally:
        ctx.close()
    assert got["games"][0]["opening"] == got["games"][1]["opening"] != got["games"][2]["opening"]
