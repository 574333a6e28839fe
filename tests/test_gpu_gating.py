"""GPU: the device move boundary (crl_advance_one_argmax, crl_push_moves_dev), the arena on it, and the gate.

The weight sets are FakeNets unless stated otherwise, so the device's games are compared with the CPU restatement
(tests/arena_util.py) move for move; tests/test_gating_cpu.py holds the choice rule and the early verdict to numpy
and to exhaustion.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle.chess_oracle import OracleGame, board_from_fen, board_to_array
from oracle.fakenet import FakeNet
from tests import arena_util as au
from tests.util import MAX_MOVES_FEN

pytestmark = pytest.mark.gpu

NO_MOVE, RESULT_NONE = 0xFFFF, 2


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


def state_of(ctx):
    return [ctx.get_positions().copy()] + [x.copy() for x in ctx.records()]


def u16(t):
    return t.cpu().numpy().view(np.uint16)


def assert_same_arena(got, want):
    assert len(got["games"]) == len(want["games"])
    for i, (g, w) in enumerate(zip(got["games"], want["games"])):
        assert g == w, "game %d" % i
    for k in ("played", "a_won", "b_won", "drawn", "unfinished", "score_a", "as_white"):
        assert got[k] == want[k], k


# ---- the device-boundary arena ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("name", ["random", "fen"])
def test_device_boundary_arena_equals_the_cpu_restatement(name, graph):
    from chessrl_amd.arena import Arena
    a, b = device_nets()
    ar = Arena(a, b, use_graph=graph, boundary="device", **(au.RANDOM_SET if name == "random" else au.FEN_SET))
    try:
        got = ar.play()
        for s in ar.sets:                                            # the mirrors agree
            x, y = s.engines["a"].ctx, s.engines["b"].ctx
            assert np.array_equal(x.get_positions(), y.get_positions())
            for p, q in zip(x.records(), y.records()):
                assert np.array_equal(p, q)
    finally:
        ar.close()
    assert_same_arena(got, au.reference(name))


# ---- advance_argmax --------------------------------------------------------------------------------------------------
def golden_prefix(golden_dir, plies, which=0):
    gm = json.load(open(os.path.join(golden_dir, "selfplay_games.json")))["games"][which]
    g = OracleGame()
    for u in gm["moves"][:plies]:
        assert g.move(u)
    return g


@pytest.mark.parametrize("sims", [300, 100])
def test_advance_argmax_equals_choose_children_and_the_one_ply_advance(golden_dir, sims):
    """Slots: the 218-move root (300 simulations expand every child and leave almost all tied at one visit; 100 leave
    ``nexp < nmoves``), a recorded game at ply 30 (tau is not 1), the start position; then three that must not move: a
    slot whose side is not ``mover_white``, a slot at its ``ply_limit``, a finished game."""
    import torch
    from chessrl_amd.engine import LockstepEngine, choose_children
    games = [OracleGame(board=board_from_fen(MAX_MOVES_FEN)), golden_prefix(golden_dir, 30), OracleGame(),
             golden_prefix(golden_dir, 31), golden_prefix(golden_dir, 12, which=1),
             OracleGame(board=board_from_fen(au.FENS[2]))]
    G = len(games)
    assert [g.turn for g in games[:5]] == [True, True, True, False, True] and games[5].get_result() == 0
    movers, still = [0, 1, 2], [3, 4, 5]
    limit = np.array([4096, 4096, 4096, 4096, 12, 4096], np.int32)
    net = FakeNet(seed=3, prior_shift=30).to("cuda:0")
    host = LockstepEngine(net, n_games=G, max_sims=sims)
    dev = LockstepEngine(net, n_games=G, max_sims=sims)
    try:
        for eng in (host, dev):
            load(eng.ctx, games)
            eng.search(sims)
        rc, rc_dev = host.root_children(), dev.root_children()
        for k in ("nchild", "visits", "moves", "root_visits"):
            assert np.array_equal(rc[k], rc_dev[k]), k
        n0 = int(rc["nchild"][0])
        row = rc["visits"][0, :n0]
        if sims == 300:
            assert n0 == 218 and (row == 1).sum() >= 218 - (sims - 218)      # almost all tied at one visit
        else:
            assert n0 == 100 < 218
        assert rc["nchild"][5] == 0 and (rc["nchild"][:5] > 0).all()
        _, plies, results = host.ctx.records(with_moves=False)
        assert list(plies) == [0, 30, 0, 31, 12, 0]
        # the host boundary: the arena's mask, choose_children, the one-ply advance
        mask = (results == RESULT_NONE) & (plies < limit) & np.array([g.turn for g in games])
        assert list(np.nonzero(mask)[0]) == movers
        want_chosen = choose_children(rc["visits"], np.where(mask, rc["nchild"], 0), rc["root_visits"], plies,
                                      noise=False)
        want_bm = host.advance(want_chosen, plies=1)
        # the device boundary
        before = state_of(dev.ctx)
        bm, chosen = dev.advance_argmax(True, torch.from_numpy(limit).to("cuda:0"))
        assert bm.is_cuda and chosen.is_cuda and chosen.dtype == torch.int32
        bm, chosen = u16(bm), chosen.cpu().numpy()
        assert np.array_equal(chosen, want_chosen) and np.array_equal(bm, want_bm)
        for k in movers:
            n = int(rc["nchild"][k])
            assert chosen[k] == int(np.argmax(rc["visits"][k, :n])) and bm[k] == rc["moves"][k, chosen[k]]
        after = state_of(dev.ctx)
        for x, y in zip(after, state_of(host.ctx)):                 # positions, records, plies, results
            assert np.array_equal(x, y)
        assert list(after[2]) == [1, 31, 1, 31, 12, 0]
        for k in still:                                              # untouched, bit for bit
            assert bm[k] == NO_MOVE and chosen[k] == -1
            for x, y in zip(before, after):
                assert np.array_equal(x[k], y[k])
        for k in (3, 4):                                             # ... and their trees are still there
            assert dev.ctx.fetch_tree(k)[2]["root_visits"] == sims + 1
        for k in movers:
            assert dev.ctx.fetch_tree(k)[2]["n_nodes"] == 0         # consumed, as by advance(plies=1)
        # black's turn: slot 3 moves now, and the numpy limit is taken as well
        bm2, chosen2 = dev.advance_argmax(False, limit)
        bm2, chosen2 = u16(bm2), chosen2.cpu().numpy()
        n = int(rc["nchild"][3])
        assert list(np.nonzero(chosen2 >= 0)[0]) == [3] and chosen2[3] == int(np.argmax(rc["visits"][3, :n]))
        assert bm2[3] == rc["moves"][3, chosen2[3]] and dev.ctx.records(with_moves=False)[1][3] == 32
    finally:
        host.close()
        dev.close()


def test_advance_argmax_is_refused_where_the_one_ply_advance_is():
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.opponent import MinimaxPlayer
    net = FakeNet(seed=3, prior_shift=30).to("cuda:0")
    limit = np.full(4, 64, np.int32)
    for kw in (dict(reply=MinimaxPlayer(False, search_depth=1)), dict(max_nodes=3 * 8 + 1), dict(threads=2)):
        eng = LockstepEngine(net, n_games=4, max_sims=8, **kw)
        try:
            eng.reset()
            eng.search(8)
            with pytest.raises(ValueError) as by_argmax:
                eng.advance_argmax(True, limit)
            with pytest.raises(ValueError) as by_advance:
                eng.advance(np.zeros(4, np.int32), plies=1)
            assert str(by_argmax.value) == str(by_advance.value)
            assert list(eng.ctx.records(with_moves=False)[1]) == [0] * 4
        finally:
            eng.close()


# ---- push_moves_dev --------------------------------------------------------------------------------------------------
def test_push_moves_dev_leaves_what_push_moves_leaves():
    import torch
    from chessrl_amd import _lib
    from oracle.chess_oracle import uci_to_move
    games = [OracleGame(), OracleGame(board=board_from_fen(au.FENS[0])), OracleGame(),
             OracleGame(board=board_from_fen(au.FENS[5]))]
    moves = np.array([uci_to_move("e2e4"), NO_MOVE, uci_to_move("g1f3"), uci_to_move("h1h2")], np.uint16)
    stream = torch.cuda.current_stream().cuda_stream
    host, dev = _lib.Context(4, 1, max_plies=8), _lib.Context(4, 1, max_plies=8)
    try:
        for ctx in (host, dev):
            ctx.set_stream(stream)
            load(ctx, games)
        before = state_of(dev)
        ok = host.push_moves(moves)
        assert list(ok) == [1, 0, 1, 1]
        dev_moves = torch.from_numpy(moves.view(np.int16)).to("cuda:0")
        dev_ok = torch.full((4,), 7, dtype=torch.uint8, device="cuda:0")
        dev.push_moves_dev(dev_moves, dev_ok)
        dev.sync()
        assert list(dev_ok.cpu().numpy()) == list(ok)
        for x, y in zip(state_of(host), state_of(dev)):
            assert np.array_equal(x, y)
        for x, y in zip(before, state_of(dev)):                     # the NO_MOVE slot: untouched
            assert np.array_equal(x[1], y[1])
        # without dev_ok; a second ply
        again = np.array([uci_to_move("e7e5"), NO_MOVE, NO_MOVE, NO_MOVE], np.uint16)
        host.push_moves(again)
        dev.push_moves_dev(torch.from_numpy(again.view(np.int16)).to("cuda:0"))
        dev.sync()
        for x, y in zip(state_of(host), state_of(dev)):
            assert np.array_equal(x, y)
        # a refused move is a device error at the next synchronising call
        dev.push_moves_dev(torch.from_numpy(np.array([uci_to_move("a1a5")] + [NO_MOVE] * 3, np.uint16)
                                            .view(np.int16)).to("cuda:0"))
        with pytest.raises(_lib.HipLibraryError):
            dev.sync()
    finally:
        host.close()
        dev.close()


# ---- the gate --------------------------------------------------------------------------------------------------------
def test_a_net_against_itself_scores_one_half():
    from chessrl_amd.gating import gate
    a, _ = device_nets()
    out = gate(a, a, threshold=0.55, **au.FEN_SET)
    assert out["score"] == 0.5 and out["half_points"] == out["played"] == 12 and out["accepted"] is False
    assert gate(a, a, threshold=0.5, **au.FEN_SET)["accepted"] is True
    again = gate(a, a, threshold=0.5, boundary="device", **au.RANDOM_SET)
    assert again["score"] == 0.5 and again["accepted"] is True and again["unfinished"] == 8


def test_exchanging_candidate_and_incumbent_exchanges_the_half_points():
    from chessrl_amd.gating import gate, gate_half_points
    a, b = device_nets()
    for name, args in (("fen", au.FEN_SET), ("random", au.RANDOM_SET)):
        ab = gate(a, b, early_stop=False, boundary="device", **args)
        ba = gate(b, a, early_stop=False, boundary="device", **args)
        assert ab["half_points"] + ba["half_points"] == 2 * args["games"]
        want = au.reference(name)
        assert_same_arena(ab, want)
        assert ab["half_points"] == gate_half_points(want) and ab["stopped_at_ply"] is None
        assert (ab["low"], ab["high"]) == (ab["half_points"] - ab["unfinished"], ab["half_points"] + ab["unfinished"])


def results_after(games, ply):
    """Per-game results for A after ``ply`` plies of the CPU restatement's games."""
    return [(g["result"] if g["a_white"] else -g["result"])
            if g["result"] is not None and len(g["moves"]) <= ply else None for g in games]


@pytest.mark.parametrize("boundary", ["device", "host"])
def test_early_stop_keeps_the_verdict_and_stops_where_the_cpu_says(boundary):
    from chessrl_amd.gating import decided, gate, verdict
    threshold = 0.7
    want = au.reference("fen")
    # the set, chosen on the CPU: the verdict is decided before the last game ends
    last = max(len(g["moves"]) for g in want["games"])
    first = next(p for p in range(1, last + 1) if decided(results_after(want["games"], p), threshold) is not None)
    assert first < last and any(r is None for r in results_after(want["games"], first))
    a, b = device_nets()
    full = gate(a, b, threshold=threshold, early_stop=False, boundary=boundary, **au.FEN_SET)
    early = gate(a, b, threshold=threshold, early_stop=True, boundary=boundary, **au.FEN_SET)
    assert full["stopped_at_ply"] is None and full["plies_played"] == last
    assert early["stopped_at_ply"] == first == early["plies_played"]
    assert early["accepted"] is full["accepted"] is decided(results_after(want["games"], first), threshold)
    assert full["accepted"] is verdict(full["half_points"], 12, threshold)
    assert early["unfinished"] == sum(r is None for r in results_after(want["games"], first)) > 0
    assert early["low"] <= full["half_points"] <= early["high"]
    for g, w in zip(early["games"], want["games"]):
        assert g["moves"] == w["moves"][:first]


# ---- a gated round on the device -------------------------------------------------------------------------------------
def digest(weights):
    return hashlib.sha1(b"".join(np.ascontiguousarray(weights[k]).tobytes() for k in sorted(weights))).hexdigest()


@pytest.mark.parametrize("threshold,accepted", [(0.0, True), (1.0, False)])
def test_gated_round_on_the_device(golden_dir, tmp_path, threshold, accepted):
    """The real ``train_weights`` and ``gate`` around a 2x32 net: at threshold 0 every candidate passes, at 1 only a
    clean sweep would -- and a game cut off is a draw."""
    from chessrl_amd import selfplay as sp
    from chessrl_amd.model import ChessModel
    from chessrl_amd.records import GameRecord
    from oracle.chess_oracle import uci_to_move
    gm = json.load(open(os.path.join(golden_dir, "selfplay_games.json")))["games"][2]      # 73 plies, white won
    records = [GameRecord(0, [uci_to_move(u) for u in gm["moves"]], gm["result"], gm["player_color"])]
    model = ChessModel(blocks=2, filters=32, seed=1)
    path = str(tmp_path / "model-0.npz")
    model.save_weights(path)
    before_file, before = open(path, "rb").read(), digest(model.weights)
    settings = dict(round=0, model_path=path, model_dir=str(tmp_path), games=4, sims=8, threshold=threshold, seed=5,
                    opening_plies=2, max_plies=6, device="cuda:0", on_accept=model.load_dict)
    weights, carried, entry = sp.gated_round(model.weights, records, [], settings,
                                             gate_fn=sp.device_gate(settings, incumbent_model=model))
    line = [json.loads(x) for x in open(os.path.join(str(tmp_path), sp.GATE_LOG))]
    assert line == [entry] and set(entry) == set(sp.GATE_LOG_KEYS)
    assert entry["accepted"] is accepted and entry["candidate"] is True and entry["trained_on"] == 1
    assert entry["played"] == 4 and entry["games"] == 4 and entry["sims"] == 8 and entry["seed"] == 5
    assert entry["a_won"] + entry["b_won"] + entry["drawn"] + entry["unfinished"] == 4
    assert entry["precision_candidate"] is not None and entry["precision_incumbent"] == model.precision
    if accepted:
        assert digest(weights) != before and digest(model.weights) == digest(weights) and carried == []
        on_file = dict(np.load(path))
        assert digest(on_file) == digest(weights)
    else:
        assert digest(weights) == before == digest(model.weights) and carried == [records]
        assert open(path, "rb").read() == before_file
