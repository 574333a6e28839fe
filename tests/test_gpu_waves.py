"""GPU: ``threads`` > 1 -- virtual-loss waves of simulations per game on the device (csrc/search_wave.hpp).

Bit-exact (visits, f64 value sums by bit pattern, f32 priors, moves, replies, root visits, node counts, wave counts)
against tests/golden/wave_cases.json -- the reference's own select / simulate / backprop driven in the wave schedule --
and against the restatement of tests/wave_util.py, which tests/test_wave_restatement.py pins to that fixture."""
import numpy as np
import pytest

from oracle import mcts_oracle
from oracle.chess_oracle import OracleGame, board_to_array, move_to_uci
from oracle.fakenet import FakeNet
from tests import wave_util as wu

pytestmark = pytest.mark.gpu

NO_MOVE = 0xFFFF
CASES = wu.load_cases()
MODES = ("nep50", "legacy")
META = ["edge0", "nmoves", "nexp", "result", "has_s2", "parent", "parent_edge"]


def hexes(a, kind):
    a = np.asarray(a)
    return [format(int(x), "016x" if kind == "f64" else "08x") for x in a.view(np.uint64 if kind == "f64" else np.uint32)]


def device_stats(rc, i):
    n = int(rc["nchild"][i])
    return {"visits": [int(v) for v in rc["visits"][i, :n]], "values": hexes(rc["values"][i, :n], "f64"),
            "priors": hexes(rc["priors"][i, :n], "f32"), "moves": [move_to_uci(m) for m in rc["moves"][i, :n]],
            "replies": [None if m == NO_MOVE else move_to_uci(m) for m in rc["replies"][i, :n]],
            "root_visits": int(rc["root_visits"][i])}


def load_games(eng, games):
    """Slot i becomes games[i] (OracleGame: a FEN root or the standard position, plus pushed moves)."""
    G = len(games)
    eng.ctx.set_positions(np.stack([board_to_array(g.board_at(len(g))) for g in games]))
    width = max(1, max(len(g) for g in games))
    tbl = np.full((G, width), NO_MOVE, np.uint16)
    cnt = np.zeros(G, np.int32)
    for i, g in enumerate(games):
        cnt[i] = len(g)
        tbl[i, :len(g)] = [g.board.move_stack[k].m for k in range(len(g))]
    assert list(eng.ctx.push_sequences(tbl, cnt)) == list(cnt)


def mode_cases(mode):
    return [c for c in CASES if c["mode"] == mode]


def batch_of(cases):
    """The seven fixture positions + the first once more: one lockstep batch of G = 8."""
    return cases + cases[:1]


def nets_of(cases):
    """{(net seed, shift, tie): [case indices]}.  A lockstep batch has one evaluator, so the whole batch of all
    positions runs once per FakeNet of the fixture and the slots whose case was made with that net are compared:
    games with and without short waves fall out of step in every one of those batches."""
    out = {}
    for i, c in enumerate(cases):
        out.setdefault((c["net_seed"], c["prior_shift"], c["tie"]), []).append(i)
    return out


def expected_short(waves, T, n):
    done = short = 0
    for w in waves:
        short += w < min(T, n - done)
        done += w
    return int(short)


def all_trees(eng):
    """Every slot's tree: the node records field by field (the hashes, boards and the reply of every node that has an
    S2; the record's padding is never written), the edge records whole, the counters."""
    out = []
    for slot in range(eng.G):
        nodes, edges, info = eng.ctx.fetch_tree(slot)
        rest = np.ascontiguousarray(nodes["rest"]).view(np.uint8).reshape(len(nodes), 160)
        full = nodes["has_s2"] == 1
        full[:1] = False                                               # the root holds S2 only
        out.append((tuple(nodes[k].tobytes() for k in META), rest[full][:, :146].tobytes(), rest[:1, 8:16].tobytes(),
                    rest[:1, 80:144].tobytes(), edges.tobytes(), info))
    return out


@pytest.mark.parametrize("T", wu.THREADS)
@pytest.mark.parametrize("mode", MODES)
def test_engine_reproduces_the_reference_driven_in_waves(mode, T):
    from chessrl_amd.engine import LockstepEngine, compute_policy
    cases = mode_cases(mode)
    games = [wu.case_game(c) for c in batch_of(cases)]
    n = cases[0]["sims"]
    for (seed, shift, tie), mine in nets_of(cases).items():
        eng = LockstepEngine(FakeNet(seed=seed, prior_shift=shift, tie=tie).to("cuda:0"), n_games=len(games), max_sims=n,
                             numpy_promotion=mode, threads=T)
        assert eng.pol_s1.shape[0] == len(games) * T
        load_games(eng, games)
        eng.search(n)
        assert -(-n // T) <= eng.wave_steps <= n
        rc = eng.root_children()
        ws = eng.ctx.wave_stats()
        _, plies, _ = eng.ctx.records(with_moves=False)
        for i in mine:
            c = cases[i]
            run = [r for r in c["runs"] if r["threads"] == T][0]
            got = device_stats(rc, i)
            for k in got:
                assert got[k] == run[k], (c["name"], mode, T, k)
            assert eng.ctx.fetch_tree(i)[2]["n_nodes"] == run["n_nodes"]
            assert (int(ws["waves"][i]), int(ws["leaves"][i])) == (len(run["waves"]), n), (c["name"], T)
            assert int(ws["short_waves"][i]) == expected_short(run["waves"], T, n) == run["events"]["short_waves"]
            pol = compute_policy(got["visits"], got["root_visits"], plies[i], noise=False)
            assert hexes(pol, "f64") == run["policy"] and int(np.argmax(pol)) == run["chosen"]
        assert eng.wave_steps == int(ws["waves"].max())                 # the batch runs until its slowest game is done
        assert eng.ctx.counters()["sims"] == len(games) * n
        eng.close()


def drive_waves_by_hand(eng, n, T):
    eng.search_begin()
    eng.ctx.wave_begin(n)
    steps = 0
    while eng.ctx.wave_remaining() > 0:
        eng.ctx.wave_select(eng.pol_s2.data_ptr(), eng.val_s2.data_ptr(), eng.planes_s1.data_ptr())
        eng.phase_tower_s1()
        eng.ctx.wave_reply(eng.pol_s1.data_ptr(), eng.planes_s2.data_ptr())
        eng.phase_tower_s2()
        steps += 1
    eng.ctx.wave_backup(eng.pol_s2.data_ptr(), eng.val_s2.data_ptr())
    return steps


@pytest.mark.parametrize("mode", MODES)
def test_one_thread_through_the_wave_kernels_is_todays_tree(mode):
    """crl_wave_* with threads = 1 against LockstepEngine.search: the whole tree, record by record."""
    from chessrl_amd.engine import LockstepEngine
    cases = [c for c in mode_cases(mode) if c["net_seed"] == 13]
    games = [wu.case_game(c) for c in cases]
    net = FakeNet(seed=13, prior_shift=30).to("cuda:0")
    n = 80
    trees = []
    for waves in (False, True):
        eng = LockstepEngine(net, n_games=len(games), max_sims=n, numpy_promotion=mode, use_graph=False)
        load_games(eng, games)
        if waves:
            eng.ctx.wave_config(1)
            assert drive_waves_by_hand(eng, n, 1) == n
            ws = eng.ctx.wave_stats()
            assert list(ws["waves"]) == [n] * len(games) and not ws["short_waves"].any()
        else:
            eng.search(n)
        trees.append((all_trees(eng), eng.root_children(), eng.ctx.counters()))
        eng.close()
    (ta, ra, ca), (tb, rb, cb) = trees
    for slot, (a, b) in enumerate(zip(ta, tb)):
        assert a[-1] == b[-1] and a[-1]["n_nodes"] > 1, slot
        assert a == b, slot
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k
    assert ca == cb


def test_graph_replay_equals_eager_and_two_runs_are_identical():
    from chessrl_amd.engine import LockstepEngine
    cases = [c for c in mode_cases("nep50") if c["net_seed"] == 13]
    games = [wu.case_game(c) for c in cases]
    net = FakeNet(seed=13, prior_shift=30).to("cuda:0")
    n, T = 100, 6
    runs = []
    for graph in (True, True, False):
        eng = LockstepEngine(net, n_games=len(games), max_sims=n, numpy_promotion="nep50", use_graph=graph, threads=T)
        load_games(eng, games)
        eng.search(n)
        runs.append((all_trees(eng), eng.wave_steps, {k: v.tolist() for k, v in eng.ctx.wave_stats().items()}))
        eng.search(n)                                                   # a second search in the same engine: the same again
        assert all_trees(eng) == runs[-1][0]
        eng.close()
    assert runs[0] == runs[1] == runs[2]
    fixture = {c["name"]: [r for r in c["runs"] if r["threads"] == T][0] for c in cases}
    assert runs[0][2]["waves"] == [len(fixture[c["name"]]["waves"]) for c in cases]


@pytest.mark.parametrize("n,T", [(5, 16), (37, 6), (1, 64), (64, 64), (101, 2)])
def test_the_budget_is_exact_whatever_the_thread_count(n, T):
    from chessrl_amd.engine import LockstepEngine
    cases = [c for c in mode_cases("nep50") if c["net_seed"] == 13]
    games = [wu.case_game(c) for c in cases]
    net = FakeNet(seed=13, prior_shift=30)
    eng = LockstepEngine(net.to("cuda:0"), n_games=len(games), max_sims=101, numpy_promotion="nep50", threads=T)
    load_games(eng, games)
    eng.search(n)
    rc = eng.root_children()
    ws = eng.ctx.wave_stats()
    assert list(rc["root_visits"]) == [n + 1] * len(games) and list(ws["leaves"]) == [n] * len(games)
    for i, c in enumerate(cases):
        _, st = wu.wave_search(games[i], mcts_oracle.OracleAgent(net), n, T, "nep50")
        got = device_stats(rc, i)
        for k in got:
            assert got[k] == st[k], (c["name"], k)
        assert int(ws["waves"][i]) == len(st["waves"])
    eng.close()


# ---- the drop-in surface ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_dropin_tree_with_virtual_loss_equals_the_fixture(mode):
    """SelfPlayTree(game, threads=6, virtual_loss=True).search_move: (bm, am) and the children of the fixture; the
    same call without virtual_loss still gives today's tree."""
    from chessrl_amd.agent import Agent
    from chessrl_amd.game import Game
    from chessrl_amd.mctree import SelfPlayTree
    T = 6
    for c in mode_cases(mode):
        run = [r for r in c["runs"] if r["threads"] == T][0]
        agent = Agent(True, model=wu.case_net(c).to("cuda:0"), numpy_promotion=mode)
        g = Game(board=c["fen"]) if c["fen"] else Game()
        for u in c["prefix_moves"]:
            assert g.move(u)
        tree = SelfPlayTree(g, threads=T, virtual_loss=True)
        pair = tree.search_move(agent, max_iters=c["sims"], noise=False, ai_move=True)
        assert pair == (run["bm"], run["am"]), (c["name"], mode)
        kids = tree.root.children
        assert tree.root.visits == run["root_visits"] and [k.visits for k in kids] == run["visits"]
        assert hexes(np.array([k.value for k in kids], np.float64), "f64") == run["values"]
        assert hexes(np.array([k.prior for k in kids], np.float32), "f32") == run["priors"]
        assert [(k.move, k.reply) for k in kids] == list(zip(run["moves"], run["replies"]))
        assert agent.engine_for(c["sims"], threads=T).threads == T and agent.engine_for(c["sims"]).threads == 1
        if c["name"] in ("castling_both_sides", "rounding_ties"):
            plain = SelfPlayTree(g, threads=T)                          # threads without virtual_loss: accepted, one worker
            plain.search_move(agent, max_iters=c["sims"], noise=False, ai_move=True)
            seq = mcts_oracle.search(wu.case_game(c), mcts_oracle.OracleAgent(wu.case_net(c), widen_priors=(mode == "legacy")),
                                     c["sims"], noise=False, mode=mode)
            assert [k.visits for k in plain.root.children] == seq.visits != run["visits"]
            assert hexes(np.array([k.value for k in plain.root.children], np.float64), "f64") == [wu.f64hex(v) for v in seq.values]
            with pytest.raises(ValueError, match="virtual_loss"):
                SelfPlayTree(tree.root.children[0], threads=T, virtual_loss=True)
        g.free()


def test_a_short_whole_game_of_the_runner_with_six_threads_matches_the_restatement():
    from chessrl_amd.selfplay import SelfPlayRunner, game_color
    net = FakeNet(seed=5, prior_shift=29)
    S, T, moves, seed, G = 40, 6, 8, 4, 4
    run = SelfPlayRunner(net.to("cuda:0"), n_parallel=G, sims=S, seed=seed, noise=False, total_games=G, max_plies=512, threads=T)
    assert run.engine.threads == T
    run.run(max_moves=moves)
    rec_moves, plies, _ = run.engine.ctx.records()
    colours = [game_color(seed, int(run.game_id[slot])) for slot in range(G)]
    assert set(colours) == {True, False}
    by_colour = {}                                                      # (noise off: games of one colour are one game)
    for slot in range(G):
        g = by_colour.get(colours[slot])
        if g is None:
            g = by_colour[colours[slot]] = wu.play_game_waves(mcts_oracle.OracleAgent(net), S, T, moves=moves,
                                                               mode=run.engine.numpy_promotion, player_color=colours[slot])
        assert list(rec_moves[slot, :plies[slot]]) == [g.board.move_stack[i].m for i in range(len(g))], slot
    seq = mcts_oracle.play_game(mcts_oracle.OracleAgent(net), max_iters=S, noise=False, mode=run.engine.numpy_promotion,
                                player_color=True, max_moves=moves)
    assert [m.m for m in seq.board.move_stack] != [m.m for m in by_colour[True].board.move_stack]   # not the one-worker game
    with pytest.raises(ValueError, match="threads > 1"):
        run.step()
    run.close()


def test_refusals_on_a_live_engine():
    from chessrl_amd.engine import LockstepEngine, StampRing
    net = FakeNet(seed=3, prior_shift=30).to("cuda:0")
    eng = LockstepEngine(net, n_games=4, max_sims=20, threads=6)
    eng.reset()
    with pytest.raises(ValueError, match="keep_root"):
        eng.search(10, keep_root=True)
    with pytest.raises(ValueError, match="reroot"):
        eng.reroot(np.zeros(4, np.int32), 10)
    with pytest.raises(ValueError, match="set_stamps"):
        eng.set_stamps(StampRing(64, eng.dev))
    with pytest.raises(ValueError, match="max_sims"):
        eng.search(21)
    eng.search(20)
    assert list(eng.root_children()["root_visits"]) == [21] * 4
    eng.close()
    plain = LockstepEngine(net, n_games=4, max_sims=20)
    plain.reset()
    from chessrl_amd import _lib
    with pytest.raises(_lib.HipLibraryError, match="crl_wave_config first"):
        plain.ctx.wave_begin(10)
    with pytest.raises(_lib.HipLibraryError):
        plain.ctx.wave_config(65)
    plain.close()


def test_real_tower_waves_are_deterministic_and_structurally_sound():
    """A small ChessModel (2 x 64) at T = 6, G = 4: graph replay, eager launches and a second run give the same trees
    record by record; every tree passes the structural checks of the one-leaf path (ids in creation order, edge runs
    in thread order, descent hints, children's visits summing to visits - 1 between waves); T = 1 through the wave
    kernels equals today's search on full policy vectors."""
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.model import ChessModel
    from tests.test_gpu_reroot import check_tree
    from tests.test_gpu_search import move_ids, random_prefix_games
    model = ChessModel(blocks=2, filters=64, seed=3)
    games = random_prefix_games(4, 40, seed=31)
    n, T = 90, 6
    runs = []
    for graph in (True, True, False):
        eng = LockstepEngine(model, n_games=4, max_sims=n, use_graph=graph, threads=T)
        assert not eng.legal_priors and eng.pol_s2.shape == (4 * T, 1968)
        eng.load_moves([move_ids(g) for g in games])
        eng.search(n)
        for slot in range(4):
            _, _, info = check_tree(eng.ctx, slot, fresh_root=True)
            assert info["root_visits"] == n + 1
        runs.append((all_trees(eng), {k: v.tolist() for k, v in eng.ctx.wave_stats().items()}))
        eng.close()
    assert runs[0] == runs[1] == runs[2]
    assert all(w < n for w in runs[0][1]["waves"])                      # waves did widen the steps
    trees = []
    for waves in (False, True):
        eng = LockstepEngine(model, n_games=4, max_sims=n, use_graph=False, legal_priors=False)
        eng.load_moves([move_ids(g) for g in games])
        if waves:
            eng.ctx.wave_config(1)
            assert drive_waves_by_hand(eng, n, 1) == n
        else:
            eng.search(n)
        trees.append(all_trees(eng))
        eng.close()
    assert trees[0] == trees[1]
    assert trees[0] != runs[0][0]


def test_real_heads_at_six_threads_equal_the_restatement_fed_the_fp32_oracle_tower():
    """A 2 x 64 ChessModel (the fused HIP tower in ``f16x3``, its fp32-grade arithmetic: the mode held to tree equality
    wherever ``auto`` would pick ``hybrid``) at T = 6, G = 4 against tests/wave_util.py's restatement whose agent is
    the fp32 oracle tower (oracle/tower_oracle.py) on the same weights, evaluated position by position on the CPU.
    The weights are calibrated on real positions (peaked policies, values spread over (-1, 1)), so that an output
    error is not hidden behind a constant tower.
    Exact: the tree -- visits, moves, replies, root visits, node count, the list of wave sizes (so every row
    g * T + t carried the policy and value of ITS leaf).  Within the tower's bar: f16x3 is held to 1e-4 of the fp32
    oracle per output (__graft_entry__.smoke, tests/test_gpu_search.py), a child's value sum adds ``visits`` such
    values, so |sum - oracle sum| <= visits * 1e-4; priors within 1e-4."""
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.model import ChessModel
    from oracle import encoder_oracle, tower_oracle
    from tests.test_gpu_search import move_ids, random_prefix_games
    sample = random_prefix_games(24, 60, seed=17)
    w = tower_oracle.calibrated_weights(2, 64, np.stack([encoder_oracle.get_game_state(g) for g in sample]), seed=5)
    model = ChessModel(weights=w, precision="f16x3")
    games = random_prefix_games(4, 36, seed=33)
    n, T, G = 60, 6, 4
    eng = LockstepEngine(model, n_games=G, max_sims=n, threads=T)
    eng.load_moves([move_ids(g) for g in games])
    eng.search(n)
    rc = eng.root_children()
    ws = eng.ctx.wave_stats()
    agent = mcts_oracle.OracleAgent(tower_oracle.TowerNet(w), widen_priors=(eng.numpy_promotion == "legacy"))
    worst_v = worst_p = 0.0
    for i, g in enumerate(games):
        _, st = wu.wave_search(g, agent, n, T, eng.numpy_promotion)
        got = device_stats(rc, i)
        nc = int(rc["nchild"][i])
        dv = np.abs(rc["values"][i, :nc] - np.array([int(h, 16) for h in st["values"]], np.uint64).view(np.float64))
        dp = np.abs(rc["priors"][i, :nc].astype(np.float64) -
                    np.array([int(h, 16) for h in st["priors"]], np.uint32).view(np.float32).astype(np.float64))
        worst_v = max(worst_v, float((dv / np.maximum(rc["visits"][i, :nc], 1)).max()))
        worst_p = max(worst_p, float(dp.max()))
        print("slot %d: waves %s (oracle %s), nodes %d (oracle %d), max |dvalue|/visits %.3e, max |dprior| %.3e, visits equal %s"
              % (i, int(ws["waves"][i]), len(st["waves"]), eng.ctx.fetch_tree(i)[2]["n_nodes"], st["n_nodes"],
                 float((dv / np.maximum(rc["visits"][i, :nc], 1)).max()), float(dp.max()), got["visits"] == st["visits"]))
        for k in ("visits", "moves", "replies", "root_visits"):
            assert got[k] == st[k], (i, k)
        assert eng.ctx.fetch_tree(i)[2]["n_nodes"] == st["n_nodes"]
        assert int(ws["waves"][i]) == len(st["waves"]) and int(ws["leaves"][i]) == n
        assert (dv <= rc["visits"][i, :nc] * 1e-4).all(), (i, dv)
        assert (dp <= 1e-4).all(), (i, dp)
    print("real heads: worst |dvalue| / visits %.3e, worst |dprior| %.3e" % (worst_v, worst_p))
    eng.close()


def test_noisy_runner_games_with_six_threads_match_the_restatement():
    """Dirichlet noise on: the draws are made from the per-game streams while the blind wave steps are enqueued."""
    from chessrl_amd.selfplay import SelfPlayRunner, game_color
    net = FakeNet(seed=5, prior_shift=29)
    S, T, moves, seed = 40, 6, 8, 7
    run = SelfPlayRunner(net.to("cuda:0"), n_parallel=2, sims=S, seed=seed, noise=True, total_games=2, max_plies=512, threads=T)
    run.run(max_moves=moves)
    rec_moves, plies, _ = run.engine.ctx.records()
    for slot in range(2):
        gid = int(run.game_id[slot])
        g = wu.play_game_waves(mcts_oracle.OracleAgent(net), S, T, moves=moves, mode=run.engine.numpy_promotion,
                               player_color=game_color(seed, gid), noise=True, rng=np.random.default_rng([seed, gid]))
        assert list(rec_moves[slot, :plies[slot]]) == [g.board.move_stack[i].m for i in range(len(g))], gid
    run.close()


def test_a_node_of_a_wave_tree_cannot_be_continued_and_says_why():
    from chessrl_amd.agent import Agent
    from chessrl_amd.game import Game
    from chessrl_amd.mctree import SelfPlayTree
    agent = Agent(True, model=FakeNet(seed=3, prior_shift=30).to("cuda:0"))
    g = Game()
    tree = SelfPlayTree(g, threads=6, virtual_loss=True)
    tree.search_move(agent, max_iters=30, noise=False)
    with pytest.raises(ValueError, match="fresh tree"):
        SelfPlayTree(tree.root.children[0], threads=6).search_move(agent, max_iters=10, noise=False)
    g.free()
