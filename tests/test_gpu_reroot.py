"""GPU: Tree(Node) on the device -- crl_reroot keeps the chosen child's subtree across the move boundary.

Bit-exact (visits, f64 value sums by bit pattern, f32 priors, moves, replies, root visits) against
tests/golden/reroot_cases.json -- the reference's own ``SelfPlayTree(Node)`` -- and against the continuation
oracle of tests/reroot_util.py, which tests/test_reroot_oracle.py pins to that fixture.  The fixture's nets are
FakeNet (an exact integer function of the planes), which hands back full policy vectors: CRL_POLICY_FULL is
what runs against the fixture; CRL_POLICY_LEGAL and CRL_POLICY_LEGAL_RAW are held to the same trees as
CRL_POLICY_FULL over two re-rootings with the real heads."""
import numpy as np
import pytest

from oracle import mcts_oracle
from oracle.chess_oracle import OracleGame, board_from_fen, board_to_array, move_to_uci, uci_to_move
from oracle.fakenet import FakeNet
from tests import reroot_util as ru

pytestmark = pytest.mark.gpu

NO_MOVE, RESULT_NONE = 0xFFFF, 2
CASES = ru.load_cases()
HINT_FULL = 1 << 31


def hexes(a, kind):
    a = np.asarray(a)
    return [format(int(x), "016x" if kind == "f64" else "08x") for x in a.view(np.uint64 if kind == "f64" else np.uint32)]


def device_stats(rc, i):
    n = int(rc["nchild"][i])
    return {"visits": [int(v) for v in rc["visits"][i, :n]], "values": hexes(rc["values"][i, :n], "f64"),
            "priors": hexes(rc["priors"][i, :n], "f32"), "moves": [move_to_uci(m) for m in rc["moves"][i, :n]],
            "replies": [None if m == NO_MOVE else move_to_uci(m) for m in rc["replies"][i, :n]],
            "root_visits": int(rc["root_visits"][i])}


def check_tree(ctx, slot, fresh_root=False):
    """Structure of one slot's tree as the kernels keep it; returns (nodes, edges, info)."""
    nodes, edges, info = ctx.fetch_tree(slot)
    n = info["n_nodes"]
    assert n >= 1 and len(nodes) == n
    par, pe = nodes["parent"].astype(np.int64), nodes["parent_edge"].astype(np.int64)
    assert par[0] == 0 and pe[0] == -1
    assert (par[1:] < np.arange(1, n)).all()                                   # ids in creation order, dense 0 .. n-1
    owned = np.where(nodes["has_s2"] == 1, nodes["nmoves"], 0).astype(np.int64)
    start = np.cumsum(owned) - owned
    has = nodes["has_s2"] == 1
    assert (nodes["edge0"][has] == start[has]).all() and (nodes["edge0"][~has] == 0).all()
    assert info["edge_top"] == int(owned.sum()) == len(edges)                  # edge_top = sum of owned edges
    child = edges["child"].astype(np.int64)
    seen = np.zeros(n, dtype=int)
    for i in range(n):
        m = nodes[i]
        nm, nexp, e0 = int(m["nmoves"]), int(m["nexp"]), int(m["edge0"])
        if i:
            p = nodes[par[i]]
            assert p["has_s2"] == 1 and p["edge0"] <= pe[i] < int(p["edge0"]) + int(p["nmoves"])
            pedge = edges[pe[i]]
            assert (int(pedge["child"]) & 0x7FFF) == i
            assert bool(int(pedge["child"]) & 0x8000) == (m["result"] != RESULT_NONE)
            full = m["has_s2"] == 1 and m["result"] == RESULT_NONE and nexp == nm
            assert int(pedge["hint"]) == ((HINT_FULL | (nm << 23) | e0) if full else 0), i   # hint_pack of the child's record
        if m["has_s2"] != 1:
            assert m["result"] != RESULT_NONE
            continue
        run = child[e0:e0 + nm]
        assert (run[:nm - nexp] == 0x7FFF).all() and (run[nm - nexp:] != 0x7FFF).all()   # expanded last legal move first
        kids = run[nm - nexp:] & 0x7FFF
        assert ((kids > i) & (kids < n)).all()
        seen[kids] += 1
        if m["result"] == RESULT_NONE:
            vsum = int(edges["visits"][e0:e0 + nm].sum())
            if i:
                assert vsum == int(edges[pe[i]]["visits"]) - 1, i               # every later visit went on to one child
            elif fresh_root:
                assert vsum == info["root_visits"] - 1
        else:
            assert nexp == 0
    assert (seen[1:] == 1).all() and seen[0] == 0
    return nodes, edges, info


def expect_pair(st):
    """(our move, reply) of the child a stage chose, from the fixture's (bm, am): a child that ended the game on
    our move has (previous ply, our move) there (mctree.py:185-194)."""
    k = st["chosen"]
    return st["moves"][k], st["replies"][k]


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=["%s-%s" % (c["name"], c["mode"]) for c in CASES])
def test_engine_rerooting_equals_the_reference_tree_of_node(ci, graph):
    from chessrl_amd.engine import LockstepEngine, compute_policy
    c = CASES[ci]
    stages = c["stages"]
    sims = [s["sims"] for s in stages]
    g = ru.case_game(c)
    G = 4
    eng = LockstepEngine(ru.case_net(c).to("cuda:0"), n_games=G, max_sims=max(sims), max_nodes=sum(sims) + 1,
                         numpy_promotion=c["mode"], use_graph=graph)
    if c["fen"]:
        eng.ctx.set_positions(np.stack([board_to_array(board_from_fen(c["fen"]))] * G))
        ok = [eng.ctx.push_moves(np.full(G, uci_to_move(u), np.uint16)) for u in c["prefix_moves"]]
        assert all(o.all() for o in ok)
    else:
        eng.load_moves([[g.board.move_stack[i].m for i in range(len(g))]] * G)
    for i, st in enumerate(stages):
        eng.search(st["sims"], keep_root=i > 0)
        rc = eng.root_children()
        _, plies, _ = eng.ctx.records(with_moves=False)
        for slot in (0, G - 1):
            got = device_stats(rc, slot)
            for k in got:
                assert got[k] == st[k], (c["name"], i, slot, k)
            assert plies[slot] == st["root_plies"]
            if st["noise_seed"] is not None:
                np.random.seed(st["noise_seed"])
            pol = compute_policy(got["visits"], got["root_visits"], plies[slot], noise=st["noise_seed"] is not None)
            assert hexes(pol, "f64") == st["policy"] and int(np.argmax(pol)) == st["chosen"]
            _, _, info = check_tree(eng.ctx, slot, fresh_root=(i == 0))
            assert info["n_nodes"] == st["n_nodes"] and info["kept"] == 0          # the flag is cleared by the begin
        chosen = np.full(G, st["chosen"], dtype=np.int32)
        last = i + 1 == len(stages)
        bm, am = eng.advance(chosen) if last else eng.reroot(chosen, stages[i + 1]["sims"])
        mv, reply = expect_pair(st)
        assert [move_to_uci(m) for m in bm] == [mv] * G
        assert [None if m == NO_MOVE else move_to_uci(m) for m in am] == [reply] * G
        if not last:
            nxt = stages[i + 1]
            for slot in (0, G - 1):
                _, _, info = check_tree(eng.ctx, slot)
                assert info["kept"] == 1 and info["root_visits"] == 1 and info["n_nodes"] == nxt["kept_nodes"]
            rc = eng.ctx.root_children(fields=("nchild", "root_visits"))
            assert list(rc["nchild"]) == [nxt["kept_children"]] * G and list(rc["root_visits"]) == [1] * G
        else:
            assert eng.ctx.fetch_tree(0)[2]["n_nodes"] == 0                        # crl_advance consumes the tree
    assert eng.ctx.counters()["sims"] == G * sum(sims)
    eng.close()


def test_no_root_evaluation_is_counted_for_a_kept_root():
    """The begin of the next move leaves a kept root alone: same nodes, no evaluation counted, the mark cleared;
    a slot without a kept root gets a fresh tree and its root evaluation as before."""
    from chessrl_amd.engine import LockstepEngine
    net = FakeNet(seed=3, prior_shift=30)
    sims = 40
    eng = LockstepEngine(net.to("cuda:0"), n_games=2, max_sims=sims, max_nodes=3 * sims + 1)
    eng.reset()
    eng.search(sims)
    rc = eng.root_children()
    chosen = np.array([int(rc["visits"][0, :rc["nchild"][0]].argmax()), -1], dtype=np.int32)
    eng.reroot(chosen, sims)                                  # slot 0 keeps its tree, slot 1 is left alone
    kept = eng.ctx.fetch_tree(0)[2]
    assert kept["kept"] == 1 and kept["n_nodes"] > 1
    before = eng.ctx.counters()["evals"]
    eng.search_begin(keep_root=True)
    eng.ctx.sync()
    assert eng.ctx.counters()["evals"] == before + 1          # slot 1 only: a fresh root is evaluated, a kept one is not
    after = eng.ctx.fetch_tree(0)[2]
    assert after == dict(kept, kept=0)
    assert eng.ctx.fetch_tree(1)[2] == {"n_nodes": 1, "edge_top": 20, "root_visits": 1, "kept": 0}
    eng.search_begin(keep_root=True)                          # the mark is gone: now both start afresh
    eng.ctx.sync()
    assert eng.ctx.counters()["evals"] == before + 3
    assert eng.ctx.fetch_tree(0)[2]["n_nodes"] == 1
    eng.close()


@pytest.mark.parametrize("sims,graph", [(40, False), (90, True)])
def test_rerooting_with_legal_priors_is_identical_to_rerooting_with_full_policies(sims, graph):
    """CRL_POLICY_LEGAL and CRL_POLICY_LEGAL_RAW against CRL_POLICY_FULL with the real heads: the same trees over
    two re-rootings (kept roots, fall-backs where the budget is short, finished roots)."""
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.model import ChessModel
    from tests.test_gpu_search import move_ids, random_prefix_games
    model = ChessModel(blocks=2, filters=64, seed=3)
    games = random_prefix_games(24, 70, seed=29)
    out = []
    for legal, raw in ((False, False), (True, False), (True, None)):
        eng = LockstepEngine(model, n_games=24, max_sims=sims, max_nodes=sims + sims // 2, legal_priors=legal,
                             use_graph=graph, raw_priors=raw)
        assert eng.legal_priors == legal and eng.raw_priors == (raw is None)
        eng.load_moves([move_ids(g) for g in games])
        log = []
        for hop in range(3):
            eng.search(sims, keep_root=True)
            rc = eng.root_children()
            live = np.arange(rc["visits"].shape[1])[None, :] < rc["nchild"][:, None]     # (rows keep stale tails)
            chosen = np.where(rc["nchild"] > 0, np.where(live, rc["visits"], -1).argmax(1), -1).astype(np.int32)
            fetch = eng.ctx.reroot_fetch(chosen, sims)
            log.append((rc, fetch))
            for slot in np.nonzero(fetch["kept_nodes"])[0][:4]:
                check_tree(eng.ctx, int(slot))
        out.append((log, eng.ctx.counters()))
        eng.close()
    kept = np.concatenate([f["kept_nodes"] for _, f in out[0][0]])
    assert (kept > 0).any() and (kept == 0).any()                         # kept roots and fall-backs both happen
    for log, cnt in out[1:]:
        for (a, fa), (b, fb) in zip(out[0][0], log):
            assert np.array_equal(a["nchild"], b["nchild"]) and np.array_equal(a["visits"], b["visits"])
            assert np.array_equal(a["values"].view(np.uint64), b["values"].view(np.uint64))
            assert np.array_equal(a["priors"].view(np.uint32), b["priors"].view(np.uint32))
            assert np.array_equal(a["replies"], b["replies"]) and np.array_equal(a["moves"], b["moves"])
            assert np.array_equal(a["root_visits"], b["root_visits"])
            for k in fa:
                assert np.array_equal(fa[k], fb[k]), k
        assert {k: int(v) for k, v in cnt.items()} == {k: int(v) for k, v in out[0][1].items()}


MIXED_FENS = ["7k/8/5KQ1/8/8/8/8/8 w - - 0 1",                    # the search chooses a mate on our move
              "7k/5Q2/6K1/8/8/8/8/8 b - - 0 1",                   # stalemate: a finished root
              "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1",   # 218 legal moves
              "7k/8/4K3/8/6Q1/8/8/8 w - - 94 80",                 # claims and mates inside the tree
              "r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1"]


def mixed_games(G):
    """FEN roots (empty move stack) in the first slots of every group of eight, seeded random prefixes from the
    standard position in the others."""
    rng = np.random.default_rng(5)
    games = []
    for i in range(G):
        if i % 8 < len(MIXED_FENS) and i < 40:
            games.append(OracleGame(board=board_from_fen(MIXED_FENS[i % 8])))
            continue
        g = OracleGame()
        while len(g) < (i % 23) and g.get_result() is None:
            lm = g.legal_move_ids()
            g.move(move_to_uci(lm[int(rng.integers(len(lm)))]))
        games.append(g)
    return games


def test_mixed_batch_of_64_slots_in_one_launch():
    """One crl_reroot over 64 slots that hold, side by side: roots that are kept, roots that fall back (the
    tree does not fit the next move's simulations), a finished game, slots with chosen = -1, a child that ended
    the game on our move, and the 218-move position -- each against the continuation oracle, over two moves."""
    from chessrl_amd.engine import LockstepEngine, compute_policy
    G, sims, nodes = 64, 50, 76
    net = FakeNet(seed=13, prior_shift=30)
    games = mixed_games(G)
    eng = LockstepEngine(net.to("cuda:0"), n_games=G, max_sims=sims, max_nodes=nodes)
    start = board_to_array(OracleGame().board_at(0))
    eng.ctx.set_positions(np.stack([board_to_array(g.board_at(0)) if len(g) == 0 else start for g in games]))
    tbl = np.full((G, 32), NO_MOVE, np.uint16)
    cnt = np.zeros(G, np.int32)
    for i, g in enumerate(games):
        cnt[i] = len(g)
        tbl[i, :len(g)] = [g.board.move_stack[k].m for k in range(len(g))]
    assert list(eng.ctx.push_sequences(tbl, cnt)) == list(cnt)
    agent = mcts_oracle.OracleAgent(net)
    roots = [ru.new_root(g) if g.get_result() is None else None for g in games]
    kinds = set()
    for move in range(2):
        eng.search(sims, keep_root=True)
        rc = eng.root_children()
        _, plies, _ = eng.ctx.records(with_moves=False)
        chosen = np.full(G, -1, dtype=np.int32)
        for i, root in enumerate(roots):
            if root is None:
                assert rc["nchild"][i] == 0
                kinds.add("finished")
                continue
            ru.grow(root, agent, sims, eng.numpy_promotion)
            exp = ru.root_stats(root)
            got = device_stats(rc, i)
            for k in got:
                assert got[k] == exp[k], (move, i, k)
            if len(root.kids) + len(root.todo) == 218:
                kinds.add("218 moves")
            pol = compute_policy(got["visits"], got["root_visits"], plies[i], noise=False)
            if i % 8 != 7:                                       # every eighth slot is left alone
                chosen[i] = int(np.argmax(pol))
        out = eng.ctx.reroot_fetch(chosen, sims)
        for i, root in enumerate(roots):
            if root is None:
                assert out["kept_nodes"][i] == 0 and out["bm"][i] == NO_MOVE
                continue
            if chosen[i] < 0:
                # left alone: the tree stays as it was and the game does not move; the next begin starts it afresh
                kinds.add("left alone")
                assert out["bm"][i] == NO_MOVE and out["kept_nodes"][i] == 0
                assert check_tree(eng.ctx, i)[2]["n_nodes"] == ru.count(root)
                roots[i] = ru.new_root(games[i])
                continue
            ch = root.kids[chosen[i]]
            assert move_to_uci(out["bm"][i]) == ch.move
            assert (None if out["am"][i] == NO_MOVE else move_to_uci(out["am"][i])) == (None if ch.reply == "00000" else ch.reply)
            assert out["results"][i] == (RESULT_NONE if ch.result is None else ch.result)
            if ch.result is not None:
                kinds.add("ended on our move" if ch.reply == "00000" else "ended after the reply")
                assert out["kept_nodes"][i] == 0
                roots[i] = None
            elif ru.count(ch) + sims <= nodes:
                kinds.add("kept")
                assert out["kept_nodes"][i] == ru.count(ch) and out["kept_children"][i] == len(ch.kids)
                assert out["legal_counts"][i] == len(ch.kids) + len(ch.todo)
                check_tree(eng.ctx, i)
                roots[i] = ru.reroot(root, chosen[i])
            else:
                kinds.add("fell back")
                assert out["kept_nodes"][i] == 0 and eng.ctx.fetch_tree(i)[2]["n_nodes"] == 0
                roots[i] = ru.new_root(ch.state)
    assert kinds >= {"kept", "fell back", "finished", "left alone", "ended on our move", "218 moves"}, kinds
    eng.ctx.sync()
    eng.close()


@pytest.mark.parametrize("net_seed,shift", [(3, 30), (5, 29), (9, 24)])
def test_whole_games_with_tree_reuse_match_the_oracle(net_seed, shift):
    """SelfPlayRunner(reuse_tree=True, noise=False), S = 60, 121 nodes per tree, 24 moves: every game equals
    play_game_reuse move for move, and the runner's counters equal the oracle's counts of kept / fallen-back
    moves -- both non-zero, so the test cannot pass by never reusing (agent as white from the standard position
    the oracle keeps the tree on 22 / 22 / 17 of 24 moves for these nets and falls back on 2 / 2 / 7)."""
    from chessrl_amd.selfplay import SelfPlayRunner, game_color
    net = FakeNet(seed=net_seed, prior_shift=shift)
    S, nodes, moves, seed, G = 60, 121, 24, 4, 4
    run = SelfPlayRunner(net.to("cuda:0"), n_parallel=G, sims=S, seed=seed, noise=False, total_games=G,
                         max_plies=512, reuse_tree=True, tree_nodes=nodes)
    run.run(max_moves=moves)
    rec_moves, plies, _ = run.engine.ctx.records()
    kept = fell = kept_nodes = 0
    assert not run.finished
    by_colour = {}                                           # (noise off: games of one colour are one game)
    colours = [game_color(seed, int(run.game_id[slot])) for slot in range(G)]
    assert set(colours) == {True, False}
    for slot in range(G):
        r = by_colour.get(colours[slot])
        if r is None:
            r = by_colour[colours[slot]] = ru.play_game_reuse(mcts_oracle.OracleAgent(net), S, nodes, moves=moves,
                                                              mode=run.engine.numpy_promotion, player_color=colours[slot])
        g = r["game"]
        assert list(rec_moves[slot, :plies[slot]]) == [g.board.move_stack[i].m for i in range(len(g))], slot
        kept, fell, kept_nodes = kept + r["kept"], fell + r["fell_back"], kept_nodes + sum(r["kept_nodes"])
    assert kept > 0 and fell > 0
    assert (run.reuse_kept, run.reuse_fell_back, run.reuse_kept_nodes) == (kept, fell, kept_nodes)
    print("tree reuse, net (%d, %d): kept %d, fell back %d, kept nodes %d" % (net_seed, shift, kept, fell, kept_nodes))
    run.close()


def test_one_noisy_game_with_tree_reuse_matches_the_oracle():
    """Dirichlet noise on, drawn ahead from the per-game streams for min(legal, kept children + sims) children."""
    from chessrl_amd.selfplay import SelfPlayRunner, game_color
    net = FakeNet(seed=5, prior_shift=29)
    S, nodes, moves, seed = 60, 181, 16, 7
    run = SelfPlayRunner(net.to("cuda:0"), n_parallel=2, sims=S, seed=seed, noise=True, total_games=2,
                         max_plies=512, reuse_tree=True, tree_nodes=nodes)
    run.run(max_moves=moves)
    rec_moves, plies, _ = run.engine.ctx.records()
    kept = 0
    for slot in range(2):
        gid = int(run.game_id[slot])
        r = ru.play_game_reuse(mcts_oracle.OracleAgent(net), S, nodes, moves=moves, mode=run.engine.numpy_promotion,
                               noise=True, rng=np.random.default_rng([seed, gid]), player_color=game_color(seed, gid))
        g = r["game"]
        assert list(rec_moves[slot, :plies[slot]]) == [g.board.move_stack[i].m for i in range(len(g))], gid
        kept += r["kept"]
    assert run.reuse_kept == kept > 0
    run.close()


def test_records_with_tree_reuse_do_not_depend_on_slot_batch_or_world_size():
    """Compaction moves games between slots after the re-root: the kept tree has to travel with its game
    (crl_copy_game_tree).  The same seeds with compact on / off and with two ranks against one give identical
    records."""
    from chessrl_amd.selfplay import SelfPlayRunner
    net = FakeNet(seed=17, prior_shift=30).to("cuda:0")
    kw = dict(sims=6, seed=9, noise=True, total_games=150, max_plies=2048, reuse_tree=True, tree_nodes=19)
    a = SelfPlayRunner(net, n_parallel=128, compact=True, **kw)
    ra = {r.game_id: r for r in a.run()}
    assert a.G == 64 and a.reuse_kept > 0 and a.reuse_fell_back > 0
    a.close()
    b = SelfPlayRunner(net, n_parallel=128, compact=False, **kw)
    rb = {r.game_id: r for r in b.run()}
    assert b.G == 128 and (b.reuse_kept, b.reuse_fell_back, b.reuse_kept_nodes) == (a.reuse_kept, a.reuse_fell_back, a.reuse_kept_nodes)
    b.close()
    assert sorted(ra) == sorted(rb) == list(range(150))
    for k in ra:
        assert ra[k] == rb[k], k
    got = {}
    for rank in range(2):
        r = SelfPlayRunner(net, n_parallel=64, rank=rank, world=2, **kw)
        got.update({x.game_id: x for x in r.run()})
        r.close()
    assert sorted(got) == sorted(ra)
    for k in ra:
        assert got[k] == ra[k], k
    plain = SelfPlayRunner(net, n_parallel=128, **dict(kw, reuse_tree=False, tree_nodes=None))
    rp = {r.game_id: r for r in plain.run()}
    plain.close()
    assert any(rp[k] != ra[k] for k in ra)                     # reuse changes what is played: the flag is not a no-op


def test_without_the_flag_nothing_changes():
    """reuse_tree=False: a seeded 16-game run equals oracle.mcts_oracle.play_game move for move, and
    crl_advance / crl_advance_fetch still leave no tree (the next search starts from one node: root visits S + 1)."""
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.selfplay import SelfPlayRunner, game_color
    net = FakeNet(seed=21, prior_shift=30)
    seed, sims = 5, 6
    run = SelfPlayRunner(net.to("cuda:0"), n_parallel=8, sims=sims, seed=seed, noise=True, total_games=16, max_plies=2048)
    assert not run.reuse_tree and run.engine.max_nodes == sims + 1
    recs = sorted(run.run(), key=lambda r: r.game_id)
    assert (run.reuse_kept, run.reuse_fell_back) == (0, 0)
    run.close()
    assert [r.game_id for r in recs] == list(range(16))
    for r in recs:
        g = mcts_oracle.play_game(mcts_oracle.OracleAgent(net), max_iters=sims, noise=True,
                                  player_color=game_color(seed, r.game_id), rng=np.random.default_rng([seed, r.game_id]))
        assert r.get_history()["moves"] == g.get_history()["moves"] and r.result == g.get_result()
    S = 30
    eng = LockstepEngine(net.to("cuda:0"), n_games=4, max_sims=S, max_nodes=4 * S)
    eng.reset()
    for fetch in (False, True):
        eng.search(S)
        rc = eng.root_children()
        chosen = rc["visits"].argmax(1).astype(np.int32)
        if fetch:
            eng.ctx.advance_fetch(chosen)
        else:
            eng.advance(chosen)
        info = eng.ctx.fetch_tree(0)[2]
        assert info["n_nodes"] == 0 and info["kept"] == 0
        eng.search(S, keep_root=True)                            # nothing was kept: fresh trees even when asked to keep
        rc = eng.root_children()
        assert list(rc["root_visits"]) == [S + 1] * 4
        assert all(int(rc["visits"][i, :rc["nchild"][i]].sum()) == S for i in range(4))
        eng.advance(rc["visits"].argmax(1).astype(np.int32))
    eng.close()


def test_dropin_tree_of_node_equals_the_reference(golden_dir):
    """SelfPlayTree(tree.root.children[k]).search_move: (bm, am) and the children of the fixture."""
    from chessrl_amd.agent import Agent
    from chessrl_amd.game import Game
    from chessrl_amd.mctree import SelfPlayTree
    for c in CASES:
        if c["name"] not in ("opening_three_equal_moves", "mates_and_fifty_move_claims_in_the_tree", "noisy_hop", "tiny_budget"):
            continue
        stages = c["stages"]
        agent = Agent(True, model=ru.case_net(c).to("cuda:0"), numpy_promotion=c["mode"],
                      tree_nodes=sum(s["sims"] for s in stages) + 1)
        g = Game(board=c["fen"]) if c["fen"] else Game()
        for u in c["prefix_moves"]:
            assert g.move(u)
        root = g
        for i, st in enumerate(stages):
            tree = SelfPlayTree(root, threads=1)
            assert tree.root.visits == 1
            if i:
                assert tree.root.state.get_history()["moves"][-2:] == [stages[i - 1]["bm"], stages[i - 1]["am"]]
            if st["noise_seed"] is not None:
                np.random.seed(st["noise_seed"])
            pair = tree.search_move(agent, max_iters=st["sims"], noise=st["noise_seed"] is not None, ai_move=True)
            assert pair == (st["bm"], st["am"]), (c["name"], c["mode"], i)
            kids = tree.root.children
            assert tree.root.visits == st["root_visits"]
            assert [k.visits for k in kids] == st["visits"]
            assert hexes(np.array([k.value for k in kids], np.float64), "f64") == st["values"]
            assert hexes(np.array([k.prior for k in kids], np.float32), "f32") == st["priors"]
            assert [(k.move, k.reply) for k in kids] == list(zip(st["moves"], st["replies"]))
            root = kids[st["chosen"]]
        g.free()


def test_dropin_limits_are_errors_never_a_silent_fresh_search():
    from chessrl_amd.agent import Agent
    from chessrl_amd.game import Game
    from chessrl_amd.mctree import SelfPlayTree, Tree
    net = FakeNet(seed=3, prior_shift=30).to("cuda:0")
    agent = Agent(True, model=net, tree_nodes=200)
    g = Game()
    tree = SelfPlayTree(g, threads=1)
    tree.search_move(agent, max_iters=60, noise=False, ai_move=True)
    first = tree.root.children
    k = int(np.argmax([c.visits for c in first]))
    # a hop with another max_iters runs in the engine that HOLDS the tree, not in an empty one
    hop = SelfPlayTree(first[k], threads=1)
    assert hop.root.visits == 1 and hop.root.state.get_history()["moves"] == [first[k].move, first[k].reply]
    hop.search_move(agent, max_iters=40, noise=False, ai_move=True)
    assert hop.root.visits == 41 and sum(c.visits for c in hop.root.children) == first[k].visits - 1 + 40
    # the first tree's device tree is gone now: its other children cannot be continued
    with pytest.raises(RuntimeError, match="device tree .* is gone"):
        SelfPlayTree(first[(k + 1) % len(first)], threads=1).search_move(agent, max_iters=40, noise=False)
    # ... and a search from a Game in the same engine overwrites the hop's tree
    other = SelfPlayTree(g, threads=1)
    other.search_move(agent, max_iters=60, noise=False)
    with pytest.raises(RuntimeError, match="device tree .* is gone"):
        SelfPlayTree(hop.root.children[0], threads=1).search_move(agent, max_iters=10, noise=False)
    # a budget the engine cannot hold names the size that was needed
    kk = int(np.argmax([c.visits for c in other.root.children]))
    need = other.root.children[kk].visits + 190
    with pytest.raises(ValueError, match="tree_nodes >= %d" % need):
        SelfPlayTree(other.root.children[kk], threads=1).search_move(agent, max_iters=190, noise=False)
    SelfPlayTree(other.root.children[kk], threads=1).search_move(agent, max_iters=50, noise=False)   # still there
    # the default budget (max_iters + 1) has no room for a kept subtree
    small = Agent(True, model=net)
    t = SelfPlayTree(g, threads=1)
    t.search_move(small, max_iters=30, noise=False)
    with pytest.raises(ValueError, match="tree_nodes >="):
        SelfPlayTree(t.root.children[int(np.argmax([c.visits for c in t.root.children]))], threads=1).search_move(
            small, max_iters=30, noise=False)
    for bad in (None, "e2e4", 5, object()):
        with pytest.raises(TypeError):
            Tree(bad)
        with pytest.raises(TypeError):
            SelfPlayTree(bad)
    g.free()
