"""No GPU: what tests/test_gpu_opponent_reply.py leans on, asserted with the oracle alone, and the host refusals of a
search against the built-in opponent (``LockstepEngine(reply=MinimaxPlayer)``).

1. on the random-prefix roots the opponent's reply differs from the net's greedy reply in most new nodes: a kernel
   that kept the net's reply cannot pass the GPU tests;
2. the set-up roots produce nodes that end on our move (mate, the fifty-move claim), nodes whose S2 is terminal by the
   opponent's mating reply, and promotion replies;
3. at depth 2 a node limit exists for which the middlegame root has cut and uncut replies (``node_limit_for``, which
   the GPU test uses);
4. the refusals, by name, before anything touches a device.
"""
import functools

import pytest

from tests import opponent_reply_util as u
from tests import opponent_util as ou

SIMS = 48


def full(root, depth):
    return u.tree(root, depth, ou.NODE_LIMIT, SIMS, "nep50")


@pytest.mark.parametrize("depth", [1, 2])
def test_the_opponents_reply_is_rarely_the_nets(depth):
    total = differ = 0
    for i in range(u.N_PREFIX):
        _, log = full(i, depth)
        total += len(log)
        differ += sum(1 for reply, greedy, _, _ in log if reply != greedy)
    print("depth", depth, "replies that differ from the greedy reply:", differ, "of", total)
    assert total >= u.N_PREFIX * SIMS - 8 and 2 * differ > total


@pytest.mark.parametrize("depth", [1, 2])
def test_set_up_roots_reach_the_edge_cases(depth):
    def ended_on_our_move(r, log):
        return (r.n_nodes - 1) - len(log)                  # new nodes without a reply

    r, log = full(u.FEN0, depth)                           # K+Q v K: mates (and stalemates) on our move
    assert ended_on_our_move(r, log) >= 1 and u.NULL_MOVE in r.child_replies
    mates = [m for m, rep in zip(r.child_moves, r.child_replies) if rep == u.NULL_MOVE]
    g = u.roots()[u.FEN0].get_copy()
    assert g.move(mates[0]) and g.get_result() is not None
    r, log = full(u.FEN0 + 5, depth)                       # clock 97: the fifty-move claim two plies down
    assert ended_on_our_move(r, log) == 26 and r.n_nodes == SIMS + 1
    r, log = full(u.FEN0 + 1, depth)                       # the opponent's reply mates: S2 terminal, the tree stays small
    assert len(log) == 2 and r.n_nodes == 3 and ended_on_our_move(r, log) == 0
    for move, reply in zip(r.child_moves, r.child_replies):
        g = u.roots()[u.FEN0 + 1].get_copy()
        assert g.move(move) and g.move(reply) and g.get_result() == -1
    for k in (2, 3):                                       # promotion replies
        _, log = full(u.FEN0 + k, depth)
        promotions = sum(1 for reply, _, _, _ in log if len(reply) == 5)
        print("depth", depth, "root", k, "promotion replies", promotions)
        assert promotions >= 5


@functools.lru_cache(maxsize=None)
def node_limit_for(depth=2, sims=SIMS):
    """The median node count of the middlegame root's uncut replies: about half of them are cut under it."""
    _, log = u.tree(u.MIDDLEGAME, depth, ou.NODE_LIMIT, sims, "nep50")
    counts = sorted(nodes for _, _, nodes, _ in log)
    return counts[len(counts) // 2]


def test_a_node_limit_mixes_cut_and_uncut_replies():
    _, log = u.tree(u.MIDDLEGAME, 2, 120, SIMS, "nep50")
    assert len(log) == SIMS and all(flag == ou.CUT and nodes == 120 for _, _, nodes, flag in log)
    _, log = full(u.MIDDLEGAME, 2)
    assert len(log) == SIMS and not any(flag for _, _, _, flag in log)
    limit = node_limit_for()
    r, log = u.tree(u.MIDDLEGAME, 2, limit, SIMS, "nep50")
    cut = sum(1 for _, _, _, flag in log if flag == ou.CUT)
    print("limit", limit, "cut", cut, "of", len(log))
    assert 0 < cut < len(log) and all(flag in (0, ou.CUT) for _, _, _, flag in log)
    assert all(nodes == limit for _, _, nodes, flag in log if flag == ou.CUT)
    assert all(nodes <= limit for _, _, nodes, flag in log if not flag)


# ---- the refusals: ValueError by name, TypeError for another type, all before a device is touched ----------------
def test_engine_refuses_what_a_reply_search_does_not_cover():
    from chessrl_amd.engine import LockstepEngine, StampRing
    from chessrl_amd.opponent import MinimaxPlayer
    from chessrl_amd.simulation import Rollouts
    net, player = object(), MinimaxPlayer(False, 2)
    with pytest.raises(ValueError, match="reply= cannot be combined with threads"):
        LockstepEngine(net, n_games=4, max_sims=10, reply=player, threads=2)
    with pytest.raises(ValueError, match="reply= cannot be combined with rollouts"):
        LockstepEngine(net, n_games=4, max_sims=10, reply=player, simulate=Rollouts(repetitions=2, max_moves=10, seed=1))
    with pytest.raises(ValueError, match="reply= cannot be combined with max_nodes"):
        LockstepEngine(net, n_games=4, max_sims=10, reply=player, max_nodes=40)
    with pytest.raises(TypeError, match="MinimaxPlayer"):
        LockstepEngine(net, n_games=4, max_sims=10, reply="stockfish")
    with pytest.raises(TypeError, match="MinimaxPlayer"):
        LockstepEngine(net, n_games=4, max_sims=10, reply=2)
    # the methods of an engine that has a player: an instance without a device behind it
    eng = LockstepEngine.__new__(LockstepEngine)
    eng.reply, eng.threads, eng.max_sims = player, 1, 10
    with pytest.raises(ValueError, match="reply= cannot be combined with reroot"):
        eng.reroot([0, 0, 0, 0], 10)
    with pytest.raises(ValueError, match="reply= cannot be combined with keep_root"):
        eng.search_begin(keep_root=True)
    with pytest.raises(ValueError, match="reply= cannot be combined with keep_root"):
        eng.search(10, keep_root=True)
    with pytest.raises(ValueError, match="reply= cannot be combined with set_stamps"):
        eng.set_stamps(StampRing.__new__(StampRing))
    eng.reply = None
    with pytest.raises(ValueError, match="without reply"):
        eng.set_reply_depths([1, 2, 1, 2])
    with pytest.raises(ValueError, match="without reply"):
        eng.reply_stats()


def test_tree_agent_and_benchmark_refuse_on_the_host():
    from chessrl_amd import benchmark as bm
    from chessrl_amd.agent import Agent
    from chessrl_amd.mctree import Node, SelfPlayTree, Tree
    from chessrl_amd.opponent import MinimaxPlayer
    from chessrl_amd.simulation import Rollouts
    player = MinimaxPlayer(False, 2)
    kept = Node(None, 3, 0.5, 0.1, "e2e4", "e7e5", tree=object(), index=0)
    kept._state = object()
    with pytest.raises(ValueError, match="reply= cannot continue a Node"):
        SelfPlayTree(kept, reply=player)
    with pytest.raises(ValueError, match="reply= cannot be combined with threads"):
        SelfPlayTree(kept, threads=6, virtual_loss=True, reply=player)
    with pytest.raises(ValueError, match="reply= cannot be combined with rollouts"):
        SelfPlayTree(kept, reply=player, simulate=Rollouts(repetitions=2, max_moves=10, seed=1))
    with pytest.raises(TypeError, match="MinimaxPlayer"):
        SelfPlayTree(kept, reply="stockfish")

    # a Node of a tree that was searched with reply=: the engine that holds it has the player
    class Holder(object):
        pass
    src, eng = Holder(), Holder()
    src._engine, eng._tree_owner, eng.reply, eng.threads = eng, src, player, 1
    child = Node(None, 3, 0.5, 0.1, "e2e4", "e7e5", tree=src, index=0)
    child._state = object()
    with pytest.raises(ValueError, match="reply= cannot continue a Node"):
        Tree(child)._continue_on_device(10)

    agent = Agent(True, model=object())
    with pytest.raises(ValueError, match="reply= cannot be combined with threads"):
        agent.engine_for(10, threads=2, reply=player)
    with pytest.raises(ValueError, match="reply= cannot be combined with rollouts"):
        agent.engine_for(10, simulate=Rollouts(repetitions=2, max_moves=10, seed=1), reply=player)
    with pytest.raises(TypeError, match="MinimaxPlayer"):
        agent.engine_for(10, reply="stockfish")
    with pytest.raises(ValueError, match="sims"):
        bm.benchmark(None, games=4, sims=-1, model=object())
    with pytest.raises(ValueError, match="opponent_depth"):
        bm.benchmark(None, games=4, sims=8, opponent_depth=6, model=object())
