"""CPU restatement of a search against the built-in opponent (``LockstepEngine(reply=MinimaxPlayer)``,
csrc/opponent.hpp ``k_reply_opponent``).

TEST INFRASTRUCTURE.  ``oracle.mcts_oracle.search`` takes the reply of a new node from
``agent.best_move(S1, real_game=True)``; an ``OracleAgent`` that answers there with ``tests.opponent_util.alphabeta``
is the exact expected tree.  Nothing under ``oracle/`` changes.

  ReplyAgent      the agent; logs (reply, the net's greedy reply, nodes, flag) per call
  roots           16 games: 8 random prefixes, 2 standard starts, 6 set-up positions
  tree            the restated search of one root, cached per (root, depth, limit, sims, mode)
  cpu_games       the benchmark's game loop against the opponent
  load_games      the roots into a device context
"""
import functools

import numpy as np

from oracle import mcts_oracle
from oracle.chess_oracle import NULL_MOVE, OracleGame, board_from_fen, board_to_array, move_to_uci, uci_to_move
from oracle.fakenet import FakeNet
from tests import opponent_util as ou

NO_MOVE = 0xFFFF
FENS = ("7k/8/5K2/6Q1/8/8/8/8 w - - 0 1",                                       # mates on our move
        "7k/8/8/8/8/1q6/r7/6K1 w - - 0 1",                                      # the opponent's reply mates
        "8/P6k/8/8/8/8/7p/K7 w - - 0 1",                                        # promotion replies
        "k7/7P/8/8/8/8/p7/7K b - - 0 1",
        "r3k2r/pppq1ppp/2n2n2/3pp3/3PP3/2N2N2/PPPQ1PPP/R3K2R w KQkq - 4 8",      # a middlegame: the node limit
        "8/8/8/4k3/8/8/3K4/7R w - - 97 90")                                     # the fifty-move claim on our move
N_PREFIX, N_START = 8, 2
FEN0 = N_PREFIX + N_START                       # root index of FENS[0]
MIDDLEGAME = FEN0 + 4
NET_SEED, NET_SHIFT = 5, 29


def net():
    return FakeNet(seed=NET_SEED, prior_shift=NET_SHIFT)


class ReplyAgent(mcts_oracle.OracleAgent):
    """``best_move(S1, real_game=True)`` is the built-in opponent's move of ``depth`` under ``limit``."""

    def __init__(self, net, depth, limit=ou.NODE_LIMIT, log_greedy=True, **kw):
        super().__init__(net, **kw)
        self.depth, self.limit, self.log_greedy = depth, limit, log_greedy
        self.log = []                           # (reply uci, greedy reply uci or None, nodes, flag)

    def best_move(self, game, real_game=False, **kw):
        if not real_game:
            return super().best_move(game, real_game=False, **kw)
        m, _, nodes, flag = ou.alphabeta(game, self.depth, self.limit)
        assert m != NO_MOVE
        greedy = super().best_move(game, real_game=True) if self.log_greedy else None
        self.log.append((move_to_uci(m), greedy, nodes, flag))
        return move_to_uci(m)


@functools.lru_cache(maxsize=None)
def roots():
    from tests.test_gpu_search import random_prefix_games
    games = list(random_prefix_games(N_PREFIX, 60, seed=129))
    games += [OracleGame() for _ in range(N_START)]
    games += [OracleGame(board=board_from_fen(f)) for f in FENS]
    return tuple(games)


@functools.lru_cache(maxsize=None)
def tree(root, depth, limit, sims, mode):
    """(SearchResult, log) of root ``root``: computed once, never changed."""
    agent = ReplyAgent(net(), depth, limit)
    r = mcts_oracle.search(roots()[root], agent, sims, noise=False, mode=mode)
    return r, tuple(agent.log)


def reply_ids(r):
    return [NO_MOVE if u == NULL_MOVE else uci_to_move(u) for u in r.child_replies]


def assert_tree_equal(rc, i, r, what=None):
    """Row ``i`` of ``root_children()`` against the restated SearchResult ``r``: integers, float64 sums by bit pattern,
    float32 priors by value."""
    n = int(rc["nchild"][i])
    assert n == len(r.visits), (what, i)
    assert list(rc["visits"][i, :n]) == r.visits, (what, i)
    assert int(rc["root_visits"][i]) == r.root_visits, (what, i)
    assert [move_to_uci(m) for m in rc["moves"][i, :n]] == r.child_moves, (what, i)
    assert list(rc["replies"][i, :n]) == reply_ids(r), (what, i)
    assert np.array_equal(rc["values"][i, :n].view(np.uint64), np.array(r.values, dtype=np.float64).view(np.uint64)), (what, i)
    assert np.array_equal(rc["priors"][i, :n], np.array(r.priors, dtype=np.float32)), (what, i)


def load_games(ctx, games):
    """Slot i of the context becomes games[i]: its first position, then its move list."""
    ctx.set_positions(np.stack([board_to_array(g.board_at(len(g))) for g in games]))
    n = max(max(len(g) for g in games), 1)
    tbl = np.full((len(games), n), NO_MOVE, np.uint16)
    cnt = np.array([len(g) for g in games], np.int32)
    for i, g in enumerate(games):
        tbl[i, :len(g)] = [g.board.move_stack[k].m for k in range(len(g))]
    assert list(ctx.push_sequences(tbl, cnt)) == list(cnt)


@functools.lru_cache(maxsize=None)
def cpu_games(colors, depth, sims, max_plies, mode):
    """The benchmark's loop on the oracle: the opponent opens where the agent is black; then per move the restated
    search (noise off), our move and -- unless the game ended on it -- the stored reply, which is what k_advance
    pushes.  A game goes on while it runs and has fewer than ``max_plies`` plies.  -> (move lists, results)."""
    moves, results = [], []
    for white in colors:
        g = OracleGame()
        agent = ReplyAgent(net(), depth, log_greedy=False)
        if not white:
            ou.play_ply(g, depth)
        while g.get_result() is None and len(g) < max_plies:
            r = mcts_oracle.search(g, agent, sims, noise=False, mode=mode)
            assert g.move(r.child_moves[r.chosen])
            if r.child_replies[r.chosen] != NULL_MOVE:
                assert g.move(r.child_replies[r.chosen])
        moves.append(g.get_history()["moves"])
        results.append(g.get_result())
    return moves, results
