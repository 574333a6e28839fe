"""CPU restatement of ``chessrl_amd.arena`` over ``oracle.mcts_oracle.search`` and ``OracleGame``.

TEST INFRASTRUCTURE.  Written from the arena's contract, not from its code:

  pairs and colours   games 2i and 2i + 1 share an opening; A is white in 2i and black in 2i + 1
  openings            ``opening_plies`` random plies per pair -- ``gen_data.opening_words`` from ``random.Random(seed)``
                      played by ``rollout_util.run_in_slot``, the restatement of ``Context.rollout_games`` -- or a given
                      list of UCI moves / a FEN per pair
  a ply               the side to move searches with its OWN agent (``mcts_oracle.search``) and plays ONE ply:
                      ``game.move(child_moves[chosen])``; with ``sims=0`` its ``best_move(real_game=True)``
  the end             a game is searched while it runs and has played fewer than ``max_plies`` plies after its opening
  noise               game i draws from ``np.random.default_rng([seed, i])``, one row per searched ply
  the tally           a_won / b_won / drawn / unfinished, ``score_a = (a_won + drawn / 2) / played``, and the same
                      over A's white games

The two "weight sets" of the tests are FakeNets: exact integer functions of the planes, so trees and games are compared
bit for bit.
"""
import functools
import random

import numpy as np

from oracle import mcts_oracle
from oracle.chess_oracle import OracleGame, board_from_fen
from oracle.fakenet import FakeNet
from tests import rollout_util as ru

NET_A = dict(seed=3, prior_shift=30)
NET_B = dict(seed=7, prior_shift=30)

FENS = ["7k/5Q2/6K1/8/8/8/8/8 w - - 0 1",                  # white mates in one
        "6k1/5ppp/8/8/8/8/5PPP/3R2K1 w - - 0 1",           # white mates in one (back rank)
        "7k/8/6K1/8/8/8/8/8 w - - 0 1",                    # bare kings: drawn before a move
        "k7/2Q5/1K6/8/8/8/8/8 b - - 0 1",                  # black is stalemated: drawn before a move
        "8/8/8/8/8/5k2/6q1/7K w - - 99 80",                # white is mated: -1 before a move
        "r3k3/8/8/8/8/8/8/4K2R w - - 98 60"]               # the fifty-move rule ends it after two plies

RANDOM_SET = dict(games=8, sims=24, seed=11, opening_plies=4, max_plies=12)
FEN_SET = dict(games=12, sims=32, openings=FENS, max_plies=10)


def nets():
    return FakeNet(**NET_A), FakeNet(**NET_B)


def float_mode():
    """the arithmetic of ``10 * prior`` under the numpy of this process (what the engine's "auto" resolves to)"""
    return "legacy" if (10 * np.float32(0.1)).dtype == np.float64 else "nep50"


def random_openings(pairs, opening_plies, seed):
    """UCI move lists: every pair plays ``opening_plies`` random plies from the word rows ``gen_data`` draws; a slot
    that used up its row goes on with its row of the next block."""
    from chessrl_amd import gen_data as gd
    if opening_plies == 0:
        return [[] for _ in range(pairs)]
    rng = random.Random(seed)
    blocks = []

    def words_of(g):
        k = 0
        while True:
            if k == len(blocks):
                blocks.append(gd.opening_words(rng, pairs, opening_plies))
            for w in blocks[k][g]:
                yield int(w)
            k += 1

    out = []
    for g in range(pairs):
        game, it = OracleGame(), words_of(g)
        ru.run_in_slot(game, lambda: next(it), max_moves=opening_plies)
        out.append([str(m) for m in game.board.move_stack])
    return out


def start_game(opening):
    """OracleGame after an opening: a FEN string, or UCI moves from the standard position."""
    if isinstance(opening, str):
        return OracleGame(board=board_from_fen(opening))
    g = OracleGame()
    for u in opening:
        assert g.move(u), u
    return g


def tally(a_white, results):
    def count(idx):
        a = b = d = u = 0
        for i in idx:
            r = results[i]
            if r is None:
                u += 1
            elif r == 0:
                d += 1
            elif (r == 1) == a_white[i]:
                a += 1
            else:
                b += 1
        n = len(idx)
        return dict(played=n, a_won=a, b_won=b, drawn=d, unfinished=u, score_a=(a + d / 2) / n if n else 0.0)
    out = count(range(len(a_white)))
    out["as_white"] = count([i for i, c in enumerate(a_white) if c])
    return out


def play(net_a, net_b, games, sims, seed=0, opening_plies=6, openings=None, max_plies=512, noise=False):
    """The arena on the CPU: the dict ``chessrl_amd.arena.arena`` returns."""
    agents = {True: mcts_oracle.OracleAgent(net_a), False: mcts_oracle.OracleAgent(net_b)}      # keyed by "is A"
    if openings is None:
        openings = random_openings(games // 2, opening_plies, seed)
    mode = float_mode()
    out = []
    for i in range(games):
        a_white = i % 2 == 0
        opening = openings[i // 2]
        g = start_game(opening)
        n0 = len(g)
        rng = np.random.default_rng([seed, i]) if noise else None
        while g.get_result() is None and len(g) - n0 < max_plies:
            agent = agents[g.turn == a_white]
            if sims > 0:
                r = mcts_oracle.search(g, agent, sims, noise=noise, mode=mode, rng=rng)
                mv = r.child_moves[r.chosen]
            else:
                mv = agent.best_move(g, real_game=True)
            assert g.move(mv), mv
        out.append(dict(a_white=a_white, opening=opening if isinstance(opening, str) else list(opening),
                        moves=[str(m) for m in g.board.move_stack][n0:], result=g.get_result()))
    res = tally([x["a_white"] for x in out], [x["result"] for x in out])
    res["games"] = out
    return res


@functools.lru_cache(maxsize=None)
def reference(name, swap=False, same=False, **kw):
    """The CPU arena of a named set, played once per process and shared: "random" / "fen", with keyword overrides;
    ``swap``: B against A; ``same``: A against A."""
    a, b = nets()
    if swap:
        a, b = b, a
    if same:
        b = a
    args = dict(RANDOM_SET if name == "random" else FEN_SET)
    args.update(kw)
    if "openings" in args:
        args["openings"] = list(args["openings"])
    return play(a, b, **args)
