"""Supervised data from games of the built-in opponent against itself -- host mirror of the reference's
``gen_data_stockfish.py``.

/root/reference/src/chessrl/gen_data_stockfish.py:12-52 lets a Stockfish of ``player_depth`` play a
``GameStockfish`` whose engine has ``game_depth`` and appends the finished game to a ``DatasetGame``.  Here both
sides are the built-in alpha-beta player (csrc/opponent.hpp; NOT Stockfish), every game is one slot of ONE device
context and all games advance together: one ``opponent_moves(depths, push=True)`` launch per ply with the per-slot
depth of the side to move.  That player is deterministic, so every game first plays ``opening_plies`` random plies
with the in-slot playout call (``Context.rollout_games``, words from ``random.Random(seed)``).

The player sees a repetition below the root only on request (``repetition=True`` / ``--repetition``, with a node
budget; csrc/opponent.hpp, REPETITION): without it a large share of the games are draws in which the side that is ahead
shuffles until the fifth occurrence.  ``evaluation="positional"`` / ``--eval positional`` (with a node budget;
csrc/opponent.hpp, EVALUATION) gives both sides the positional static evaluation instead of material and centrality.
``selective=True`` / ``--selective`` (with ordering; csrc/opponent.hpp, SELECTIVE) gives both sides null-move pruning
and late-move reductions.  ``exchange=True`` / ``--exchange`` (with ordering and quiescence; csrc/opponent.hpp, EXCHANGE)
gives both sides delta and exchange pruning in quiescence.
"""
import argparse
import logging
import random
from datetime import datetime

import numpy as np

from . import _lib
from .dataset import DatasetGame
from .opponent import clamp_depth
from .records import GameRecord

log = logging.getLogger("chessrl_amd.gen_data")
WORDS_PER_PLY = 8         # words handed to a slot per opening ply and call (a choice rejects a word with p < 1/2)


def draw_games(num_games, depth=1, random_dep=False, seed=0):
    """Per game, in game order, from ``np.random.RandomState(seed)``: (is_white, game_depth, player_depth) as
    gen_data_stockfish.py:13-19 draws them -- ``random() <= .5``, then with ``random_dep`` two
    ``int(normal(depth, 1))`` -- the depths clamped to [1, CRL_OPP_MAX_DEPTH]."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(num_games):
        is_white = True if rs.random_sample() <= .5 else False
        game_depth = player_depth = depth
        if random_dep:
            game_depth = int(rs.normal(depth, 1))
            player_depth = int(rs.normal(depth, 1))
        out.append((is_white, clamp_depth(game_depth), clamp_depth(player_depth)))
    return out


def opening_words(rng, num_games, opening_plies):
    """The next block of opening words: uint32 [num_games][WORDS_PER_PLY * opening_plies], row by row from
    ``rng.getrandbits(32)``."""
    n = WORDS_PER_PLY * opening_plies
    rows = [[rng.getrandbits(32) for _ in range(n)] for _ in range(num_games)]
    return np.array(rows, dtype=np.uint32).reshape(num_games, n)


def side_depths(draws, white_to_move):
    """Depth of the side to move per game: the player (colour ``is_white``) has ``player_depth``, the other side
    ``game_depth``."""
    return np.array([pd if is_white == white_to_move else gd for is_white, gd, pd in draws], dtype=np.int32)


def gen_data(save_path, num_games=100, depth=1, random_dep=False, opening_plies=4, seed=0, workers=2, max_plies=512,
             quiescence=0, node_budget=None, ordering=False, repetition=False, evaluation="material",
             selective=False, exchange=False):
    """Plays ``num_games`` games, saves the finished ones to ``save_path`` (appending to what the file holds, as
    ``DatasetGame.save`` does) and returns the ``DatasetGame`` it saved.  The reference's ``gen_data`` forgets to
    pass ``depth`` and ``random_dep`` on to ``play_game`` (gen_data_stockfish.py:44-49); here both are honoured.
    ``workers`` is accepted and ignored; a game still running after ``max_plies`` plies is dropped.  ``quiescence``:
    the quiescence plies of both sides past their depths (0 .. CRL_OPP_MAX_QUIESCENCE; 0: none).  ``node_budget``
    (None: none): both sides deepen iteratively up to their depths and stop at that many nodes per move; ``ordering``
    (needs a ``node_budget``): with the move ORDERING of csrc/opponent.hpp; ``repetition`` (needs a ``node_budget``):
    with its REPETITION rule, both sides score a position below the root that occurred before a draw; ``evaluation``
    ("positional" needs a ``node_budget``): both sides search with its EVALUATION; ``selective`` (needs ``ordering``):
    both sides search with its SELECTIVE rules; ``exchange`` (needs ``ordering`` and ``quiescence`` >= 1): both sides
    search with its EXCHANGE rules."""
    opts = _lib.OpponentOptions(quiescence, node_budget, ordering, repetition, evaluation, selective, exchange)
    num_games, opening_plies, max_plies = int(num_games), int(opening_plies), int(max_plies)
    d = DatasetGame()
    if num_games < 1:
        d.save(save_path)
        return d
    draws = draw_games(num_games, depth, random_dep, seed)
    rng = random.Random(seed)
    ctx = _lib.Context(num_games, 1, max_plies=max(max_plies, opening_plies, 2))
    try:
        if opening_plies > 0:
            played = np.zeros(num_games, np.int32)
            while True:
                words = opening_words(rng, num_games, opening_plies)
                played, _, res = ctx.rollout_games(words, np.full(num_games, words.shape[1], np.int32), 1,
                                                   opening_plies, played=played)
                if ((played >= opening_plies) | (res[:, 0] != _lib.RESULT_NONE)).all():
                    break
        _, plies, results = ctx.records(with_moves=False)
        for ply in range(opening_plies, max_plies):
            running = results == _lib.RESULT_NONE
            if not running.any():
                break
            ctx.opponent_moves(np.where(running, side_depths(draws, ply % 2 == 0), 0), push=True, **opts.kwargs)
            results = ctx.results()
        moves, plies, results = ctx.records()
    finally:
        ctx.close()
    date = datetime.now().strftime("%d/%m/%Y %H:%M:%S")
    for i in range(num_games):
        if results[i] != _lib.RESULT_NONE:
            d.append(GameRecord(i, moves[i, :plies[i]], int(results[i]), draws[i][0], date=date))
    log.info("Saving dataset...")
    d.save(save_path)
    return d


def main(argv=None):
    p = argparse.ArgumentParser(description="Plays some chess games of the built-in opponent against itself and "
                                            "stores them as a dataset.")
    p.add_argument("data_path", metavar="datadir", help="Path of .JSON dataset.")
    p.add_argument("--games", metavar="games", type=int, default=10)
    p.add_argument("--depth", metavar="depth", type=int, default=1, help="Search depth of the built-in opponent.")
    p.add_argument("--quiescence", type=int, default=0,
                   help="Quiescence plies of the built-in opponent past its depth, both sides (0-6; 0: none).")
    p.add_argument("--nodes", type=int, default=None,
                   help="Node budget per move, both sides: iterative deepening up to the depth (default: none).")
    p.add_argument("--ordering", action="store_true", default=False,
                   help="Order the moves of the --nodes search by victim and killer moves, both sides.")
    p.add_argument("--repetition", action="store_true", default=False,
                   help="The --nodes search scores a position below the root that occurred before a draw, both sides.")
    p.add_argument("--eval", dest="evaluation", choices=sorted(_lib.OPP_EVALUATIONS), default="material",
                   help="Static evaluation of the --nodes search, both sides (positional needs --nodes).")
    p.add_argument("--selective", action="store_true", default=False,
                   help="Null-move pruning and late-move reductions in the --ordering search, both sides.")
    p.add_argument("--exchange", action="store_true", default=False,
                   help="Delta and exchange pruning in the quiescence of the --ordering search, both sides.")
    p.add_argument("--random_depth", action="store_true", default=False,
                   help="Use normal distribution of depths with mean --depth.")
    p.add_argument("--debug", action="store_true", default=False, help="Log debug messages on screen. Default false.")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--opening-plies", type=int, default=4)
    a = p.parse_args(argv)
    logging.basicConfig(level=logging.DEBUG if a.debug else logging.INFO)
    gen_data(a.data_path, num_games=a.games, depth=a.depth, random_dep=a.random_depth,
             opening_plies=a.opening_plies, seed=a.seed, quiescence=a.quiescence,
             node_budget=a.nodes, ordering=a.ordering, repetition=a.repetition, evaluation=a.evaluation,
             selective=a.selective, exchange=a.exchange)


if __name__ == "__main__":
    main()
