"""Benchmark of a weight set against the built-in opponent -- host mirror of the reference's ``benchmark.py``.

/root/reference/src/chessrl/benchmark.py:59-143 plays N games of ``Agent.best_move(real_game=True)`` against a
Stockfish of chosen depth, one process per game, and tallies played / won / drawn.  Here the fixed yardstick is the
built-in depth-d alpha-beta player (csrc/opponent.hpp): NOT Stockfish, no Elo -- the summary reads "against the
built-in depth-d opponent".  All games sit in ONE device context and advance together: on the agent's plies one
tower call for the slots where the agent is to move and ``greedy_moves(policy, mask, push=True)``
(agentdistributed.py:56-58), on the opponent's plies one ``opponent_moves(depths, push=True)`` launch.
MCTS on the agent's side is out of scope: the lockstep search engine advances two plies per search.
"""
import argparse
import os
import random

import numpy as np

from . import _lib
from .game import move_to_uci


def tally(colors, results):
    """The reference's summary (benchmark.py:130-143) of per-game (agent is white, result for white or None)."""
    won = sum(1 for c, r in zip(colors, results) if (c is True and r == 1) or (c is False and r == -1))
    return dict(played=len(colors), won=won, drawn=sum(1 for r in results if r == 0))


def game_colors(games, seed=None):
    """``random.random() <= .5`` per game (benchmark.py:70) from ``random.Random(seed)``, in game order."""
    rng = random.Random(seed)
    return [True if rng.random() <= .5 else False for _ in range(games)]


def _load_model(model_dir):
    from .model import ChessModel
    from .selfplay import get_model_path
    path = get_model_path(model_dir)
    return ChessModel(weights=path if os.path.exists(path) else None)


def benchmark(model_dir, workers=1, games=10, opponent_depth=2, log=False, seed=None, max_plies=512, model=None):
    """Plays ``games`` games against the built-in depth-``opponent_depth`` opponent and returns
    ``dict(played=, won=, drawn=, games=)``: the reference's tallies and the per-game UCI move lists.  ``workers`` is
    accepted and ignored (the games run in lockstep on one GPU); ``model`` takes a ready evaluator (planes ->
    (policy, value) on the GPU) instead of the newest weights of ``model_dir``.  A game still running after
    ``max_plies`` plies counts as played, neither won nor drawn."""
    import torch
    if not 1 <= int(opponent_depth) <= _lib.OPP_MAX_DEPTH:
        raise ValueError("opponent_depth must lie in [1, %d]" % _lib.OPP_MAX_DEPTH)
    games, max_plies = int(games), int(max_plies)
    colors = game_colors(games, seed)
    if games < 1:
        return dict(tally([], []), games=[])
    if model is None:
        model = _load_model(model_dir)
    dev = getattr(model, "device", None) or torch.device("cuda", 0)
    dev = torch.device(dev)
    ctx = _lib.Context(games, 1, max_plies=max(max_plies, 2), device=dev.index or 0)
    try:
        planes = torch.zeros((games, 8, 8, _lib.PLANES), dtype=torch.float16, device=dev)
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        agent_white = np.array(colors, dtype=bool)
        results = ctx.results()
        for ply in range(max_plies):
            running = results == _lib.RESULT_NONE
            if not running.any():
                break
            white_to_move = ply % 2 == 0                     # every game starts from the standard position
            agent_turn = running & (agent_white == white_to_move)
            opp_turn = running & ~agent_turn
            if agent_turn.any():
                ctx.encode(planes.data_ptr())
                policy = model(planes)[0].float().contiguous()
                ctx.greedy_moves(policy.data_ptr(), mask=agent_turn, push=True, want_moves=False)
            if opp_turn.any():
                ctx.opponent_moves(np.where(opp_turn, int(opponent_depth), 0), push=True)
            results = ctx.results()
        moves, plies, results = ctx.records()
    finally:
        ctx.close()
    res = [None if r == _lib.RESULT_NONE else int(r) for r in results]
    out = tally(colors, res)
    out["games"] = [[move_to_uci(m) for m in moves[i, :plies[i]]] for i in range(games)]
    if log:
        print("##################### SUMMARY ###################")
        print("Against the built-in depth-%d opponent (not Stockfish, no Elo)" % opponent_depth)
        print("Games played: %d" % out["played"])
        print("Games won: %d" % out["won"])
        print("Games drawn: %d" % out["drawn"])
        print("#################################################")
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description="Plays games of the newest weights of a model directory against the "
                                            "built-in depth-d alpha-beta opponent and prints the summary.")
    p.add_argument("model_dir", help="directory of the model-<v>.npz / .h5 weight files")
    p.add_argument("--games", type=int, default=10)
    p.add_argument("--depth", type=int, default=2, help="search depth of the built-in opponent (1-5)")
    p.add_argument("--seed", type=int, default=None, help="seed of the colour draw")
    p.add_argument("--max-plies", type=int, default=512)
    a = p.parse_args(argv)
    benchmark(a.model_dir, games=a.games, opponent_depth=a.depth, seed=a.seed, max_plies=a.max_plies, log=True)


if __name__ == "__main__":
    main()
