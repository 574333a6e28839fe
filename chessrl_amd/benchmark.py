"""Benchmark of a weight set against the built-in opponent -- host mirror of the reference's ``benchmark.py``.

/root/reference/src/chessrl/benchmark.py:59-143 plays N games of ``Agent.best_move(real_game=True)`` against a
Stockfish of chosen depth, one process per game, and tallies played / won / drawn.  Here the fixed yardstick is the
built-in depth-d alpha-beta player (csrc/opponent.hpp): NOT Stockfish, no Elo -- the summary reads "against the
built-in depth-d opponent".  All games sit in ONE device context and advance together: on the agent's plies one
tower call for the slots where the agent is to move and ``greedy_moves(policy, mask, push=True)``
(agentdistributed.py:56-58), on the opponent's plies one ``opponent_moves(depths, push=True)`` launch.

``benchmark(..., sims=N)`` (``--sims N``) measures the SEARCHING agent: one ``LockstepEngine(reply=MinimaxPlayer)``
whose trees hold the built-in opponent's replies (csrc/opponent.hpp ``k_reply_opponent``).  The engine's two-ply step
fits exactly: the reply stored for our move is the move the opponent plays from that board, so ``advance`` pushes (our
move, the opponent's real reply) and every game is a real game against the opponent.  Games in which the agent is
black first get the opponent's opening move (gamestockfish.py:31-33); then per move ``search(N)``, ``root_children``,
``choose_children(noise=False)``, ``advance``.  ``sims=0`` is the greedy benchmark above.

The opponent sees a repetition below the root only on request: ``opponent_repetition=True`` / ``--repetition`` (needs a
budget; csrc/opponent.hpp, REPETITION).  Without it, games it is winning may still end as draws by the fifth occurrence.
Its static evaluation is material and centrality unless ``opponent_evaluation="positional"`` / ``--eval positional``
(needs a budget; csrc/opponent.hpp, EVALUATION) asks for the positional one.  ``opponent_selective=True`` /
``--selective`` (needs ordering; csrc/opponent.hpp, SELECTIVE) adds null-move pruning and late-move reductions.
``opponent_exchange=True`` / ``--exchange`` (needs ordering and quiescence; csrc/opponent.hpp, EXCHANGE) adds delta and
exchange pruning at the quiescence nodes that stand pat.
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


def _play_greedy(model, dev, games, opponent_depth, max_plies, agent_white, opts=_lib.OpponentOptions()):
    """(moves, plies, results) of the games with ``Agent.best_move(real_game=True)`` on the agent's plies; ``opts``:
    the opponent's ``OpponentOptions``."""
    import torch
    ctx = _lib.Context(games, 1, max_plies=max(max_plies, 2), device=dev.index or 0)
    try:
        planes = torch.zeros((games, 8, 8, _lib.PLANES), dtype=torch.float16, device=dev)
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
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
                ctx.opponent_moves(np.where(opp_turn, int(opponent_depth), 0), push=True, **opts.kwargs)
            results = ctx.results()
        return ctx.records()
    finally:
        ctx.close()


def _play_search(model, dev, games, opponent_depth, max_plies, agent_white, sims, opts=_lib.OpponentOptions()):
    """(moves, plies, results) of the games with ``sims`` simulations per move against the opponent's replies.  A game
    is searched while it runs and has fewer than ``max_plies`` plies; a move adds two plies (one if it ends the game),
    so a game may end one ply past ``max_plies``."""
    from .engine import LockstepEngine, choose_children
    from .opponent import MinimaxPlayer
    eng = LockstepEngine(model, games, sims, device=dev.index or 0, max_plies=max_plies + 2,
                         reply=MinimaxPlayer(False, search_depth=opponent_depth, **opts.kwargs))
    try:
        ctx = eng.ctx
        if not agent_white.all():                            # gamestockfish.py:31-33: the opponent opens as white
            ctx.opponent_moves(np.where(agent_white, 0, int(opponent_depth)), push=True, **opts.kwargs)
        while True:
            _, plies, results = ctx.records(with_moves=False)
            live = (results == _lib.RESULT_NONE) & (plies < max_plies)
            if not live.any():
                break
            eng.search(sims)
            rc = eng.root_children()
            chosen = choose_children(rc["visits"], rc["nchild"], rc["root_visits"], plies, noise=False)
            chosen[~live] = -1
            eng.advance(chosen)
        return ctx.records()
    finally:
        eng.close()


def benchmark(model_dir, workers=1, games=10, opponent_depth=2, log=False, seed=None, max_plies=512, model=None,
              sims=0, opponent_quiescence=0, opponent_budget=None, opponent_ordering=False,
              opponent_repetition=False, opponent_evaluation="material", opponent_selective=False,
              opponent_exchange=False):
    """Plays ``games`` games against the built-in depth-``opponent_depth`` opponent (with ``opponent_quiescence``
    plies of quiescence search, 0 by default) and returns
    ``dict(played=, won=, drawn=, games=)``: the reference's tallies and the per-game UCI move lists.  ``workers`` is
    accepted and ignored (the games run in lockstep on one GPU); ``model`` takes a ready evaluator (planes ->
    (policy, value) on the GPU) instead of the newest weights of ``model_dir``.  A game still running after
    ``max_plies`` plies counts as played, neither won nor drawn.  ``sims`` > 0: the agent's move is the choice of an
    MCTS of ``sims`` simulations against the opponent's replies instead of its greedy move (module docstring).
    ``opponent_budget`` (None: none): the opponent deepens iteratively up to ``opponent_depth`` and stops at that many
    nodes per move (csrc/opponent.hpp, ITERATIVE DEEPENING); ``opponent_ordering`` (needs ``opponent_budget``): with
    the move ORDERING of that header; ``opponent_repetition`` (needs ``opponent_budget``): with its REPETITION rule, a
    position below the root that occurred before is a draw to the opponent's search; ``opponent_evaluation``
    ("positional" needs ``opponent_budget``): with its EVALUATION in place of the material evaluation;
    ``opponent_selective`` (needs ``opponent_ordering``): with its SELECTIVE rules, null-move pruning and late-move
    reductions; ``opponent_exchange`` (needs ``opponent_ordering`` and ``opponent_quiescence`` >= 1): with its EXCHANGE
    rules, delta and exchange pruning in quiescence."""
    if not 1 <= int(opponent_depth) <= _lib.OPP_MAX_DEPTH:
        raise ValueError("opponent_depth must lie in [1, %d]" % _lib.OPP_MAX_DEPTH)
    quiescence = int(opponent_quiescence)
    if not 0 <= quiescence <= _lib.OPP_MAX_QUIESCENCE:
        raise ValueError("opponent_quiescence must lie in [0, %d]" % _lib.OPP_MAX_QUIESCENCE)
    budget = None if opponent_budget is None else int(opponent_budget)
    if budget is not None and budget < 1:
        raise ValueError("opponent_budget must be None or at least 1")
    if opponent_ordering and budget is None:
        raise ValueError("opponent_ordering needs an opponent_budget")
    opts = _lib.OpponentOptions(quiescence, budget, opponent_ordering, opponent_repetition, opponent_evaluation,
                                opponent_selective, opponent_exchange)
    sims = int(sims)
    if sims < 0:
        raise ValueError("sims must be 0 (the greedy agent) or the number of simulations per move")
    import torch
    games, max_plies = int(games), int(max_plies)
    colors = game_colors(games, seed)
    if games < 1:
        return dict(tally([], []), games=[])
    if model is None:
        model = _load_model(model_dir)
    dev = getattr(model, "device", None) or torch.device("cuda", 0)
    dev = torch.device(dev)
    agent_white = np.array(colors, dtype=bool)
    if sims > 0:
        moves, plies, results = _play_search(model, dev, games, opponent_depth, max_plies, agent_white, sims, opts)
    else:
        moves, plies, results = _play_greedy(model, dev, games, opponent_depth, max_plies, agent_white, opts)
    res = [None if r == _lib.RESULT_NONE else int(r) for r in results]
    out = tally(colors, res)
    out["games"] = [[move_to_uci(m) for m in moves[i, :plies[i]]] for i in range(games)]
    if log:
        print("##################### SUMMARY ###################")
        if budget is None:
            print("Against the built-in depth-%d opponent%s (not Stockfish, no Elo)"
                  % (opponent_depth, ", quiescence %d" % quiescence if quiescence else ""))
        else:
            print("Against the built-in opponent, depth <= %d within %d nodes per move%s%s%s%s%s%s (not Stockfish, no Elo)"
                  % (opponent_depth, budget, ", ordered" if opts.ordering else "",
                     ", repetition-aware" if opts.repetition else "",
                     ", quiescence %d" % quiescence if quiescence else "",
                     ", positional evaluation" if opts.evaluation == "positional" else "",
                     ", selective" if opts.selective else "", ", exchange-pruned" if opts.exchange else ""))
        if sims > 0:
            print("agent: MCTS, %d simulations per move" % sims)
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
    p.add_argument("--quiescence", type=int, default=0,
                   help="quiescence plies of the built-in opponent past its depth (0-6; 0: none)")
    p.add_argument("--nodes", type=int, default=None,
                   help="node budget per move of the built-in opponent: iterative deepening up to --depth (default: "
                        "none, the fixed depth)")
    p.add_argument("--ordering", action="store_true",
                   help="order the moves of the --nodes search by victim and killer moves (needs --nodes)")
    p.add_argument("--repetition", action="store_true",
                   help="the --nodes search scores a position below the root that occurred before a draw (needs --nodes)")
    p.add_argument("--eval", dest="evaluation", choices=sorted(_lib.OPP_EVALUATIONS), default="material",
                   help="static evaluation of the --nodes search (positional needs --nodes)")
    p.add_argument("--selective", action="store_true",
                   help="null-move pruning and late-move reductions in the --ordering search (needs --ordering)")
    p.add_argument("--exchange", action="store_true",
                   help="delta and exchange pruning in the quiescence of the --ordering search (needs --ordering and "
                        "--quiescence)")
    p.add_argument("--seed", type=int, default=None, help="seed of the colour draw")
    p.add_argument("--max-plies", type=int, default=512)
    p.add_argument("--sims", type=int, default=0,
                   help="simulations per move of the agent's search against the opponent's replies (0: the greedy agent)")
    a = p.parse_args(argv)
    benchmark(a.model_dir, games=a.games, opponent_depth=a.depth, seed=a.seed, max_plies=a.max_plies, log=True,
              sims=a.sims, opponent_quiescence=a.quiescence, opponent_budget=a.nodes, opponent_ordering=a.ordering,
              opponent_repetition=a.repetition, opponent_evaluation=a.evaluation, opponent_selective=a.selective,
              opponent_exchange=a.exchange)


if __name__ == "__main__":
    main()
