#!/usr/bin/env python
"""Two settings of the built-in opponent (csrc/opponent.hpp) play each other over paired openings.

    python tools/opponent_match.py [--pairs 512] [--depth 3] [--budget 600] [--quiescence 2] [--ordering] [--repetition]
                                   [--eval-a positional] [--eval-b material] [--selective] [--exchange]
                                   [--opening-plies 6] [--max-plies 300] [--seed 0]
                                   [--out profiles/opponent_match.json]

Games 2i and 2i + 1 share --opening-plies random plies (the in-slot playout call; the words come from
``chessrl_amd.gen_data.opening_words``, the source ``gen_data`` draws them from); setting A is white in game 2i and
black in game 2i + 1.  All games advance in lockstep: per ply two ``opponent_moves(push=True)`` launches under
complementary depth masks -- depth 0 leaves a slot alone -- so each side is searched with its own settings.  --depth,
--budget, --quiescence, --ordering and --repetition hold for both sides; the sides differ in their evaluation and,
with --selective (it needs --ordering), in that A searches with the SELECTIVE rules of opponent.hpp and B without: give
both sides the same evaluation to measure the rules alone.  With --exchange (it needs --ordering and --quiescence >= 1)
A searches with the EXCHANGE rules of opponent.hpp and B without, everything else equal when both sides get the same
evaluation; a node of A is dearer in time, the match is at equal nodes.

Printed and written: wins, draws and losses of A, its score (a game still running at --max-plies counts as a draw)
with a 95 % interval over the pair scores, the games still running and their share, and how every game ended (the
moves are replayed on the CPU oracle).  A score over paired openings at equal nodes per move: no Elo claim.
"""
import argparse
import json
import math
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENDINGS = ("mate", "stalemate", "fifth_occurrence", "seventy_five_move_rule", "fifty_move_claim",
           "insufficient_material", "running")


def side_kw(settings):
    """The keywords of ``Context.opponent_moves`` of one side's settings (without its depth)."""
    from chessrl_amd import _lib
    return _lib.OpponentOptions(**{k: v for k, v in settings.items() if k != "depth"}).kwargs


def play(pairs, a, b, opening_plies=6, max_plies=300, seed=0):
    """Plays 2 * ``pairs`` games between the settings ``a`` and ``b`` (dicts: depth, node_budget, quiescence, ordering,
    repetition, evaluation, selective, exchange) and returns (a_white bool [G], moves u16 [G][plies], plies, results): A is white in the
    even games."""
    import numpy as np
    from chessrl_amd import _lib
    from chessrl_amd.gen_data import opening_words
    G = 2 * int(pairs)
    a_white = np.arange(G) % 2 == 0
    rng = random.Random(seed)
    ctx = _lib.Context(G, 1, max_plies=max(max_plies, opening_plies, 2))
    try:
        if opening_plies > 0:
            played = np.zeros(G, np.int32)
            while True:                                          # (more words where a slot rejected too many)
                words = np.repeat(opening_words(rng, pairs, opening_plies), 2, axis=0)
                played, _, res = ctx.rollout_games(words, np.full(G, words.shape[1], np.int32), 1, opening_plies,
                                                   played=played)
                if ((played >= opening_plies) | (res[:, 0] != _lib.RESULT_NONE)).all():
                    break
        results = ctx.results()
        for ply in range(opening_plies, max_plies):
            running = results == _lib.RESULT_NONE
            if not running.any():
                break
            a_turn = running & (a_white == (ply % 2 == 0))       # both masks before either launch
            b_turn = running & ~a_turn
            if a_turn.any():
                ctx.opponent_moves(np.where(a_turn, int(a["depth"]), 0), push=True, **side_kw(a))
            if b_turn.any():
                ctx.opponent_moves(np.where(b_turn, int(b["depth"]), 0), push=True, **side_kw(b))
            results = ctx.results()
        moves, plies, results = ctx.records()
    finally:
        ctx.close()
    return a_white, moves, plies, results


def ending(game):
    """How a replayed game ended, in the order ``position_result`` decides it."""
    from oracle.chess_oracle import lib as oracle_lib
    result = game.get_result()
    if result is None:
        return "running"
    if result != 0:
        return "mate"
    clock = (int(game.board_at(0).state) >> 12) & 255
    legal = len(game.legal_move_ids())
    if clock >= 100 and legal > 0:
        return "fifty_move_claim"
    if legal == 0:
        return "stalemate"
    if oracle_lib().og_insufficient(game._h):
        return "insufficient_material"
    if game.repetitions() >= 5:
        return "fifth_occurrence"
    return "seventy_five_move_rule"


def summary(a_white, moves, plies, results):
    """The figures of a match from A's side.  A game still running counts as a draw."""
    from chessrl_amd import _lib
    from chessrl_amd.game import move_to_uci
    from oracle.chess_oracle import OracleGame
    G = len(a_white)
    points, endings, games = [], dict.fromkeys(ENDINGS, 0), []
    won = drawn = lost = running = 0
    for i in range(G):
        uci = [move_to_uci(m) for m in moves[i, :plies[i]]]
        g = OracleGame()
        for u in uci:
            assert g.move(u), (i, u)
        r = None if results[i] == _lib.RESULT_NONE else int(results[i])
        assert g.get_result() == r, i
        endings[ending(g)] += 1
        games.append(uci)
        if r is None:
            running += 1
        if r is None or r == 0:
            drawn += 1
            points.append(0.5)
        elif (r == 1) == bool(a_white[i]):
            won += 1
            points.append(1.0)
        else:
            lost += 1
            points.append(0.0)
    pair = [(points[2 * i] + points[2 * i + 1]) / 2 for i in range(G // 2)]
    mean = sum(pair) / len(pair)
    var = sum((p - mean) ** 2 for p in pair) / (len(pair) - 1) if len(pair) > 1 else 0.0
    half = 1.96 * math.sqrt(var / len(pair))
    return dict(games=G, pairs=G // 2, won=won, drawn=drawn, lost=lost, score=mean, score_95=[mean - half, mean + half],
                running_at_max_plies=running, running_share=running / G, endings=endings,
                mean_plies=float(sum(int(p) for p in plies)) / G), games


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--budget", type=int, default=600)
    ap.add_argument("--quiescence", type=int, default=2)
    ap.add_argument("--ordering", action="store_true")
    ap.add_argument("--repetition", action="store_true")
    ap.add_argument("--eval-a", default="positional", choices=("material", "positional"))
    ap.add_argument("--eval-b", default="material", choices=("material", "positional"))
    ap.add_argument("--selective", action="store_true", help="A searches with the selective rules, B without")
    ap.add_argument("--exchange", action="store_true", help="A searches with delta and exchange pruning, B without")
    ap.add_argument("--opening-plies", type=int, default=6)
    ap.add_argument("--max-plies", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "opponent_match.json"))
    args = ap.parse_args(argv)
    if args.selective and not args.ordering:
        ap.error("--selective needs --ordering")
    if args.exchange and not (args.ordering and args.quiescence >= 1):
        ap.error("--exchange needs --ordering and --quiescence >= 1")
    common = dict(depth=args.depth, node_budget=args.budget, quiescence=args.quiescence, ordering=args.ordering,
                  repetition=args.repetition)
    # the sides differ in the last option named: with --exchange a --selective holds for both
    a = dict(common, evaluation=args.eval_a, selective=args.selective, exchange=args.exchange)
    b = dict(common, evaluation=args.eval_b, selective=args.selective and args.exchange)
    out, _ = summary(*play(args.pairs, a, b, args.opening_plies, args.max_plies, args.seed))
    out.update(a=a, b=b, opening_plies=args.opening_plies, max_plies=args.max_plies, seed=args.seed,
               note="a score over paired openings at equal nodes per move, no Elo claim")
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
