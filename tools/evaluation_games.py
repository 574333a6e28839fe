#!/usr/bin/env python
"""How the games of ``chessrl_amd.gen_data`` end with the built-in opponent's material evaluation and with its
positional EVALUATION (csrc/opponent.hpp): the same seed, so the same colours, depths and opening plies, the
REPETITION rule on in both (the settings of tools/repetition_games.py).

    python tools/evaluation_games.py [--games 256] [--depth 2] [--budget 2000] [--max-plies 200] [--seed 0]
                                     [--out profiles/evaluation_games.json]

Per evaluation: the games that finished within --max-plies and how they ended -- mates, stalemates, the fifth
occurrence of a position, the 75-move rule, the fifty-move claim, insufficient material (the moves are replayed on the
CPU oracle; the kinds are those of tools/opponent_match.py).  A count of game endings, not a strength figure: no Elo.
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--budget", type=int, default=2000)
    ap.add_argument("--max-plies", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluation_games.json"))
    args = ap.parse_args()
    from chessrl_amd import gen_data as gd
    from oracle.chess_oracle import OracleGame
    from opponent_match import ENDINGS, ending
    out = {}
    for evaluation in ("material", "positional"):
        with tempfile.TemporaryDirectory() as t:
            d = gd.gen_data(os.path.join(t, "games.json"), num_games=args.games, depth=args.depth,
                            node_budget=args.budget, repetition=True, evaluation=evaluation, opening_plies=4,
                            seed=args.seed, max_plies=args.max_plies)
        endings, plies, decisive = dict.fromkeys(ENDINGS, 0), [], 0
        for rec in d.games:
            h = rec.get_history()
            g = OracleGame()
            for u in h["moves"]:
                assert g.move(u), u
            assert g.get_result() == h["result"]
            plies.append(len(g))
            endings[ending(g)] += 1
            decisive += h["result"] != 0
        endings["running"] = args.games - len(d.games)                     # dropped by gen_data at --max-plies
        out[evaluation] = dict(games=args.games, depth=args.depth, node_budget=args.budget, repetition=True,
                               max_plies=args.max_plies, seed=args.seed, finished=len(d.games), decisive=decisive,
                               endings=endings, mean_plies=sum(plies) / max(len(plies), 1))
        print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
