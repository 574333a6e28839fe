#!/usr/bin/env python
"""How the games of ``chessrl_amd.gen_data`` end with the built-in opponent's REPETITION rule (csrc/opponent.hpp) off
and on: the same seed, so the same colours, depths and opening plies.

    python tools/repetition_games.py [--games 256] [--depth 2] [--budget 2000] [--max-plies 200] [--seed 0]
                                     [--out profiles/repetition_games.json]

Per setting: the games that finished within --max-plies, how many of them are decisive, how many are draws by the
fifth occurrence of a position (the moves are replayed on the CPU oracle, which counts the occurrences) and how many
are other draws.  A count of game endings, not a strength figure: no Elo.
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--budget", type=int, default=2000)
    ap.add_argument("--max-plies", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repetition_games.json"))
    args = ap.parse_args()
    from chessrl_amd import gen_data as gd
    from oracle.chess_oracle import OracleGame
    out = {}
    for rule in (False, True):
        with tempfile.TemporaryDirectory() as t:
            d = gd.gen_data(os.path.join(t, "games.json"), num_games=args.games, depth=args.depth,
                            node_budget=args.budget, repetition=rule, opening_plies=4, seed=args.seed,
                            max_plies=args.max_plies)
        fifth = decisive = other = 0
        plies = []
        for rec in d.games:
            h = rec.get_history()
            g = OracleGame()
            for u in h["moves"]:
                assert g.move(u), u
            assert g.get_result() == h["result"]
            plies.append(len(g))
            if h["result"] != 0:
                decisive += 1
            elif g.repetitions() >= 5:
                fifth += 1
            else:
                other += 1
        out["repetition_%s" % ("on" if rule else "off")] = dict(
            games=args.games, depth=args.depth, node_budget=args.budget, max_plies=args.max_plies, seed=args.seed,
            finished=len(d.games), decisive=decisive, fivefold=fifth, other_draws=other,
            mean_plies=sum(plies) / max(len(plies), 1))
        print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
