#!/usr/bin/env python
"""What a search step costs with the built-in opponent's reply inside it (csrc/opponent.hpp k_reply_opponent): ms per
step of the default engine (the net's reply: two tower calls) and of ``reply=MinimaxPlayer`` at depths 1 and 2 (one
tower call + the alpha-beta search), over the same games and weights in one process.

    python tools/reply_probe.py [--games 4096] [--opening-plies 6] [--towers 10x128:f16] [--depths 1,2]
                                [--steps 32] [--windows 3] [--out profiles/reply_probe.json]
                                [--budget 150,300,600 [--max-depth 3] [--ordering]]

Every slot first plays --opening-plies random plies (the in-slot playout call, seeded words: the same games in every
engine).  All engines live side by side; after ``search_begin`` and 8 warm-up steps each (graphs captured before),
the timed windows alternate between them: a window is ``run_steps(--steps)`` between two synchronisations, host
clock; the median window is reported.  The trees grow alike in all engines, so window k compares like with like.
Then one more step with cleared accumulators gives the nodes per reply (mean / max over the slots that needed one)
and the cuts; the accumulators over the whole run give the mean per slot and step.  --budget B[,B..] adds one engine
per node budget, ``reply=MinimaxPlayer(search_depth=--max-depth, node_budget=B)`` (iterative deepening: the
k_reply_opponent_id kernel template), with the histogram of the completed depths of the last step's replies; such a run is stored as the
block "node_budget" of the output file, whose other content stays.  --ordering adds, next to every budgeted engine,
the same engine with ``ordering=True`` (its ORD instantiation), so every budget runs with ordering off and on in the same
process; such a run is stored as the block "ordering".  No threshold: a measurement.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--opening-plies", type=int, default=6)
    ap.add_argument("--towers", default="10x128:f16", help="comma list of BLOCKSxFILTERS:precision")
    ap.add_argument("--depths", default="1,2")
    ap.add_argument("--steps", type=int, default=32, help="steps per timed window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--budget", default="", help="node budgets of the iterative-deepening engines (default: none)")
    ap.add_argument("--max-depth", type=int, default=3, help="maximum depth of the --budget engines")
    ap.add_argument("--ordering", action="store_true", help="every --budget engine with ordering off and on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reply_probe.json"))
    args = ap.parse_args()
    budgets = [int(b) for b in args.budget.split(",") if b]
    import numpy as np
    import torch
    from chessrl_amd import _lib
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.gen_data import opening_words
    from chessrl_amd.model import ChessModel
    from chessrl_amd.opponent import MinimaxPlayer
    G, steps = args.games, args.steps
    sims = WARM + args.windows * steps + 1
    words = opening_words(random.Random(1), G, args.opening_plies)
    out = {"games": G, "opening_plies": args.opening_plies, "steps_per_window": steps, "windows": args.windows,
           "warm_up_steps": WARM, "node_limit": _lib.OPP_NODE_LIMIT, "towers": {}}
    for spec in args.towers.split(","):
        size, precision = spec.split(":")
        blocks, filters = (int(x) for x in size.split("x"))
        model = ChessModel(blocks=blocks, filters=filters, seed=1, precision=precision)
        engines = {"net reply": LockstepEngine(model, G, sims)}
        for depth in (int(x) for x in args.depths.split(",")):
            engines["depth %d" % depth] = LockstepEngine(model, G, sims, reply=MinimaxPlayer(False, search_depth=depth))
        for b in budgets:
            engines["depth <= %d within %d" % (args.max_depth, b)] = LockstepEngine(
                model, G, sims, reply=MinimaxPlayer(False, search_depth=args.max_depth, node_budget=b))
            if args.ordering:
                engines["depth <= %d within %d, ordered" % (args.max_depth, b)] = LockstepEngine(
                    model, G, sims, reply=MinimaxPlayer(False, search_depth=args.max_depth, node_budget=b, ordering=True))
        for eng in engines.values():
            eng.ctx.rollout_games(words, np.full(G, words.shape[1], np.int32), 1, args.opening_plies)
            eng.search_begin()
            eng.prepare_graphs(steps)
            eng.run_steps(WARM)
            eng.ctx.sync()
        running = int((engines["net reply"].ctx.results() == _lib.RESULT_NONE).sum())
        times = {k: [] for k in engines}
        for _ in range(args.windows):
            for k, eng in engines.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.run_steps(steps)
                eng.ctx.sync()
                times[k].append(time.perf_counter() - t0)
        rows = {}
        for k, eng in engines.items():
            ms = 1e3 * statistics.median(times[k]) / steps
            rows[k] = {"ms_per_step": ms, "window_seconds": times[k], "phases": [p for _, p in eng._plan],
                       "sims_per_s": G / ms * 1e3}
            if eng.reply is not None:
                done = WARM + args.windows * steps
                nodes, cuts = eng.reply_stats()[:2]
                rows[k]["nodes_per_slot_and_step_mean"] = float(nodes.sum()) / (G * done)
                rows[k]["cuts"] = int(cuts.sum())
                eng.reply_nodes.zero_()
                eng.reply_cuts.zero_()
                budgeted = eng.reply.node_budget is not None
                if budgeted:
                    rows[k]["depth_done_per_slot_and_step_mean"] = float(eng.reply_stats()[2].sum()) / (G * done)
                    eng.reply_depth_sum.zero_()
                eng.run_steps(1)
                eng.ctx.sync()
                stats = eng.reply_stats()
                nodes, cuts = stats[:2]
                replied = nodes > 0
                rows[k]["last_step"] = {"replies": int(replied.sum()), "nodes_per_reply_mean": float(nodes[replied].mean()),
                                        "nodes_per_reply_max": int(nodes.max()), "cuts": int(cuts.sum())}
                if budgeted:                     # one reply per slot in this step: the sum is that reply's depth
                    rows[k]["last_step"]["depth_done_histogram"] = np.bincount(
                        stats[2][replied], minlength=eng.reply.search_depth + 1).tolist()
            print(spec, k, json.dumps(rows[k]), flush=True)
            eng.close()
        out["towers"][spec] = {"precision": str(getattr(model, "precision", precision)), "running_games": running,
                               "engines": rows}
    if budgets:                                  # an added block: what the file holds stays
        kept = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                kept = json.load(f)
        kept["ordering" if args.ordering else "node_budget"] = dict(out, budgets=budgets, max_depth=args.max_depth)
        out = kept
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
