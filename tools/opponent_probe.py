#!/usr/bin/env python
"""Node rate of the built-in opponent (csrc/opponent.hpp): ms per launch, nodes per slot and nodes/s at depths 1, 2, 3.

    python tools/opponent_probe.py [--games 4096] [--opening-plies 6] [--node-limit 200000] [--out profiles/opponent_probe.json]
    python tools/opponent_probe.py --quiescence 2,4,6 --depths 1,2 --out profiles/opponent_probe_q.json
    python tools/opponent_probe.py --budget 150,300,600,1500 --depths 2,3 --max-depth 3
    python tools/opponent_probe.py --ordering --budget 150,300,600,1500 --depths 2,3 --max-depth 3 --quiescence 0,2
    python tools/opponent_probe.py --repetition --budget 150,300,600,1500 --depths 2,3 --max-depth 3 --quiescence 0,2 --opening-plies 40
    python tools/opponent_probe.py --eval positional --budget 150,300,600,1500 --depths 2,3 --max-depth 3 --quiescence 0,2
    python tools/opponent_probe.py --selective --ordering --budget 600,1500,6000 --max-depth 5 --quiescence 0,2
    python tools/opponent_probe.py --exchange --ordering --budget 600,3000 --max-depth 5 --quiescence 2,6
    python tools/opponent_probe.py --exchange --ordering --budget 600,3000 --max-depth 5 --quiescence 2,6 --exchange-counts 32

Every slot first plays --opening-plies random plies (the in-slot playout call, seeded words), so the slots hold
different positions.  Per depth, in depth order: one warm-up launch, then three timed ones (host wall time around the
synchronous call, copies included); the median is reported.  Nothing is pushed, so every launch searches the same
positions.  --quiescence Q[,Q..]: the same per quiescence (opponent.hpp QUIESCENCE), keyed "<depth>+q<Q>"; 0, the
default, is the fixed-depth search and leaves the output as it was.  --budget B[,B..]: after the fixed depths, on the
same games in the same process, iterative deepening up to --max-depth under each node budget (opponent.hpp ITERATIVE
DEEPENING), keyed "<=<depth>@<B>[+q<Q>]", with the histogram of the completed depths; the output then goes to
profiles/opponent_probe_id.json unless --out names another file.  --ordering: every budget is run with the move
ORDERING of opponent.hpp off and on in the same process, the launches alternating (warm-up off, warm-up on, then three
times off, on); the ordered rows are keyed "<=<depth>@<B>[+q<Q>] ordered" and the output goes to
profiles/opponent_probe_ord.json.  --repetition: likewise every budget is run with the REPETITION rule of opponent.hpp
off and on in the same process, the launches alternating; the rule-on rows are keyed "<=<depth>@<B>[+q<Q>] repeating-aware"
and carry the cost per node as a ratio to the rule-off row of the same run and the share of slots that play another
move; the output goes to profiles/opponent_probe_rep.json.  At --opening-plies 6 few slots have reversible plies behind
them; at 40 most do.  With --ordering as well, both rows of a budget are ordered.  --eval positional: every budget is
run with the material evaluation and with the positional EVALUATION of opponent.hpp in the same process, the launches
alternating; --ordering and --repetition then hold for both rows, the positional rows are keyed "... positional" and
carry the time per node and per launch as ratios to the material row of the same run and the share of slots that play
another move; the output goes to profiles/opponent_probe_eval.json.  --selective (with --ordering): every budget is
run with the SELECTIVE rules of opponent.hpp (null-move pruning, late-move reductions) off and on in the same process,
the launches alternating; --repetition and --eval then hold for both rows, the selective rows are keyed "... selective"
and carry the time per node and per launch as ratios to the full-width row of the same run, the mean completed depth of
both and the share of slots that play another move; the output goes to profiles/opponent_probe_sel.json.  --exchange
(with --ordering and quiescence plies): every budget is run with the EXCHANGE rules of opponent.hpp (delta and exchange
pruning at the stand-pat nodes) off and on in the same process, the launches alternating; --repetition, --eval and
--selective then hold for both rows, the pruned rows are keyed "... exchange-pruned" and carry the time per node and per
launch as ratios to the unpruned row of the same run, the mean completed depth of both and the share of slots that play
another move; the output goes to profiles/opponent_probe_exc.json.  The kernels do not count what the filter removes;
--exchange-counts N does, WITHOUT a GPU: the first N slots' positions are rebuilt on the CPU oracle from the same words,
searched by the restatement tests/exchange_util.py (which the GPU test holds equal to the kernels), and the moves
removed by each of the two tests per 1000 nodes are added to the pruned rows of the file already written.  No threshold:
this is a measurement.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--opening-plies", type=int, default=6)
    ap.add_argument("--node-limit", type=int, default=200000)
    ap.add_argument("--depths", default="1,2,3")
    ap.add_argument("--quiescence", default="0")
    ap.add_argument("--budget", default="", help="node budgets of the iterative-deepening launches (default: none)")
    ap.add_argument("--max-depth", type=int, default=3, help="maximum depth of the --budget launches")
    ap.add_argument("--ordering", action="store_true", help="run every --budget with ordering off and on, alternating")
    ap.add_argument("--repetition", action="store_true",
                    help="run every --budget with the repetition rule off and on, alternating")
    ap.add_argument("--eval", dest="evaluation", default="material", choices=("material", "positional"),
                    help="positional: run every --budget with the material and the positional evaluation, alternating")
    ap.add_argument("--selective", action="store_true",
                    help="run every --budget with the selective rules off and on, alternating (needs --ordering)")
    ap.add_argument("--exchange", action="store_true",
                    help="run every --budget with delta and exchange pruning off and on, alternating (needs --ordering "
                         "and --quiescence >= 1)")
    ap.add_argument("--exchange-counts", type=int, default=0, metavar="N",
                    help="no GPU: add the moves the two tests remove per 1000 nodes, counted by the CPU restatement "
                         "on the first N slots, to the pruned rows of --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    budgets = [int(b) for b in args.budget.split(",") if b]
    if args.selective and not args.ordering:
        ap.error("--selective needs --ordering")
    if args.exchange and not (args.ordering and all(int(q) >= 1 for q in args.quiescence.split(","))):
        ap.error("--exchange needs --ordering and --quiescence >= 1")
    if args.out is None:
        name = ("opponent_probe.json" if not budgets else
                "opponent_probe_exc.json" if args.exchange else
                "opponent_probe_sel.json" if args.selective else
                "opponent_probe_eval.json" if args.evaluation == "positional" else
                "opponent_probe_rep.json" if args.repetition else
                "opponent_probe_ord.json" if args.ordering else "opponent_probe_id.json")
        args.out = os.path.join(ROOT, "profiles", name)
    import numpy as np
    from chessrl_amd import _lib
    from chessrl_amd.gen_data import opening_words
    G = args.games
    if args.exchange_counts:
        return exchange_counts(args, budgets, opening_words(random.Random(1), G, args.opening_plies))
    ctx = _lib.Context(G, 1, max_plies=max(64, args.opening_plies + 2))
    words = opening_words(random.Random(1), G, args.opening_plies)
    played, _, _ = ctx.rollout_games(words, np.full(G, words.shape[1], np.int32), 1, args.opening_plies)
    out = {"games": G, "opening_plies": args.opening_plies, "mean_opening_plies": float(played.mean()),
           "node_limit": args.node_limit, "clock_at_least_4_share": float((((ctx.get_positions()[:, 7] >> 12) & 255) >= 4).mean()),
           "running": int((ctx.results() == _lib.RESULT_NONE).sum()), "depths": {}}
    cases = [(int(d), int(q), None) for q in args.quiescence.split(",") for d in args.depths.split(",")]
    cases += [(args.max_depth, int(q), b) for q in args.quiescence.split(",") for b in budgets]
    for depth, quiescence, budget in cases:
        row = np.full(G, depth, np.int32)
        key = (str(depth) if budget is None else "<=%d@%d" % (depth, budget)) + ("+q%d" % quiescence if quiescence else "")
        kw = {"quiescence": quiescence} if quiescence else {}
        if budget is not None:
            kw["node_budget"] = budget
        # the launches of a case alternate between its variants: ordering off and, with --ordering, on
        variants = [(key, kw)]
        if budget is not None and args.exchange:
            base = (key + " ordered" + (" repeating-aware" if args.repetition else "") +
                    (" positional" if args.evaluation == "positional" else "") +
                    (" selective" if args.selective else ""),
                    dict(kw, ordering=True, repetition=args.repetition, evaluation=args.evaluation,
                         selective=args.selective))
            variants = [base, (base[0] + " exchange-pruned", dict(base[1], exchange=True))]
        elif budget is not None and args.selective:
            base = (key + " ordered" + (" repeating-aware" if args.repetition else "") +
                    (" positional" if args.evaluation == "positional" else ""),
                    dict(kw, ordering=True, repetition=args.repetition, evaluation=args.evaluation))
            variants = [base, (base[0] + " selective", dict(base[1], selective=True))]
        elif budget is not None and args.evaluation == "positional":
            base = (key + (" ordered" if args.ordering else "") + (" repeating-aware" if args.repetition else ""),
                    dict(kw, ordering=args.ordering, repetition=args.repetition))
            variants = [base, (base[0] + " positional", dict(base[1], evaluation="positional"))]
        elif budget is not None and args.repetition:
            if args.ordering:
                variants = [(key + " ordered", dict(kw, ordering=True))]
            variants.append((variants[0][0] + " repeating-aware", dict(variants[0][1], repetition=True)))
        elif budget is not None and args.ordering:
            variants.append((key + " ordered", dict(kw, ordering=True)))
        variants = [(k, _lib.OpponentOptions(**vkw)) for k, vkw in variants]
        times = dict((k, []) for k, _ in variants)
        last = {}
        for i in range(4):
            for k, opts in variants:
                t0 = time.perf_counter()
                last[k] = ctx.opponent_moves(row, node_limit=args.node_limit, **opts.kwargs)
                if i:
                    times[k].append(time.perf_counter() - t0)
        for k, _ in variants:
            moves, scores, nodes, flags = last[k][:4]
            t = statistics.median(times[k])
            searched = flags != _lib.OPP_SKIPPED
            total = int(nodes.sum())
            out["depths"][k] = {
                "seconds": times[k], "ms_per_launch": 1e3 * t, "nodes": total,
                "nodes_per_slot_mean": float(nodes[searched].mean()),
                "nodes_per_slot_max": int(nodes.max()), "nodes_per_s": total / t, "us_per_node_of_the_longest_slot":
                1e6 * t / max(int(nodes.max()), 1), "cut_share": float((flags == _lib.OPP_CUT).mean())}
            if budget is not None:
                out["depths"][k]["depth_done_histogram"] = np.bincount(last[k][4][searched], minlength=depth + 1).tolist()
            print(k, json.dumps(out["depths"][k]), flush=True)
        if len(variants) == 2 and args.exchange:                       # against the unpruned row of this run
            off, on = out["depths"][variants[0][0]], out["depths"][variants[1][0]]
            on["time_per_node_ratio_to_unpruned"] = off["nodes_per_s"] / on["nodes_per_s"]
            on["ms_per_launch_ratio_to_unpruned"] = on["ms_per_launch"] / off["ms_per_launch"]
            on["share_of_slots_with_another_move"] = float((last[variants[0][0]][0] != last[variants[1][0]][0]).mean())
            for k, _ in variants:
                out["depths"][k]["depth_done_mean"] = float(last[k][4][last[k][3] != _lib.OPP_SKIPPED].mean())
        elif len(variants) == 2 and args.selective:                    # against the full-width row of this run
            off, on = out["depths"][variants[0][0]], out["depths"][variants[1][0]]
            on["time_per_node_ratio_to_full_width"] = off["nodes_per_s"] / on["nodes_per_s"]
            on["ms_per_launch_ratio_to_full_width"] = on["ms_per_launch"] / off["ms_per_launch"]
            on["share_of_slots_with_another_move"] = float((last[variants[0][0]][0] != last[variants[1][0]][0]).mean())
            for k, _ in variants:
                out["depths"][k]["depth_done_mean"] = float(last[k][4][last[k][3] != _lib.OPP_SKIPPED].mean())
        elif len(variants) == 2 and args.evaluation == "positional":   # against the material row of this run
            off, on = out["depths"][variants[0][0]], out["depths"][variants[1][0]]
            on["time_per_node_ratio_to_material"] = off["nodes_per_s"] / on["nodes_per_s"]
            on["ms_per_launch_ratio_to_material"] = on["ms_per_launch"] / off["ms_per_launch"]
            on["share_of_slots_with_another_move"] = float((last[variants[0][0]][0] != last[variants[1][0]][0]).mean())
        elif len(variants) == 2 and args.repetition:   # the rule's cost per node against the rule-off row of this run
            off, on = out["depths"][variants[0][0]], out["depths"][variants[1][0]]
            on["time_per_node_ratio_to_rule_off"] = off["nodes_per_s"] / on["nodes_per_s"]
            on["ms_per_launch_ratio_to_rule_off"] = on["ms_per_launch"] / off["ms_per_launch"]
            on["share_of_slots_with_another_move"] = float((last[variants[0][0]][0] != last[variants[1][0]][0]).mean())
        elif len(variants) == 2:                     # what ORDERING promises when no slot is cut: the same answers
            a, b = last[variants[0][0]], last[variants[1][0]]
            if not (a[3] == _lib.OPP_CUT).any() and not (b[3] == _lib.OPP_CUT).any():
                same = all(np.array_equal(a[j], b[j]) for j in (0, 1, 3, 4))
                out["depths"][variants[1][0]]["answers_equal_unordered"] = bool(same)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


def exchange_counts(args, budgets, words):
    """--exchange-counts: what the filter removes, counted by the restatement on the first N slots' positions."""
    from oracle.chess_oracle import OracleGame
    from tests import exchange_util as xu
    from tests import rollout_util as ru
    with open(args.out) as f:
        out = json.load(f)
    games = []
    for row in words[:args.exchange_counts]:
        g, w = OracleGame(), iter(int(x) for x in row)
        ru.run_in_slot(g, lambda: next(w), max_moves=args.opening_plies)
        games.append(g)
    for quiescence in (int(q) for q in args.quiescence.split(",")):
        for budget in budgets:
            key = ("<=%d@%d+q%d ordered" % (args.max_depth, budget, quiescence) +
                   (" repeating-aware" if args.repetition else "") +
                   (" positional" if args.evaluation == "positional" else "") +
                   (" selective" if args.selective else "") + " exchange-pruned")
            counts, nodes = xu.new_counts(), 0
            for g in games:
                nodes += xu.search(g, args.max_depth, min(budget, args.node_limit), quiescence, args.repetition,
                                   args.evaluation, args.selective, counts=counts)[2]
            row = out["depths"][key]
            row["removed_counted_on"] = {"slots": len(games), "nodes": nodes, "by": "tests/exchange_util.py on the CPU"}
            row["removed_by_delta_per_1000_nodes"] = 1e3 * counts["delta_removed"] / nodes
            row["removed_by_exchange_per_1000_nodes"] = 1e3 * counts["exchange_removed"] / nodes
            row["stand_pat_nodes_per_1000_nodes"] = 1e3 * counts["nodes_4c"] / nodes
            row["tactical_moves_at_them_per_1000_nodes"] = 1e3 * counts["tactical_moves"] / nodes
            print(key, json.dumps({k: v for k, v in row.items() if "per_1000" in k or k == "removed_counted_on"}),
                  flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
