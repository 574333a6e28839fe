"""tools/reroot_probe.py -- what tree reuse (``SelfPlayRunner(reuse_tree=True)``) costs and keeps on one GPU.

    python tools/reroot_probe.py [G=4096] [blocks=10] [filters=128] [sims=800] [moves=6] [out.json]

Seeded random-init net, the same seeds for every leg.  Legs: reuse off (the boundary is crl_advance_fetch, the
unchanged kernel), reuse on with tree_nodes = 2 * sims + 1 and 3 * sims + 1, each with noise on and off.  Per
leg, over ``moves`` whole moves after one warm-up move:
  * step_ms: GPU time of the ``sims`` lockstep steps of a move / sims (HIP events around ``run_steps``), median
    with min / max -- deeper trees lengthen the descent;
  * boundary_ms: wall time of ``end_move`` + ``begin_move`` between two device synchronisations, median with
    min / max -- with reuse on it holds the compaction;
  * kept / fell back moves, mean kept nodes, and an ESTIMATE of the bytes the compaction moved (kept nodes x
    (176 + mean branching x 24) read and written; the device does not count them).
Nothing here is part of bench.py; results go to the JSON file given (or stdout)."""
import json
import sys
import time

import numpy as np
import torch


def leg(model, G, sims, moves, reuse, tree_nodes, noise, seed=11):
    from chessrl_amd.selfplay import SelfPlayRunner
    run = SelfPlayRunner(model, n_parallel=G, sims=sims, seed=seed, noise=noise, max_plies=1024,
                         reuse_tree=reuse, tree_nodes=tree_nodes)
    run.GUARD_EVERY = 0
    dev = run.engine.dev
    step_ms, boundary_ms = [], []
    run.begin_move()
    for m in range(moves + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        run.engine.run_steps(sims)
        e1.record()
        run._sims_in_move = sims
        run._draw_noise_ahead()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        run.end_move()
        run.begin_move()
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        if m:                                                 # (move 0 captures the graphs)
            step_ms.append(e0.elapsed_time(e1) / sims)
            boundary_ms.append((t1 - t0) * 1e3)
    cnt = run.engine.ctx.counters()
    branch = cnt["branch_sum"] / max(cnt["nodes"], 1)
    out = {"reuse_tree": reuse, "tree_nodes": tree_nodes, "noise": noise, "moves": moves,
           "step_ms": {"median": float(np.median(step_ms)), "min": min(step_ms), "max": max(step_ms)},
           "boundary_ms": {"median": float(np.median(boundary_ms)), "min": min(boundary_ms), "max": max(boundary_ms)},
           "moves_kept": run.reuse_kept, "moves_fell_back": run.reuse_fell_back,
           "mean_kept_nodes": run.reuse_kept_nodes / max(run.reuse_kept, 1),
           "mean_branching": branch,
           "compaction_bytes_estimate_per_boundary": int(run.reuse_kept_nodes * (176 + branch * 24) / (moves + 1))}
    run.close()
    return out


def main(argv):
    args = (argv + [None] * 5)[:5]
    G, blocks, filters, sims, moves = (int(a) if a is not None else d for a, d in zip(args, (4096, 10, 128, 800, 6)))
    out_path = argv[5] if len(argv) > 5 else None
    from chessrl_amd.model import ChessModel
    model = ChessModel(blocks=blocks, filters=filters, seed=1)
    res = {"G": G, "blocks": blocks, "filters": filters, "sims": sims, "device": torch.cuda.get_device_name(0), "legs": []}
    for noise in (True, False):
        for reuse, nodes in ((False, None), (True, 2 * sims + 1), (True, 3 * sims + 1)):
            r = leg(model, G, sims, moves, reuse, nodes, noise)
            res["legs"].append(r)
            print(json.dumps(r), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
