"""tools/wave_probe.py -- what ``threads`` > 1 (virtual-loss waves, csrc/search_wave.hpp) costs and buys on one GPU.

    python -m tools.wave_probe [G=1] [blocks=10] [filters=128] [sims=800] [moves=5] [threads=1,2,6,16,64] [out.json]

Seeded random-init net, the same seeds for every leg, noise off (every leg plays its own game from the second move on:
another T is another search).  Legs: one per T; T = 1 is today's one-leaf path (its kernels are untouched by the wave
mode), the baseline.  Per leg, over ``moves`` whole moves after one warm-up move that also captures the graphs:
  * move_ms: wall time of a whole ``sims``-simulation search between two device synchronisations -- search_begin, the
    steps, the last backup (crl_sim_backup at T = 1, crl_wave_backup at T > 1: the same region for every leg) and, for
    T > 1, the polls of the remaining budget, which are part of what a wave search costs -- median with min / max;
  * steps per move, mean wave size (simulations / steps of the slowest game = sims / steps) and the share of short
    waves over all games (crl_wave_stats).
Nothing here is part of bench.py; results go to the JSON file given (and stdout)."""
import json
import sys
import time

import numpy as np
import torch


def leg(model, G, sims, moves, T, seed=11):
    from chessrl_amd.selfplay import SelfPlayRunner
    run = SelfPlayRunner(model, n_parallel=G, sims=sims, seed=seed, noise=False, max_plies=1024, threads=T)
    run.GUARD_EVERY = 0
    eng, dev = run.engine, run.engine.dev
    eng.prepare_graphs()                                      # graphs are captured outside the timed region
    move_ms, steps, waves, short = [], [], 0, 0
    for m in range(moves + 1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        run.begin_move()
        if T > 1:
            k = eng.run_waves(sims)
        else:
            eng.run_steps(sims)
            eng.ctx.sim_backup(eng.pri_s2.data_ptr(), eng.val_s2.data_ptr())
            k = sims
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        if T > 1:
            ws = eng.ctx.wave_stats()
            live = run.active()[:len(ws["waves"])]
        run._sims_in_move = sims
        run.end_move()
        if m:
            move_ms.append((t1 - t0) * 1e3)
            steps.append(k)
            if T > 1:
                waves += int(ws["waves"][live].sum())
                short += int(ws["short_waves"][live].sum())
    out = {"threads": T, "G": G, "sims": sims, "moves": moves,
           "move_ms": {"median": float(np.median(move_ms)), "min": min(move_ms), "max": max(move_ms)},
           "steps_per_move": float(np.mean(steps)), "mean_wave_size": sims / float(np.mean(steps)),
           "short_wave_share": (short / waves) if waves else 0.0}
    run.close()
    return out


def main(argv):
    args = (argv + [None] * 5)[:5]
    G, blocks, filters, sims, moves = (int(a) if a is not None else d for a, d in zip(args, (1, 10, 128, 800, 5)))
    threads = [int(t) for t in (argv[5] if len(argv) > 5 else "1,2,6,16,64").split(",")]
    out_path = argv[6] if len(argv) > 6 else None
    from chessrl_amd.model import ChessModel
    model = ChessModel(blocks=blocks, filters=filters, seed=1)
    res = {"G": G, "blocks": blocks, "filters": filters, "sims": sims, "device": torch.cuda.get_device_name(0), "legs": []}
    for T in threads:
        r = leg(model, G, sims, moves, T)
        res["legs"].append(r)
        print(json.dumps(r), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
