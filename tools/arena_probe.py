"""tools/arena_probe.py -- what an arena ply costs on one GPU, and where the time goes.

    python tools/arena_probe.py [games=512] [blocks=6] [filters=64] [sims=100] [plies=6] [out=profiles/arena_probe.json]

Two seeded random-init weight sets play ``games`` games (``chessrl_amd.arena.Arena``: four engines of games/2 slots,
six random opening plies per pair).  The arena's own ply loop is run phase by phase with a device synchronisation
between the phases, so that every phase can be timed by the wall clock:

  * ms_per_searched_ply: one set's ply -- search, root_children, choose_children, advance(plies=1), the mirror push --
    median over the plies of both sets after one warm-up ply (which captures the graphs);
  * step_ms: GPU time of the ``sims`` lockstep steps of such a ply / sims (HIP events around ``run_steps``), beside
    plain_step_ms, the same for a plain ``LockstepEngine`` of games/2 slots on weight set A and the same openings --
    the code path an arena engine shares with self-play.  The two are ALTERNATED (an arena ply, a plain window) and each
    figure is the median of three windows;
  * boundary: ms and share of a ply spent in root_children, choose_children, advance and the mirror push.

The expectation this probe confirms or refutes: an arena step costs what a leaf step of games/2 rows costs, and the
boundary is noise at 100 simulations per move.  Nothing here is part of bench.py."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(dev, fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return out, (time.perf_counter() - t0) * 1e3


def steps_ms(eng, sims):
    """search_begin, then ``sims`` steps between two HIP events, then the last backup: (ms per step, wall ms of all)"""
    dev = eng.dev
    t0 = time.perf_counter()
    eng.search_begin()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    eng.run_steps(sims)
    e1.record()
    eng._backup(eng.pri_s2.data_ptr(), eng.val_s2.data_ptr())
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / sims, (time.perf_counter() - t0) * 1e3


def arena_ply(ar, s, state):
    """One ply of set ``s`` as ``Arena._search_ply`` plays it, phase by phase; None when the set has nothing to search
    or its games are not all on one side (the probe's openings leave them on one)."""
    from chessrl_amd import _lib
    from chessrl_amd.engine import choose_children
    plies, results, white = state
    live = results == _lib.RESULT_NONE
    movers = ar._movers(s, live, white)
    who = [w for w in ("a", "b") if movers[w].any()]
    if len(who) != 1:
        return None
    who = who[0]
    eng, mirror = s.engines[who], s.engines["b" if who == "a" else "a"]
    dev = eng.dev
    step, t_search = steps_ms(eng, ar.sims)
    rc, t_rc = timed(dev, eng.root_children)
    nchild = np.where(movers[who], rc["nchild"], 0)
    chosen, t_choose = timed(dev, lambda: choose_children(rc["visits"], nchild, rc["root_visits"], plies, noise=False))
    bm, t_adv = timed(dev, lambda: eng.advance(chosen, plies=1))
    _, t_push = timed(dev, lambda: mirror.ctx.push_moves(bm))
    _, state[0], state[1] = eng.ctx.records(with_moves=False)
    state[2] = np.where(live, ~white, white)
    return {"step_ms": step, "search_ms": t_search, "root_children_ms": t_rc, "choose_children_ms": t_choose,
            "advance_ms": t_adv, "mirror_push_ms": t_push,
            "ply_ms": t_search + t_rc + t_choose + t_adv + t_push, "searched": int(movers[who].sum())}


def main(argv):
    args = (argv + [None] * 5)[:5]
    games, blocks, filters, sims, plies = (int(a) if a is not None else d
                                           for a, d in zip(args, (512, 6, 64, 100, 6)))
    out_path = argv[5] if len(argv) > 5 else os.path.join("profiles", "arena_probe.json")
    from chessrl_amd.arena import Arena, _load
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.model import ChessModel
    model_a = ChessModel(blocks=blocks, filters=filters, seed=1)
    model_b = ChessModel(blocks=blocks, filters=filters, seed=2)
    ar = Arena(model_a, model_b, games=games, sims=sims, seed=5, opening_plies=6, max_plies=plies + 4)
    plain = LockstepEngine(model_a, games // 2, sims, max_plies=64)
    _load(plain.ctx, ar.specs)
    state = []
    for s in ar.sets:
        ctx = s.main_ctx()
        _, p, r = ctx.records(with_moves=False)
        state.append([p, r, (ctx.get_positions()[:, 7] & np.uint64(1)).astype(bool)])
    rows, plain_steps = [], []
    for ply in range(plies + 1):
        for s, st in zip(ar.sets, state):
            row = arena_ply(ar, s, st)
            if row is not None and ply:                        # (ply 0 captures the graphs of the first two engines,
                rows.append(row)                               #  ply 1 those of the other two: both are dropped below)
        step, _ = steps_ms(plain, sims)
        if ply:
            plain_steps.append(step)
    rows, plain_steps = rows[2:], plain_steps[1:]
    if not rows:
        raise RuntimeError("no ply was timed")

    def med(key, sel=rows):
        return float(np.median([r[key] for r in sel]))
    windows = [[r["step_ms"] for r in rows[i::3]] for i in range(3)]
    boundary = {k: med(k) for k in ("root_children_ms", "choose_children_ms", "advance_ms", "mirror_push_ms")}
    ply_ms = med("ply_ms")
    res = {"games": games, "blocks": blocks, "filters": filters, "sims": sims, "plies_timed": len(rows),
           "device": torch.cuda.get_device_name(0),
           "precision": {"a": model_a.precision, "b": model_b.precision},
           "rows_per_engine": games // 2, "games_searched_per_ply": med("searched"),
           "ms_per_searched_ply": ply_ms, "search_ms": med("search_ms"),
           "step_ms": {"median_of_three_windows": float(np.median([np.median(w) for w in windows if w])),
                       "windows": [float(np.median(w)) for w in windows if w],
                       "min": min(r["step_ms"] for r in rows), "max": max(r["step_ms"] for r in rows)},
           "plain_step_ms": {"median_of_three_windows": float(np.median(
                                 [np.median(plain_steps[i::3]) for i in range(3) if plain_steps[i::3]])),
                             "min": min(plain_steps), "max": max(plain_steps), "engine_rows": games // 2},
           "boundary_ms": boundary, "boundary_total_ms": sum(boundary.values()),
           "boundary_share_of_a_ply": sum(boundary.values()) / ply_ms}
    res["arena_step_over_plain_step"] = (res["step_ms"]["median_of_three_windows"] /
                                         res["plain_step_ms"]["median_of_three_windows"])
    ar.close()
    plain.close()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
