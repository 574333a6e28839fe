#!/usr/bin/env python
"""Throughput of the random playouts (csrc/rollout.hpp): playouts/s and plies/s of the private form, the per-ply
cost of the in-slot form beside it, and the restatement's loop on the C oracle on one host core for the ratio.

    python tools/rollout_probe.py [--roots 4096] [--repetitions 64] [--max-moves 100] [--out profiles/rollout_probe.json]

Legs (each GPU leg is a child process under its own time limit; a leg that fails ends the probe):
  private_start    roots x repetitions playouts from the standard position
  private_midgame  the same from mid-game positions (64 seeded random prefixes of 40 plies, tiled over the roots)
  inslot_start     every slot plays its own game on for max_moves plies (history ring in HBM, words from the host)
  host             the restatement (tests/rollout_util.py) on the C oracle, one core, --host-playouts playouts
One warm-up launch, then three timed ones; the median is reported.  No threshold: this is a measurement.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEG_TIMEOUT_S = 240


def midgame_prefixes(n=64, plies=40):
    from tests import rollout_util as ru
    return [ru.random_prefix(plies, seed=1000 + i) for i in range(n)]


def leg_private(args, midgame):
    import numpy as np
    import torch
    from chessrl_amd import _lib
    from chessrl_amd.simulation import stream_keys
    dev = torch.device("cuda", 0)
    G, R = args.roots, args.repetitions
    ctx = _lib.Context(G, 1, max_plies=256)
    if midgame:
        pre = midgame_prefixes()
        tbl = np.array([pre[i % len(pre)] for i in range(G)], dtype=np.uint16)
        assert (ctx.push_sequences(tbl, np.full(G, tbl.shape[1], np.int32)) == tbl.shape[1]).all()
    keys = torch.from_numpy(stream_keys(1, G).view(np.int64)).to(dev)
    value = torch.zeros(G, dtype=torch.float32, device=dev)
    results = torch.zeros((G, R), dtype=torch.int8, device=dev)
    plies = torch.zeros((G, R), dtype=torch.int16, device=dev)
    times = []
    for i in range(4):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ctx.rollout(_lib.ROLLOUT_GAMES, R, args.max_moves, keys.data_ptr(), value.data_ptr(), results.data_ptr(),
                    plies.data_ptr())
        ctx.sync()
        if i:
            times.append(time.perf_counter() - t0)
    n_plies = int(plies.cpu().numpy().view(np.uint16).astype(np.int64).sum())
    res = results.cpu().numpy()
    ctx.close()
    t = statistics.median(times)
    return {"playouts": G * R, "plies": n_plies, "seconds": times, "median_s": t, "playouts_per_s": G * R / t,
            "plies_per_s": n_plies / t, "ns_per_ply": 1e9 * t / n_plies, "mean_plies": n_plies / (G * R),
            "decided": float((res != 0).mean()), "mean_value": float(value.mean())}


def leg_inslot(args):
    import numpy as np
    from chessrl_amd import _lib
    G = args.roots
    ctx = _lib.Context(G, 1, max_plies=256)
    stride = 4 * args.max_moves
    words = np.random.default_rng(1).integers(0, 1 << 32, size=(G, stride), dtype=np.uint64).astype(np.uint32)
    counts = np.full(G, stride, np.int32)
    times, n_plies = [], 0
    for i in range(4):
        ctx.reset_games()
        ctx.sync()
        t0 = time.perf_counter()
        played, used, _ = ctx.rollout_games(words, counts, 1, args.max_moves)
        if i:
            times.append(time.perf_counter() - t0)
        n_plies = int(played.sum())
    ctx.close()
    t = statistics.median(times)
    return {"playouts": G, "plies": n_plies, "seconds": times, "median_s": t, "plies_per_s": n_plies / t,
            "ns_per_ply": 1e9 * t / n_plies, "note": "includes the copy of the words to the device"}


def leg_host(args):
    from oracle.chess_oracle import OracleGame
    from tests import rollout_util as ru
    root = OracleGame()
    t0 = time.perf_counter()
    n_plies = sum(ru.playout(root, 1, 0, r, args.max_moves)[1] for r in range(args.host_playouts))
    t = time.perf_counter() - t0
    return {"playouts": args.host_playouts, "plies": n_plies, "seconds": t, "playouts_per_s": args.host_playouts / t,
            "plies_per_s": n_plies / t, "note": "python loop over the C oracle, one core, standard position"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=4096)
    ap.add_argument("--repetitions", type=int, default=64)
    ap.add_argument("--max-moves", type=int, default=100)
    ap.add_argument("--host-playouts", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_probe.json"))
    ap.add_argument("--leg", default=None)
    args = ap.parse_args()
    if args.leg:                                                   # child: one leg, its result as one JSON line
        fn = {"private_start": lambda: leg_private(args, False), "private_midgame": lambda: leg_private(args, True),
              "inslot_start": lambda: leg_inslot(args), "host": lambda: leg_host(args)}[args.leg]
        print("LEG " + json.dumps(fn()))
        return 0
    out = {"roots": args.roots, "repetitions": args.repetitions, "max_moves": args.max_moves, "legs": {}}
    for leg in ("private_start", "private_midgame", "inslot_start", "host"):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--roots", str(args.roots), "--repetitions",
               str(args.repetitions), "--max-moves", str(args.max_moves), "--host-playouts", str(args.host_playouts)]
        try:
            p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                               timeout=LEG_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print("leg %s ran into its time limit: stopping" % leg)
            return 1
        line = [x for x in p.stdout.splitlines() if x.startswith("LEG ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:])
            print("leg %s failed (%d): stopping" % (leg, p.returncode))
            return 1
        out["legs"][leg] = json.loads(line[-1][4:])
        print(leg, json.dumps(out["legs"][leg]))
    legs = out["legs"]
    out["gpu_over_host_plies_per_s"] = legs["private_start"]["plies_per_s"] / legs["host"]["plies_per_s"]
    out["private_over_inslot_ns_per_ply"] = legs["private_start"]["ns_per_ply"] / legs["inslot_start"]["ns_per_ply"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
