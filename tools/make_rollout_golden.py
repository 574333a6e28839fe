#!/usr/bin/env python
"""Writes tests/golden/rollout_cases.json: inputs and outputs of the reference's own RandomSimulation.run.

The reference's ``simulation.py`` is imported where it lies (the pattern of oracle/ref_loader.py: a stub ``game``
module whose ``Game`` is the C-oracle duck type), ``random`` is seeded, and only data is recorded: the start (FEN
or standard position + move list), seed, max_moves, repetitions, the final move list, the list ``np.mean`` was
handed (the per-chunk results), the return value or the TypeError, the number of 32-bit Mersenne-Twister outputs
the run consumed and a digest of ``random.getstate()`` afterwards.  Nothing of the reference's text is copied.

    python tools/make_rollout_golden.py        (needs the reference tree; CPU only)
"""
import hashlib
import importlib
import json
import os
import random
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                                       # noqa: E402
from oracle import ref_loader                                            # noqa: E402
from oracle.chess_oracle import OracleGame, board_from_fen               # noqa: E402

KQK = "7k/8/5KQ1/8/8/8/8/8 w - - 0 1"                  # mate in one available (Qg7#)
BACK_RANK = "6k1/5ppp/8/8/8/8/8/R5K1 w - - 0 1"     # Ra8# available; seeds that mate at once, at ply 3, end in chunk 3, run on
FOOLS_MATE = ["f2f3", "e7e5", "g2g4", "d8h4"]
CASES = (
    [dict(name="start_seed%d" % s, fen=None, start_moves=[], seed=s, max_moves=100, repetitions=1) for s in (1, 2, 3, 4)] +
    [dict(name="start_three_chunks", fen=None, start_moves=[], seed=11, max_moves=40, repetitions=3),
     dict(name="game_already_over", fen=None, start_moves=FOOLS_MATE, seed=5, max_moves=100, repetitions=2),
     dict(name="five_plies_type_error", fen=None, start_moves=[], seed=6, max_moves=5, repetitions=1),
     dict(name="zero_plies", fen=None, start_moves=["e2e4"], seed=6, max_moves=0, repetitions=2)] +
    [dict(name="mate_in_one_available_seed%d" % s, fen=KQK, start_moves=[], seed=s, max_moves=100, repetitions=3)
     for s in (1, 2, 3, 4)] +
    [dict(name="back_rank_seed%d" % s, fen=BACK_RANK, start_moves=[], seed=s, max_moves=30, repetitions=3)
     for s in (1, 5, 18, 36)] +
    [dict(name="after_moves_seed%d" % s, fen=None, start_moves=["e2e4", "e7e5", "g1f3", "b8c6"], seed=s, max_moves=60,
          repetitions=2) for s in (7, 8)]
)


def load_simulation():
    stub = types.ModuleType("game")
    stub.Game = OracleGame
    saved = sys.modules.get("game")
    sys.modules["game"] = stub
    sys.modules.pop("simulation", None)
    sys.path.insert(0, ref_loader.REF_DIR)
    try:
        mod = importlib.import_module("simulation")
    finally:
        sys.path.remove(ref_loader.REF_DIR)
        sys.modules.pop("simulation", None)
        if saved is None:
            sys.modules.pop("game", None)
        else:
            sys.modules["game"] = saved
    return mod


def state_digest(state=None):
    return hashlib.sha256(repr(state or random.getstate()).encode()).hexdigest()


class _Numpy(object):
    """``np`` as simulation.py uses it (np.mean), remembering what mean was handed."""

    def __init__(self):
        self.seen = None

    def mean(self, values):
        self.seen = list(values)
        return np.mean(values)


def main():
    sim = load_simulation()
    out = []
    for c in CASES:
        g = OracleGame(board=board_from_fen(c["fen"])) if c["fen"] else OracleGame()
        for u in c["start_moves"]:
            assert g.move(u), u
        shim = sim.np = _Numpy()
        random.seed(c["seed"])
        try:
            ret = sim.RandomSimulation(g).run(max_moves=c["max_moves"], repetitions=c["repetitions"])
            ret = {"type": type(ret).__name__, "value": float(ret)}
        except TypeError:
            ret = {"type": "TypeError", "value": None}
        after = random.getstate()
        random.seed(c["seed"])
        words = 0
        while random.getstate() != after:
            random.getrandbits(32)
            words += 1
            assert words < 100000
        rec = dict(c)
        rec.update(final_moves=g.get_history()["moves"], chunk_results=shim.seen, final_result=g.get_result(),
                   returned=ret, words=words, state_sha256=state_digest(after))
        out.append(rec)
        print("%-32s plies %3d  chunks %-18s -> %-22s words %d" % (c["name"], len(rec["final_moves"]) - len(c["start_moves"]),
                                                                 shim.seen, ret, words))
    path = os.path.join(ROOT, "tests", "golden", "rollout_cases.json")
    with open(path, "w") as f:
        json.dump({"generator": "tools/make_rollout_golden.py", "python": sys.version.split()[0], "cases": out}, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
