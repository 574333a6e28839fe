"""tools/make_golden_reroot.py -- TEST INFRASTRUCTURE: writes tests/golden/reroot_cases.json.

Needs the reference checkout (oracle/ref_loader.py imports its mctree.py where it lies); run from the
repository root:

    python -m tools.make_golden_reroot

Every case is the reference's own ``SelfPlayTree(game).search_move`` followed by one and two hops
``SelfPlayTree(tree.root.children[k]).search_move`` (mctree.py:98-111: the node is kept with everything
below it, ``root.visits = 1``), on the C-oracle chess rules with the deterministic FakeNet, in both numpy
promotion modes (see oracle/make_golden.py).  Per stage: the root children (visits, value sums as float64
hex, priors as float32 hex, our move, the stored reply), root visits, node count, the un-normalised
``compute_policy`` output, the child it chose and the ``(bm, am)`` ``search_move`` returned; for a hop also
what the kept node looked like before (children, legal moves, kept nodes, terminal nodes in the kept
subtree of both kinds: game over on our move / after the reply).  ``noise_seed`` on a stage:
``np.random.seed`` was called before that ``search_move(noise=True)``.

The file holds inputs and outputs only; no reference source text is stored.
"""
import json
import os

import numpy as np

from oracle import mcts_oracle, ref_loader
from oracle.fakenet import FakeNet
from oracle.make_golden import case2_game, f32hex, f64hex

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "reroot_cases.json")

# sims: [first search, hop 1, hop 2]; noise: {stage index: np.random seed}
CASES = [
    dict(name="opening_three_equal_moves", prefix=(1, 6), net=3, shift=30, sims=[60, 40, 40]),
    dict(name="wide_tree_child_not_fully_expanded", prefix=(2, 10), net=5, shift=24, sims=[120, 12]),
    dict(name="deep_tree_long_hops", prefix=(7, 40), net=9, shift=30, sims=[100, 120, 80]),
    dict(name="tiny_budget", prefix=(3, 16), net=5, shift=31, sims=[25, 10, 10]),
    dict(name="mates_and_fifty_move_claims_in_the_tree", fen="7k/8/4K3/8/6Q1/8/8/8 w - - 94 80", net=13, shift=30, sims=[90, 60, 60]),
    dict(name="rounding_ties", prefix=(9, 10), net=11, shift=30, tie=True, sims=[100, 60]),
    dict(name="castling_both_sides", fen="r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1", net=13, shift=30, sims=[90, 90, 90]),
    dict(name="noisy_hop", prefix=(5, 12), net=7, shift=30, sims=[80, 80], noise={1: 1234}),
]


def count(n, pred=lambda n: True):
    return int(pred(n)) + sum(count(k, pred) for k in n.children)


def walk(n):
    yield n
    for k in n.children:
        for x in walk(k):
            yield x


def stage_record(tree, moves, sims, root_plies, noise_seed, before):
    kids = tree.root.children
    if noise_seed is not None:
        np.random.seed(noise_seed)                       # the same draw search_move just made
    pol = tree.compute_policy(tree.root, noise=noise_seed is not None)
    chosen = int(np.argmax(pol))
    stacks = [[m.uci() for m in k.state.board.move_stack][root_plies:] for k in kids]

    def over_on_our_move(n):
        return n is not tree.root and n.state.get_result() is not None and \
            len(n.state.board.move_stack) - len(n.parent.state.board.move_stack) == 1

    def over_after_reply(n):
        return n is not tree.root and n.state.get_result() is not None and \
            len(n.state.board.move_stack) - len(n.parent.state.board.move_stack) == 2

    rec = {
        "sims": sims, "noise_seed": noise_seed, "root_plies": root_plies,
        "visits": [int(k.visits) for k in kids], "values": [f64hex(k.value) for k in kids],
        "priors": [f32hex(k.prior) for k in kids],
        "moves": [s[0] for s in stacks], "replies": [s[1] if len(s) > 1 else None for s in stacks],
        "root_visits": int(tree.root.visits), "n_nodes": count(tree.root),
        "terminal_on_our_move": count(tree.root, over_on_our_move),
        "terminal_after_reply": count(tree.root, over_after_reply),
        "root_fully_expanded": len(tree.root.unexpanded_actions) == 0,
        "policy": [f64hex(p) for p in pol], "policy_sum": float(np.sum(pol)), "chosen": chosen,
        "bm": moves[0], "am": moves[1],
        "chosen_child_result": kids[chosen].state.get_result(),
    }
    rec.update(before)
    return rec


def run_case(mct, c, mode):
    g = case2_game(c)
    agent = mcts_oracle.OracleAgent(FakeNet(seed=c["net"], prior_shift=c["shift"], tie=c.get("tie", False)), widen_priors=(mode == "legacy"))
    noise = c.get("noise", {})
    stages = []
    root = g
    before = {}
    for i, sims in enumerate(c["sims"]):
        tree = mct.SelfPlayTree(root, threads=1)
        assert tree.root.visits == 1
        seed = noise.get(i)
        if seed is not None:
            np.random.seed(seed)
        moves = tree.search_move(agent, max_iters=sims, noise=seed is not None, ai_move=True)
        stages.append(stage_record(tree, moves, sims, len(tree.root.state.board.move_stack), seed, before))
        ch = tree.root.children[stages[-1]["chosen"]]
        if ch.state.get_result() is not None:
            break
        over = [n_ for n_ in walk(ch) if n_ is not ch and n_.state.get_result() is not None]
        plies = [len(n_.state.board.move_stack) - len(n_.parent.state.board.move_stack) for n_ in over]
        before = {"kept_children": len(ch.children), "kept_legal_moves": len(ch.children) + len(ch.unexpanded_actions),
                  "kept_nodes": count(ch), "kept_terminal_on_our_move": plies.count(1),
                  "kept_terminal_after_reply": plies.count(2)}
        root = ch
    return {"name": c["name"], "mode": mode, "fen": c.get("fen"), "net_seed": c["net"], "prior_shift": c["shift"],
            "tie": c.get("tie", False), "prefix_moves": [m.uci() for m in g.board.move_stack], "stages": stages}


def main():
    mct = ref_loader.load_mctree()
    cases = []
    for c in CASES:
        for mode in ("nep50", "legacy"):
            r = run_case(mct, c, mode)
            cases.append(r)
            print(c["name"], mode, [(s["n_nodes"], s.get("kept_nodes"), s.get("kept_children"), s.get("kept_legal_moves"), s.get("kept_terminal_on_our_move"), s.get("kept_terminal_after_reply"),
                                     len(s["visits"]), s["root_fully_expanded"], s["terminal_on_our_move"],
                                     s["terminal_after_reply"], round(s["policy_sum"], 2), s["bm"], s["am"])
                                    for s in r["stages"]])
    with open(OUT, "w") as f:
        json.dump({"source": "mctree.SelfPlayTree(game).search_move and SelfPlayTree(Node).search_move (mctree.py:98-111, "
                             "159-198) of the reference, imported with a stub game module; numpy %s" % np.__version__,
                   "cases": cases}, f, separators=(",", ":"))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
