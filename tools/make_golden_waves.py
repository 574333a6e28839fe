"""tools/make_golden_waves.py -- TEST INFRASTRUCTURE: writes tests/golden/wave_cases.json.

Needs the reference checkout (oracle/ref_loader.py imports its mctree.py where it lies); run from the
repository root:

    python -m tools.make_golden_waves

The reference's ``SelfPlayTree(root, threads=T)`` runs T ``explore_tree`` workers on one tree, kept apart by a
virtual loss (mctree.py:12,173-176,226-227,289-293).  Its thread pool is racy, but ``select``, ``simulate`` and
``backprop`` are separate public methods, and one legal schedule of the workers is deterministic -- the WAVE
schedule: up to T workers select one after the other (statistics frozen, only ``vloss`` and the tree's structure
change), then all simulate, then all back up in thread order.  A worker whose descent would step onto a node that
another worker of the same wave has just created stays idle for that wave (the wave ends short).  This tool
drives exactly that schedule on the reference's own ``SelfPlayTree.select / simulate / backprop``, on the C-oracle
chess rules with the deterministic FakeNet, in both numpy promotion modes (see oracle/make_golden.py).

Per case, mode and T: the root children (visits, value sums as float64 hex, priors as float32 hex, our move, the
stored reply), root visits, node count, the list of wave sizes, ``compute_policy(noise=False)`` and the
``(bm, am)`` that ``search_move`` derives from it.  The generator asserts the invariants of the schedule on every
run and that every event class the device kernels must handle occurs at least once in the file.

The file holds inputs and outputs only; no reference source text is stored.
"""
import json
import os

import numpy as np

from oracle import mcts_oracle, ref_loader
from oracle.fakenet import FakeNet
from oracle.make_golden import case2_game, f32hex, f64hex

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "wave_cases.json")

SIMS = 100
THREADS = (2, 6, 16, 64)
CASES = [
    dict(name="opening_three_equal_moves", prefix=(1, 6), net=3, shift=30),
    dict(name="deep_tree", prefix=(7, 40), net=9, shift=30),
    dict(name="rounding_ties", prefix=(9, 10), net=11, shift=30, tie=True),
    dict(name="mates_and_fifty_move_claims_in_the_tree", fen="7k/8/4K3/8/6Q1/8/8/8 w - - 94 80", net=13, shift=30),
    dict(name="castling_both_sides", fen="r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1", net=13, shift=30),
    dict(name="one_move_root", fen="k7/8/1K6/8/8/8/8/7R b - - 0 1", net=13, shift=30),
    dict(name="back_rank_mate", fen="6k1/5ppp/8/8/8/8/8/R3K3 w Q - 0 1", net=13, shift=30),
]


def walk(n):
    yield n
    for k in n.children:
        for x in walk(k):
            yield x


def dry_descent(root, fresh, ev):
    """The walk ``select`` is about to make, without side effects: (node it ends on, stepped onto a fresh node)."""
    node = root
    while not node.is_terminal_state and node.is_fully_expanded:
        for c in node.children:
            if c.visits == 0:
                ev["visits0_sibling_scored"] += 1
            if c.vloss and c.is_terminal_state:
                ev["terminal_child_scored_with_vloss"] += 1
        node = node.get_best_child()
        if id(node) in fresh:
            return node, True
    return node, False


def wave_search(tree, agent, n, T, ev):
    """``n`` simulations on ``tree`` in the wave schedule; returns the list of wave sizes."""
    done, waves = 0, []
    while done < n:
        W = min(T, n - done)
        leaves, fresh, completed = [], set(), []
        while len(leaves) < W:
            end, stop = dry_descent(tree.root, fresh, ev)
            if stop:
                break
            leaf = tree.select(tree.root, agent)
            if not end.is_terminal_state:                      # this select expanded ``end``
                assert leaf.parent is end and leaf.visits == 0
                fresh.add(id(leaf))
                if end.is_fully_expanded:
                    completed.append(len(leaves))
            else:
                assert leaf is end
            leaves.append(leaf)
        assert leaves
        ev["parent_full_mid_wave"] += sum(1 for i in completed if i < len(leaves) - 1)
        if len(leaves) < W:
            ev["short_waves"] += 1
        if W < T and done + W == n:
            ev["partial_last_wave"] += 1
        values = [tree.simulate(leaf, agent) for leaf in leaves]
        for leaf, v in zip(leaves, values):
            tree.backprop(leaf, v, remove_vloss=True)
        done += len(leaves)
        waves.append(len(leaves))
        for nd in walk(tree.root):                             # the invariants between waves
            assert nd.vloss == 0
            if nd is not tree.root and not nd.is_terminal_state:
                assert sum(c.visits for c in nd.children) == nd.visits - 1
    assert tree.root.visits == n + 1 and sum(waves) == n
    return waves


def record(tree, waves, T, root_plies, moves):
    kids = tree.root.children
    pol = tree.compute_policy(tree.root, noise=False)
    stacks = [[m.uci() for m in k.state.board.move_stack][root_plies:] for k in kids]
    return {"threads": T, "visits": [int(k.visits) for k in kids], "values": [f64hex(k.value) for k in kids],
            "priors": [f32hex(k.prior) for k in kids], "moves": [s[0] for s in stacks],
            "replies": [s[1] if len(s) > 1 else None for s in stacks], "root_visits": int(tree.root.visits),
            "n_nodes": sum(1 for _ in walk(tree.root)), "waves": waves, "policy": [f64hex(p) for p in pol],
            "chosen": int(np.argmax(pol)), "bm": moves[0], "am": moves[1]}


def moves_of(tree):
    """What search_move returns after its loop (mctree.py:178-198), noise off."""
    return tree.search_move(_NoAgent(), max_iters=0, noise=False, ai_move=True)


class _NoAgent(object):
    pass


def run_case(mct, c, mode, ev):
    g = case2_game(c)

    def agent():
        return mcts_oracle.OracleAgent(FakeNet(seed=c["net"], prior_shift=c["shift"], tie=c.get("tie", False)),
                                       widen_priors=(mode == "legacy"))
    # one thread in this schedule IS search_move
    seq = mct.SelfPlayTree(g, threads=1)
    seq_moves = seq.search_move(agent(), max_iters=SIMS, noise=False, ai_move=True)
    one = mct.SelfPlayTree(g, threads=1)
    wave_search(one, agent(), SIMS, 1, dict.fromkeys(ev, 0))
    root_plies = len(g.board.move_stack)
    base = record(one, [1] * SIMS, 1, root_plies, moves_of(one))
    ref = record(seq, [1] * SIMS, 1, root_plies, seq_moves)
    assert base == ref, c["name"]
    runs = []
    for T in THREADS:
        tree = mct.SelfPlayTree(g, threads=T)
        e = dict.fromkeys(ev, 0)
        waves = wave_search(tree, agent(), SIMS, T, e)
        r = record(tree, waves, T, root_plies, moves_of(tree))
        if len(base["visits"]) > 1:
            assert any(r[k] != base[k] for k in ("visits", "values", "n_nodes")), (c["name"], T)
        r["events"] = e
        for k in ev:
            ev[k] += e[k]
        runs.append(r)
    return {"name": c["name"], "mode": mode, "fen": c.get("fen"), "net_seed": c["net"], "prior_shift": c["shift"],
            "tie": c.get("tie", False), "prefix_moves": [m.uci() for m in g.board.move_stack], "sims": SIMS,
            "root_plies": root_plies, "runs": runs}


def main():
    mct = ref_loader.load_mctree()
    ev = {"short_waves": 0, "partial_last_wave": 0, "visits0_sibling_scored": 0,
          "terminal_child_scored_with_vloss": 0, "parent_full_mid_wave": 0}
    cases = []
    for c in CASES:
        for mode in ("nep50", "legacy"):
            r = run_case(mct, c, mode, ev)
            cases.append(r)
            print(c["name"], mode, [(x["threads"], len(x["waves"]), x["n_nodes"], x["events"]) for x in r["runs"]])
    for k, v in ev.items():
        assert v > 0, "event class %s never occurs in the fixture" % k
    with open(OUT, "w") as f:
        json.dump({"source": "mctree.SelfPlayTree.select / simulate / backprop (mctree.py:216-296) of the reference, "
                             "imported with a stub game module and driven in the wave schedule; numpy %s" % np.__version__,
                   "events": ev, "cases": cases}, f, separators=(",", ":"))
    print("wrote", OUT, os.path.getsize(OUT), "bytes", ev)


if __name__ == "__main__":
    main()
