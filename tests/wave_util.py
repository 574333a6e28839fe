"""Test-side restatement of the wave schedule (``threads`` > 1 with virtual loss) over oracle/mcts_oracle.py's node
type.  tests/test_wave_restatement.py pins it to tests/golden/wave_cases.json, which tools/make_golden_waves.py made
by driving the reference's own ``SelfPlayTree.select / simulate / backprop`` (mctree.py:216-296) in this schedule.

Per wave, up to T workers select one after the other on frozen statistics -- only the virtual loss (on the reached
node alone, mctree.py:226-227) and the tree's structure change -- then all simulate, then all back up in thread order.
A worker whose descent would step onto a node created earlier in the same wave stays idle: the wave ends short.
The virtual loss of a node is the number of this wave's leaves that ARE that node, so it lives in the wave's leaf
list and nowhere else."""
import json
import os

import numpy as np

from oracle import mcts_oracle
from oracle.chess_oracle import NULL_MOVE, OracleGame, board_from_fen
from oracle.fakenet import FakeNet
from oracle.make_golden import f32hex, f64hex
from oracle.mcts_oracle import _new_node, _puct

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wave_cases.json")
THREADS = (2, 6, 16, 64)


def load_cases():
    return json.load(open(GOLDEN))["cases"]


def case_game(c):
    g = OracleGame(board=board_from_fen(c["fen"])) if c["fen"] else OracleGame()
    for u in c["prefix_moves"]:
        assert g.move(u), u
    return g


def case_net(c):
    return FakeNet(seed=c["net_seed"], prior_shift=c["prior_shift"], tie=c["tie"])


def new_root(game):
    root = _new_node(game.get_copy(), None)
    root.visits = 1                                                    # mctree.py:111
    return root


def _score(c, mode, leaves):
    """Node.get_value (mctree.py:71-87): Q + U, then ``- self.vloss`` as one more float64 operation."""
    return _puct(c, mode) - sum(1 for x in leaves if x is c)


def _best(node, mode, leaves):
    return node.kids[int(np.argmax([_score(c, mode, leaves) for c in node.kids]))]


def _expand(node, agent):
    st = node.state.get_copy()
    mv = node.todo.pop()
    st.move(mv)
    reply = NULL_MOVE
    if st.get_result() is None:
        reply = agent.best_move(st, real_game=True)
        st.move(reply)
    child = _new_node(st, node)
    child.move, child.reply = mv, reply
    node.kids.append(child)
    if not node.todo:
        pri = agent.predict_policy(node.state, mask_legal_moves=True)
        for p, k in zip(pri, reversed(node.kids)):
            k.prior = p
    return child


def grow_waves(root, agent, n, threads, mode):
    """``n`` simulations below ``root`` in the wave schedule; returns the list of wave sizes."""
    done, waves = 0, []
    while done < n:
        W = min(threads, n - done)
        leaves, fresh = [], []
        while len(leaves) < W:
            node, stop = root, False
            while node.result is None and not node.todo:
                node = _best(node, mode, leaves)
                if any(node is f for f in fresh):
                    stop = True
                    break
            if stop:
                break
            if node.result is None:
                node = _expand(node, agent)
                fresh.append(node)
            leaves.append(node)
        values = [leaf.result if leaf.result is not None else agent.predict_outcome(leaf.state) for leaf in leaves]
        for leaf, v in zip(leaves, values):                            # thread order fixes the order of the f64 additions
            node = leaf
            while node is not None:
                node.visits += 1
                node.value += v
                node = node.parent
        done += len(leaves)
        waves.append(len(leaves))
    return waves


def count(n):
    return 1 + sum(count(k) for k in n.kids)


def root_stats(root):
    return {"visits": [int(c.visits) for c in root.kids], "values": [f64hex(c.value) for c in root.kids],
            "priors": [f32hex(c.prior) for c in root.kids], "moves": [c.move for c in root.kids],
            "replies": [None if c.reply == NULL_MOVE else c.reply for c in root.kids],
            "root_visits": int(root.visits), "n_nodes": count(root)}


def wave_search(game, agent, n, threads, mode):
    """(root, stats incl. waves / policy / chosen / bm / am) of one search from ``game``."""
    root = new_root(game)
    waves = grow_waves(root, agent, n, threads, mode)
    st = root_stats(root)
    pol = mcts_oracle.compute_policy(st["visits"], st["root_visits"], len(game), noise=False)
    st["waves"], st["policy"], st["chosen"] = waves, [f64hex(p) for p in pol], int(np.argmax(pol))
    ch = root.kids[st["chosen"]]
    stack = ch.state.board.move_stack
    st["bm"], st["am"] = (str(stack[-2]), str(stack[-1])) if len(stack) >= 2 else (NULL_MOVE, NULL_MOVE)
    return root, st


def play_game_waves(agent, sims, threads, moves=None, mode="nep50", player_color=True, noise=False, rng=None):
    """selfplay.play_game (selfplay.py:59-84), every move searched in the wave schedule; with ``noise`` the child is
    chosen by compute_policy's Dirichlet-noised argmax, drawn from ``rng``."""
    gam = OracleGame(player_color=player_color)
    agent.color = player_color
    if player_color is False:
        gam.move(agent.best_move(gam, real_game=True))
    n = 0
    while gam.get_result() is None and (moves is None or n < moves):
        root, st = wave_search(gam, agent, sims, threads, mode)
        chosen = st["chosen"]
        if noise:
            chosen = int(np.argmax(mcts_oracle.compute_policy(st["visits"], st["root_visits"], len(gam), noise=True, rng=rng)))
        ch = root.kids[chosen]
        gam.move(ch.move)
        if ch.reply != NULL_MOVE:
            gam.move(ch.reply)
        n += 1
    return gam
