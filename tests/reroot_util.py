"""Test-side oracle of tree reuse (Tree(Node), mctree.py:98-111) over oracle/mcts_oracle.py's node type:
``grow`` continues a tree by ``iters`` simulations, ``reroot`` takes a root child and sets ``visits = 1`` (the old
parent pointer stays, as in the reference: the backprop walks on into the abandoned part, harmlessly), and
``play_game_reuse`` plays a game with the keep-or-fresh rule of the device (kept nodes + sims <= tree_nodes).
tests/test_reroot_oracle.py pins it to tests/golden/reroot_cases.json, the reference's own runs."""
import json
import os

import numpy as np

from oracle import mcts_oracle
from oracle.chess_oracle import NULL_MOVE, OracleGame, board_from_fen
from oracle.fakenet import FakeNet
from oracle.make_golden import f32hex, f64hex
from oracle.mcts_oracle import _new_node, _puct

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reroot_cases.json")


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


def grow(root, agent, iters, mode):
    """``iters`` more explore_tree calls on the tree below ``root`` (mcts_oracle.search's loop body).  An agent with
    a ``sim`` attribute (tests.rollout_util.RolloutAgent) is told the 0-based index of every simulation."""
    for i in range(iters):
        if hasattr(agent, "sim"):
            agent.sim = i
        node = root
        while node.result is None:
            if node.todo:
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
                node = child
                break
            node = node.kids[int(np.argmax([_puct(c, mode) for c in node.kids]))]
        v = node.result
        if v is None:
            v = agent.predict_outcome(node.state)
        while node is not None:
            node.visits += 1
            node.value += v
            node = node.parent


def reroot(root, k):
    """SelfPlayTree(root.children[k]): that node with everything below it, visits = 1."""
    ch = root.kids[k]
    ch.visits = 1
    return ch


def count(n):
    return 1 + sum(count(k) for k in n.kids)


def root_stats(root):
    return {"visits": [int(c.visits) for c in root.kids], "values": [f64hex(c.value) for c in root.kids],
            "priors": [f32hex(c.prior) for c in root.kids], "moves": [c.move for c in root.kids],
            "replies": [None if c.reply == NULL_MOVE else c.reply for c in root.kids],
            "root_visits": int(root.visits), "n_nodes": count(root)}


def stage_policy(stats, root_plies, noise_seed):
    """compute_policy of a stage as the fixture made it (np.random.seed before a noisy one)."""
    if noise_seed is not None:
        np.random.seed(noise_seed)
    return mcts_oracle.compute_policy(stats["visits"], stats["root_visits"], root_plies, noise=noise_seed is not None)


def play_game_reuse(agent, sims, tree_nodes, moves=None, mode="nep50", noise=False, rng=None, player_color=True):
    """selfplay.play_game with tree reuse: after every move the chosen child's subtree is kept iff the game goes
    on and kept nodes + sims <= tree_nodes, else the next move starts from a fresh tree.  Returns the game and,
    per move, whether the tree was kept (True), dropped for lack of room (False) or the game ended (None), and
    the kept node counts."""
    gam = OracleGame(player_color=player_color)
    agent.color = player_color
    if player_color is False:
        gam.move(agent.best_move(gam, real_game=True))
    root = new_root(gam)
    decisions, kept_nodes = [], []
    n = 0
    while gam.get_result() is None and (moves is None or n < moves):
        grow(root, agent, sims, mode)
        pol = mcts_oracle.compute_policy([c.visits for c in root.kids], root.visits, len(gam), noise=noise, rng=rng)
        ch = root.kids[int(np.argmax(pol))]
        gam.move(ch.move)
        if ch.reply != NULL_MOVE:
            gam.move(ch.reply)
        n += 1
        if ch.result is not None:
            decisions.append(None)
            break
        kept = count(ch)
        if kept + sims <= tree_nodes:
            root = reroot(root, root.kids.index(ch))
            decisions.append(True)
            kept_nodes.append(kept)
        else:
            root = new_root(gam)
            decisions.append(False)
    return {"game": gam, "decisions": decisions, "kept": decisions.count(True), "fell_back": decisions.count(False),
            "kept_nodes": kept_nodes}
