"""``SelfPlayTree`` -- host mirror of the reference's MCTS class.

Same surface as /root/reference/src/chessrl/mctree.py:98-111,148-198: construct from a ``Game``
-- or from a ``Node`` that came out of a previous ``search_move`` (``tree.root.children[k]``), which
keeps that child's subtree: ``root.visits`` is 1 again and ``search_move`` adds ``max_iters`` more
simulations to what is already there -- call ``search_move(agent, max_iters, verbose, noise, ai_move)``, then read
``tree.root.visits`` and ``tree.root.children[i].visits / .value / .prior / .state``.  The
tree itself lives in HBM (flat node/edge arrays, one wavefront per game); select / expand /
backup are the HIP kernels behind crl_sim_* and the final ``compute_policy``
(mctree.py:305-322) stays on the host in numpy so that the Dirichlet noise comes from the
same ``np.random`` stream as the reference's.

The root is the caller's game as it stands -- whatever position it was set up from (standard
start, FEN, board row) and whatever moves were pushed since: the search engine's slot is a
device-side deep copy of the Game's arena slot (``crl_copy_game_from``), the counterpart of
``Node(root.get_copy())`` in mctree.py:105-109.

A kept subtree lives in the single-game engine that searched it and is overwritten by the next
search there: a ``Node`` can be continued only while its tree is the last one that engine searched
(``RuntimeError`` otherwise, never a silent fresh search), and only if the kept nodes plus
``max_iters`` fit the engine's node budget (``Agent(tree_nodes=...)``; ``ValueError`` naming the
size otherwise).  As in the reference, the kept children keep their visits while the root restarts
at 1, so ``compute_policy`` of a continued tree sums to more than 1.

``threads`` is accepted for signature compatibility and, by default, ignored: simulations run with the
reference's sequential (threads=1) semantics.  ``SelfPlayTree(game, threads=T, virtual_loss=True)`` honours it:
the search runs T workers per tree in the wave schedule (csrc/search_wave.hpp) -- the deterministic one among the
legal schedules of the reference's virtual-loss thread pool (mctree.py:12,173-176,226-227,289-293).  It is opt-in
because ``Agent`` passes ``threads=6`` today and honouring it would change what every caller gets.  A wave search
starts from a fresh tree: continuing a ``Node`` with ``virtual_loss=True`` raises.

``SelfPlayTree(game, reply=MinimaxPlayer(...))`` searches against the built-in opponent (``chessrl_amd/opponent.py``):
the reply stored in every new node, and shown as ``Node.reply``, is that opponent's move from the position after our
move instead of the net's greedy move.  One worker, the value head, a fresh tree: combining it with ``virtual_loss``
waves or rollouts, or continuing a ``Node`` of such a tree, raises ``ValueError``.
"""
import numpy as np

from .engine import compute_policy
from .game import Game, arena, move_to_uci
from .searchmode import SearchMode
from . import _lib


class Node(object):
    """Read-only view of one root child.  ``state`` (the child's Game: root + our move + the
    stored reply) is built on first access from the tree's SNAPSHOT of the root -- the copy taken
    when the search ran, mctree.py:105-109 ``Node(root.get_copy())`` -- so it does not depend on
    what the caller did to its own game afterwards; the device tree keeps only boards."""

    def __init__(self, root_snapshot, visits, value, prior, move, reply, tree=None, index=None):
        self.visits, self.value, self.prior = int(visits), float(value), np.float32(prior)
        self.move, self.reply = move, reply
        self.vloss = 0
        self.children = []
        self._root_snapshot, self._state = root_snapshot, None
        self._tree, self._index = tree, index        # where the device keeps this child's subtree

    @property
    def state(self):
        if self._state is None:
            g = self._root_snapshot.get_copy()
            for mv in (self.move, self.reply):
                if mv is not None and not g.move(mv):
                    raise RuntimeError("tree child %s%s does not replay on the root snapshot"
                                       % (self.move, "+" + self.reply if self.reply else ""))
            self._state = g
        return self._state


class _Root(object):
    def __init__(self, game, visits, children):
        self.state, self.visits, self.children = game, int(visits), children
        self.parent = None


def _subtree_size(nodes, c):
    """Nodes below and including node ``c`` (ids are handed out in creation order: parent < child)."""
    keep = np.zeros(len(nodes), dtype=bool)
    keep[c] = True
    parent = nodes["parent"]
    for i in range(c + 1, len(nodes)):
        keep[i] = keep[parent[i]]
    return int(keep.sum())


class Tree(object):
    def __init__(self, root):
        self._engine = None                              # the engine that holds this tree after search_move
        self._from = None
        if isinstance(root, Node) and root._tree is not None:
            # mctree.py:98-111: the node is kept with everything below it, root.visits = 1
            self._from = root
            self._game = root.state
            self.root = _Root(root.state, 1, [])
            return
        if not isinstance(root, Game):
            raise TypeError("root must be a chessrl_amd Game or a Node of a searched chessrl_amd tree")
        self._game = root
        self.root = _Root(root.get_copy(), 1, [])        # mctree.py:105-109: Node(root.get_copy())

    def _continue_on_device(self, max_iters):
        """Re-root the engine that holds the source tree at the node this tree was built from."""
        node = self._from
        src = node._tree
        eng = src._engine
        if eng is None or getattr(eng, "_tree_owner", None) is not src:
            raise RuntimeError("the device tree of this Node is gone: its engine has searched another tree since "
                               "(a Node can be continued only while its tree is the last one searched there)")
        SearchMode.of(eng).require("tree_reuse", "node")
        if node.reply is None:
            raise ValueError("search_move on a finished game (attempt to get argmax of an empty sequence)")
        nodes, edges, info = eng.ctx.fetch_tree(0)
        root = nodes[0]
        edge = edges[int(root["edge0"]) + int(root["nmoves"]) - 1 - node._index]
        kept = _subtree_size(nodes, int(edge["child"]) & 0x7FFF)
        if max_iters > eng.max_sims or kept + max_iters > eng.max_nodes:
            raise ValueError("continuing this Node needs %d tree nodes (%d kept + %d simulations), the engine "
                             "that holds it has %d: create the Agent with tree_nodes >= %d"
                             % (kept + max_iters, kept, max_iters, eng.max_nodes, kept + max_iters))
        chosen = np.array([node._index], dtype=np.int32)
        eng.reroot(chosen, max_iters)
        eng._tree_owner = None                           # the source tree is consumed
        return eng


class SelfPlayTree(Tree):

    def __init__(self, root, threads=6, simulate=None, virtual_loss=False, reply=None):
        """``simulate``: None -- leaves are valued by ``agent.predict_outcome`` (the value head) -- or a
        ``chessrl_amd.simulation.Rollouts``: by random playouts, the alternative mctree.py:272-274 names.
        ``virtual_loss``: the search uses ``threads`` workers per tree (the wave schedule).
        ``reply``: None -- the opponent's reply in a node is the net's greedy move -- or a
        ``chessrl_amd.opponent.MinimaxPlayer``: the built-in opponent's move ("the simulations against stockfish");
        ``Node.reply`` is then that move.  Such a search uses one worker, values leaves by the value head and starts
        from a fresh tree: the combinations are refused as ``LockstepEngine(reply=...)`` refuses them."""
        self.mode = SearchMode(threads if virtual_loss else 1, simulate, reply, tree=True)
        if isinstance(root, Node) and root._tree is not None:
            self.mode.require("tree_reuse", "tree:node")
        self.reply = reply
        super().__init__(root)
        self.num_threads = threads
        self.simulate = simulate
        self.virtual_loss = bool(virtual_loss)

    def search_move(self, agent, max_iters=200, verbose=False, noise=True, ai_move=False):
        # the tree searches its own snapshot of the caller's game (taken at construction, as the
        # reference's Node(root.get_copy())); one arena slot, returned when the tree is collected
        game = self.root.state
        if self._from is not None:
            eng = self._continue_on_device(max_iters)
            eng.search(max_iters, keep_root=True)
        else:
            eng = agent.engine_for(max_iters, mode=self.mode)
            eng._tree_owner = None
            eng.ctx.copy_game_from(0, arena().ctx, game._slot)
            eng.search(max_iters)
        rc = eng.root_children()
        n = int(rc["nchild"][0])
        if n == 0:
            # a finished root has no children; the reference's np.argmax([]) raises here too
            raise ValueError("search_move on a finished game (attempt to get argmax of an empty sequence)")
        kids = []
        for k in range(n):
            reply = rc["replies"][0, k]
            kids.append(Node(game, rc["visits"][0, k], rc["values"][0, k], rc["priors"][0, k],
                             move_to_uci(rc["moves"][0, k]),
                             None if reply == _lib.NO_MOVE else move_to_uci(reply), tree=self, index=k))
        self.root = _Root(game, rc["root_visits"][0], kids)
        self._engine, eng._tree_owner = eng, self
        stack = game.move_ids()
        policy = compute_policy([c.visits for c in kids], self.root.visits, len(stack), noise=noise)
        best = kids[int(np.argmax(policy))]
        # mctree.py:185-194 reads the last two entries of the chosen child's move stack
        if best.reply is not None:
            pair = (best.move, best.reply)
        elif len(stack) >= 1:                    # game over after our move: (previous ply, our move)
            pair = (move_to_uci(stack[-1]), best.move)
        else:                                    # one-entry stack: the IndexError branch
            pair = (Game.NULL_MOVE, Game.NULL_MOVE)
        return pair if ai_move else pair[0]
