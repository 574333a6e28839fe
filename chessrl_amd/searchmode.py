"""``SearchMode`` -- which kind of step a search runs and which optional capabilities that kind covers.

The one statement of the rule: ``LockstepEngine``, ``SelfPlayTree``, ``Agent.engine_for`` and ``SelfPlayRunner`` build
a mode from ``(threads, simulate, reply)`` and ask it; none of them restates a combination.  Widening a combination is
one cell of ``COVERS`` (and the kernels behind it).  Needs neither a GPU nor the HIP library.
"""
from ._lib import WAVE_MAX_THREADS
from .simulation import Rollouts

# kind -> the capabilities it covers (DESIGN.md section 4 shows the same table)
COVERS = {
    "leaf": {"tree_reuse", "stamps", "legal_priors", "raw_priors", "rollouts"},
    "wave": set(),
    "opponent": {"legal_priors", "raw_priors"},
}

# what LockstepEngine(reply=MinimaxPlayer) does not cover, each refused with a ValueError that names it
REPLY_REFUSED = {
    "threads": "reply= cannot be combined with threads > 1: the opponent's reply kernel serves one pending leaf per game",
    "simulate": "reply= cannot be combined with rollouts (simulate=Rollouts): the three-phase step has no playout phase",
    "max_nodes": "reply= cannot be combined with max_nodes (tree reuse): a search against the opponent starts from a "
                 "fresh tree",
    "reroot": "reply= cannot be combined with reroot: a search against the opponent starts from a fresh tree",
    "keep_root": "reply= cannot be combined with keep_root=True: a search against the opponent starts from a fresh tree",
    "set_stamps": "reply= cannot be combined with set_stamps: the stamped step is the four-phase step",
    "node": "reply= cannot continue a Node: a search against the opponent starts from a fresh tree (construct the "
            "tree from the Game)",
}

# (kind, how the capability was asked for) -> the refusal.  "node" is worded by the tree (virtual_loss is how a tree asks
# for waves); "tree:node" and "tree:simulate" are what SelfPlayTree(...) itself says before any engine exists.
REFUSED = {("opponent", how): text for how, text in REPLY_REFUSED.items() if how != "threads"}
REFUSED.update({
    ("wave", "simulate"): "threads > 1 cannot be combined with rollouts (simulate=Rollouts): the playout kernel values "
                          "one pending leaf per game",
    ("wave", "legal_priors"): "threads > 1 cannot be combined with legal_priors=True: the wave kernels read full policy "
                              "vectors",
    ("wave", "raw_priors"): "threads > 1 cannot be combined with raw_priors=True: the wave kernels read full policy "
                            "vectors",
    ("wave", "max_nodes"): "threads > 1 cannot be combined with max_nodes (tree reuse): a wave search starts from a "
                           "fresh tree",
    ("wave", "keep_root"): "threads > 1 cannot be combined with keep_root=True: a wave search starts from a fresh tree",
    ("wave", "reroot"): "threads > 1 cannot be combined with reroot: a wave search starts from a fresh tree",
    ("wave", "reuse_tree"): "threads > 1 cannot be combined with reuse_tree=True: a wave search starts from a fresh tree",
    ("wave", "set_stamps"): "threads > 1 cannot be combined with set_stamps: the stamped step is the one-leaf step",
    ("wave", "node"): "this Node comes from a search with virtual_loss=True and threads > 1: a wave engine starts every "
                      "search from a fresh tree and cannot continue a Node (construct the tree from the Game)",
    ("wave", "tree:node"): "virtual_loss=True with threads > 1 cannot continue a Node: a wave search starts from a "
                           "fresh tree (construct the tree from the Game)",
    ("wave", "tree:simulate"): "virtual_loss=True with threads > 1 cannot be combined with rollouts (simulate=Rollouts)",
})


class SearchMode(object):
    """``kind``: "leaf" (one leaf per game and step, the net's greedy reply), "wave" (``threads`` > 1: virtual-loss
    waves) or "opponent" (``reply``: the built-in opponent's replies).  ``tree=True`` words the wave x rollouts
    refusal as ``SelfPlayTree`` does."""

    def __init__(self, threads=1, simulate=None, reply=None, tree=False):
        if reply is not None:
            from .opponent import MinimaxPlayer
            if not isinstance(reply, MinimaxPlayer):
                raise TypeError("reply must be None or a chessrl_amd.opponent.MinimaxPlayer")
            if int(threads) > 1:
                raise ValueError(REPLY_REFUSED["threads"])
            if simulate is not None:
                raise ValueError(REFUSED["opponent", "simulate"])
        if simulate is not None and not isinstance(simulate, Rollouts):
            raise TypeError("simulate must be None or a chessrl_amd.simulation.Rollouts")
        threads = int(threads)
        if not 1 <= threads <= WAVE_MAX_THREADS:
            raise ValueError("threads must lie in [1, %d]" % WAVE_MAX_THREADS)
        self.threads, self.simulate, self.reply = threads, simulate, reply
        self.kind = "opponent" if reply is not None else "wave" if threads > 1 else "leaf"
        if simulate is not None:
            self.require("rollouts", "tree:simulate" if tree else "simulate")

    @classmethod
    def of(cls, holder):
        """The mode of whatever carries the plain attributes ``threads``, ``simulate`` and ``reply`` (an engine)."""
        return cls(getattr(holder, "threads", 1), getattr(holder, "simulate", None), getattr(holder, "reply", None))

    def covers(self, capability):
        return capability in COVERS[self.kind]

    def require(self, capability, how):
        """ValueError with the message of (kind, ``how``) unless the kind covers ``capability``; ``how`` names the
        entry that asked: max_nodes, keep_root, reroot, node, set_stamps, simulate, legal_priors, raw_priors,
        reuse_tree (and, from ``SelfPlayTree(...)``, tree:node and tree:simulate)."""
        if not self.covers(capability):
            raise ValueError(REFUSED.get((self.kind, how)) or REFUSED[self.kind, how.split(":")[-1]])

    @property
    def plan(self):
        """One step: [(the stamp in front of a phase when a StampRing is attached, the phase method by name)]."""
        from . import engine as e                # (the stamp ids live there: bench.py and the tools import them)
        if self.kind == "opponent":              # no tower call on S1: the opponent's search reads the board
            return [(e.STAMP_STEP, "phase_select_expand"), (e.STAMP_S1_DONE, "phase_reply_opponent"),
                    (e.STAMP_REPLIED, "phase_tower_s2")]
        plan = [(e.STAMP_STEP, "phase_select_expand"), (e.STAMP_SELECTED, "phase_tower_s1"),
                (e.STAMP_S1_DONE, "phase_reply"), (e.STAMP_REPLIED, "phase_tower_s2")]
        return plan + [(e.STAMP_ROLLOUT, "phase_rollout")] if self.simulate is not None else plan

    @property
    def kernels(self):
        """The ``Context`` methods of a step's kernel triple: select, reply and the last backup."""
        if self.kind == "wave":
            return ("wave_select", "wave_reply", "wave_backup")
        return ("sim_select_expand", "sim_reply", "sim_backup")

    @property
    def rows_per_game(self):
        return self.threads

    @property
    def key(self):
        """Hashable; equal for modes that search alike (the player's settings, not its identity)."""
        r = self.reply
        return (self.threads, self.simulate,
                None if r is None else (r.search_depth, r.node_limit, r.quiescence, r.node_budget, r.ordering, r.repetition,
                                         r.evaluation, r.selective, r.exchange))
