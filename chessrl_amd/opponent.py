"""``MinimaxPlayer`` / ``GameOpponent`` -- the built-in opponent in the reference's shapes.

The reference measures and bootstraps against an engine: ``Stockfish(Player)``
(/root/reference/src/chessrl/stockfish.py:11-34) and ``GameStockfish(Game)``, a game that answers
every move of ours with the engine's (gamestockfish.py:6-61).  No engine binary belongs to this
package; what stands in its place is the fixed-depth alpha-beta player of ``csrc/opponent.hpp``,
one wavefront per game on the GPU.  It is NOT Stockfish: repetition below the root only on request
(``repetition=True``, below), no time control, and no Elo is claimed -- a result reads "against the built-in depth-d opponent".  Past the
fixed depth it can search ``quiescence`` plies of captures, promotions and check evasions
(opponent.hpp, QUIESCENCE); 0, the default, is the fixed-depth search alone.  With ``node_budget`` it deepens
iteratively up to ``search_depth`` and stops at that many nodes per move (opponent.hpp, ITERATIVE DEEPENING): the
deterministic counterpart of the reference's ``Limit(time=...)`` (stockfish.py:14-21); ``ordering=True`` on top of a
budget orders the moves below the root by victim and killer moves (opponent.hpp, ORDERING); ``repetition=True`` on top
of a budget scores a position below the root that occurred before -- on the search path or in the game's reversible
history -- a draw (opponent.hpp, REPETITION), so a side that is ahead stops shuffling into the fivefold;
``evaluation="positional"`` on top of a budget replaces the static evaluation (material and centrality) by a tapered
one with pawn structure, mobility, files, king shelter and king attack (opponent.hpp, EVALUATION);
``selective=True`` on top of ``ordering`` adds null-move pruning and late-move reductions, so the budget goes to fewer
lines, deeper (opponent.hpp, SELECTIVE); ``exchange=True`` on top of ``ordering`` and ``quiescence`` >= 1 drops, at the
quiescence nodes that stand pat, the captures that cannot come near alpha or lose material on their square (opponent.hpp,
EXCHANGE).  The batched form (thousands of games per launch) is ``Context.opponent_moves``;
these classes are the one-game drop-in surface over it.
"""
import numpy as np

from . import _lib
from .game import Game, arena, move_to_uci
from .player import Player

MAX_DEPTH = _lib.OPP_MAX_DEPTH
MAX_QUIESCENCE = _lib.OPP_MAX_QUIESCENCE
NODE_LIMIT = _lib.OPP_NODE_LIMIT


def clamp_depth(depth):
    """A search depth the kernel takes: [1, MAX_DEPTH]."""
    return max(1, min(MAX_DEPTH, int(depth)))


class MinimaxPlayer(Player):
    """Mirror of ``Stockfish(Player)``: ``best_move(game)`` is the UCI string of the depth-``search_depth``
    alpha-beta move for a ``chessrl_amd.Game`` (``'00000'`` on a finished game), with ``quiescence`` plies of
    quiescence search past that depth.  ``node_budget`` (None: no budget, the fixed-depth search): iterative deepening
    with ``search_depth`` as the maximum depth under ``min(node_budget, node_limit)`` nodes per move; ``last_depth`` is
    then the depth the last search completed (None without a budget).  ``ordering`` (needs a ``node_budget``): below
    the root that search tries the moves by victim, then the killer moves of the ply (opponent.hpp, ORDERING); with a
    budget it does not reach it plays the same move for fewer nodes.  ``repetition`` (needs a ``node_budget``): a node
    below the root whose position occurred before is worth 0 (opponent.hpp, REPETITION).  ``evaluation``: "material"
    or "positional" (needs a ``node_budget``; opponent.hpp, EVALUATION).  ``selective`` (needs ``ordering``): null-move
    pruning and late-move reductions (opponent.hpp, SELECTIVE); the search is then no longer full-width.  ``exchange``
    (needs ``ordering`` and ``quiescence`` >= 1): delta and exchange pruning in quiescence (opponent.hpp, EXCHANGE)."""

    def __init__(self, color, search_depth=2, node_limit=NODE_LIMIT, quiescence=0, node_budget=None, ordering=False,
                 repetition=False, evaluation="material", selective=False, exchange=False):
        super().__init__(color)
        if not 1 <= int(search_depth) <= MAX_DEPTH:
            raise ValueError("search_depth must lie in [1, %d]" % MAX_DEPTH)
        if int(node_limit) < 1:
            raise ValueError("node_limit must be at least 1")
        self.options = _lib.OpponentOptions(quiescence, node_budget, ordering, repetition, evaluation, selective,
                                            exchange)
        self.search_depth = int(search_depth)
        self.node_limit = int(node_limit)
        (self.quiescence, self.node_budget, self.ordering, self.repetition, self.evaluation, self.selective,
         self.exchange) = self.options
        self.last = None                      # (score, nodes, flag) of the last search
        self.last_depth = None                # with a budget: the depth that search completed

    def best_move(self, game):
        if game._slot is None:
            raise RuntimeError("Game was freed")
        ctx = arena().one(game._slot)
        out = ctx.opponent_moves(np.array([self.search_depth], np.int32), push=False, node_limit=self.node_limit,
                                 **self.options.kwargs)
        moves, scores, nodes, flags = out[:4]
        self.last = (int(scores[0]), int(nodes[0]), int(flags[0]))
        self.last_depth = int(out[4][0]) if self.node_budget is not None else None
        if int(moves[0]) == _lib.NO_MOVE:
            return Game.NULL_MOVE
        return move_to_uci(moves[0])

    def kill(self):
        """Nothing to end: kept for the drop-in shape (stockfish.py:33-34)."""


class GameOpponent(Game):
    """Mirror of ``GameStockfish``: a game against the built-in opponent.  ``opponent``: a ``MinimaxPlayer``, or
    None for one of depth ``opponent_depth``, ``opponent_quiescence``, ``opponent_budget`` (the player's
    ``node_budget``), ``opponent_ordering`` (its ``ordering``), ``opponent_repetition`` (its ``repetition``) and
    ``opponent_evaluation`` (its ``evaluation``), ``opponent_selective`` (its ``selective``) and ``opponent_exchange``
    (its ``exchange``) with the colour opposite to ``player_color``."""

    def __init__(self, opponent=None, player_color=Game.WHITE, board=None, date=None, opponent_depth=2,
                 opponent_quiescence=0, opponent_budget=None, opponent_ordering=False, opponent_repetition=False,
                 opponent_evaluation="material", opponent_selective=False, opponent_exchange=False):
        if opponent is not None and not isinstance(opponent, MinimaxPlayer):
            raise ValueError("opponent must be a MinimaxPlayer or None")
        self.opponent = None                  # (a board's move stack is replayed by plain Game.move)
        super().__init__(board=board, player_color=player_color, date=date)
        if opponent is None:
            opponent = MinimaxPlayer(not self.player_color, search_depth=opponent_depth,
                                     quiescence=opponent_quiescence, node_budget=opponent_budget,
                                     ordering=opponent_ordering, repetition=opponent_repetition,
                                     evaluation=opponent_evaluation, selective=opponent_selective,
                                     exchange=opponent_exchange)
        self.opponent = opponent

    def move(self, movement):
        """gamestockfish.py:27-41: if the opponent is white and nothing was played yet, the opponent moves and
        ``movement`` is ignored; otherwise our move is made and, if it was legal and the game goes on, the
        opponent replies."""
        if self.opponent is None:
            return Game.move(self, movement)
        if self.opponent.color and len(self) == 0:
            Game.move(self, self.opponent.best_move(self))
        else:
            made = Game.move(self, movement)
            if made and self.get_result() is None:
                Game.move(self, self.opponent.best_move(self))

    def get_copy(self):
        return GameOpponent(opponent=self.opponent, player_color=self.player_color, board=self, date=self.date)

    def tearup(self):
        self.opponent.kill()

    def free(self):
        """Unlinks the game from its opponent (gamestockfish.py:54-56) and gives the device slot back."""
        self.opponent = None
        Game.free(self)
