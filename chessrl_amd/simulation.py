"""``RandomSimulation`` -- host mirror of the reference's random-playout leaf estimate, played on the GPU.

Same surface as /root/reference/src/chessrl/simulation.py:7-34: ``RandomSimulation(game).run(max_moves=100,
repetitions=1)``, the evaluator ``SelfPlayTree.simulate`` names as its alternative to ``predict_outcome``
(mctree.py:272-274).  Every ply -- move generation, the choice, the push, ``get_result`` -- is taken by the
gfx950 kernels of csrc/rollout.hpp through ``crl_rollout_games``; the host only supplies the random words.

The reference's behaviour is kept as it is, quirks included:

* the game handed in is MUTATED: the playout is pushed onto it;
* repetition r >= 1 does not start over, it plays the SAME game on for another ``max_moves`` plies;
* its ``n_mov > max_moves`` is never true, so a chunk that is still running yields ``None`` (not a draw), and
  ``np.mean`` over a list holding ``None`` raises ``TypeError`` -- raised here too, after the game was played;
* the return value is ``np.float64``.

Moves are chosen by ``random.choice`` in the reference; here the words that call would consume are drawn from the
global ``random`` module (one ``getrandbits(32)`` per Mersenne-Twister output, which is exactly what
``random._randbelow`` takes per try for n < 2^32), handed to the kernel in blocks, and afterwards the module's
state is put back and advanced by exactly the number of words the playout consumed: after ``random.seed(s)`` the
game played and the state ``random`` is left in are the reference's.

Beside the drop-in: ``rollout_values`` (independent playouts from many games at once, words from the device's
counter generator) and ``Rollouts``, the setting ``LockstepEngine(simulate=...)`` / ``SelfPlayTree(simulate=...)``
take to evaluate leaves by playouts instead of the value head.
"""
import collections
import random

import numpy as np

from . import _lib


class Rollouts(collections.namedtuple("Rollouts", "repetitions max_moves seed")):
    """Leaf evaluation by ``repetitions`` independent random playouts of at most ``max_moves`` plies (a playout
    still running then counts as a draw).  ``seed`` goes into the default stream keys: key of slot i =
    seed * 2^32 + i."""
    __slots__ = ()

    def __new__(cls, repetitions=1, max_moves=100, seed=0):
        if int(repetitions) < 1 or not 0 <= int(max_moves) <= 65534:
            raise ValueError("Rollouts: repetitions >= 1 and 0 <= max_moves <= 65534")
        return super().__new__(cls, int(repetitions), int(max_moves), int(seed))


def stream_keys(seed, n):
    """Default 64-bit stream keys of n slots: seed * 2^32 + slot (mod 2^64), as np.uint64."""
    return np.array([((int(seed) << 32) + i) & 0xFFFFFFFFFFFFFFFF for i in range(n)], dtype=np.uint64)


class RandomSimulation(object):
    """Drop-in for the reference's class of the same name; ``game`` is a ``chessrl_amd.game.Game``."""

    WORD_BLOCK = 512           # words drawn ahead per launch (a 100-ply playout takes about 160)

    def __init__(self, game):
        self.game = game

    def run(self, max_moves=100, repetitions=1, _word_block=None):
        """Plays the game on by random moves, ``repetitions`` chunks of ``max_moves`` plies (until it ends), and
        returns the mean of ``get_result()`` after every chunk -- ``TypeError`` when a chunk was still running.
        ``_word_block`` (tests only) sets how many words a launch is handed."""
        max_moves, repetitions = int(max_moves), int(repetitions)
        if repetitions < 1:
            return np.mean([])
        if max_moves < 0:
            max_moves = 0                                    # `n_mov < max_moves` is never true: nothing is played
        ctx = self.game._ctx()
        start = len(self.game)
        if start + repetitions * max_moves > ctx.max_plies:
            raise ValueError("a playout of %d x %d plies from ply %d does not fit the %d plies a Game slot holds"
                             % (repetitions, max_moves, start, ctx.max_plies))
        block = int(_word_block or self.WORD_BLOCK)
        state = random.getstate()
        played, consumed = None, 0
        try:
            while True:
                words = np.array([[random.getrandbits(32) for _ in range(block)]], dtype=np.uint32)
                played, used, chunks = self.game._ctx().rollout_games(words, [block], repetitions, max_moves, played)
                consumed += int(used[0])
                if int(used[0]) < block or int(played[0]) >= repetitions * max_moves or chunks[0, -1] != _lib.RESULT_NONE:
                    break
        finally:
            random.setstate(state)                           # leave the stream where random.choice would have
            for _ in range(consumed):
                random.getrandbits(32)
        return np.mean([None if r == _lib.RESULT_NONE else int(r) for r in chunks[0]])


_batch = {}


def _batch_context(n, max_plies, device):
    """A context of n slots for rollout_values, kept between calls of the same shape."""
    key = (n, max_plies, device)
    if key not in _batch:
        _batch.clear()
        _batch[key] = _lib.Context(n, 1, max_plies=max_plies, device=device)
    return _batch[key]


def rollout_values(games, repetitions, max_moves=100, seed=0, return_results=False):
    """Mean result of ``repetitions`` INDEPENDENT random playouts (at most ``max_moves`` plies each, a playout
    still running then counts 0) from the current position of every ``Game`` in ``games``; the games are not
    touched.  Words come from the device's counter generator, keyed by seed * 2^32 + index of the game, the
    game's ply and the repetition, so a call is reproducible.  Returns float32 [len(games)], with
    ``return_results`` also the int8 results and uint16 ply counts [len(games)][repetitions]."""
    import torch
    from .game import arena, ARENA_MAX_PLIES
    cfg = Rollouts(repetitions, max_moves, seed)
    n = len(games)
    if n == 0:
        raise ValueError("rollout_values: no games")
    src = arena()
    dev = torch.device("cuda", src.device)
    ctx = _batch_context(n, ARENA_MAX_PLIES, src.device)
    for i, g in enumerate(games):
        if g._slot is None:
            raise RuntimeError("Game was freed")
        ctx.copy_game_from(i, src.ctx, g._slot)
    keys = torch.from_numpy(stream_keys(cfg.seed, n).view(np.int64)).to(dev)
    value = torch.zeros(n, dtype=torch.float32, device=dev)
    results = torch.zeros((n, cfg.repetitions), dtype=torch.int8, device=dev)
    plies = torch.zeros((n, cfg.repetitions), dtype=torch.int16, device=dev)
    torch.cuda.synchronize(dev)
    ctx.rollout(_lib.ROLLOUT_GAMES, cfg.repetitions, cfg.max_moves, keys.data_ptr(), value.data_ptr(),
                results.data_ptr(), plies.data_ptr())
    ctx.sync()
    out = value.cpu().numpy()
    if return_results:
        return out, results.cpu().numpy(), plies.cpu().numpy().view(np.uint16)
    return out
