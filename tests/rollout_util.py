"""CPU restatement of the random playouts (chessrl_amd/csrc/rollout.hpp) over ``oracle.chess_oracle.OracleGame``.

TEST INFRASTRUCTURE.  Pure Python + numpy integers:

  choice_index       CPython's ``random.choice`` as a function of 32-bit words (the choice rule)
  philox4x32_10      the counter generator, restated from the header comment of rollout.hpp alone
  PhiloxWords        key / counter layout of one private playout's word stream
  run_in_slot        RandomSimulation.run (simulation.py:19-34) with the words handed in: the in-slot form
  playout / private  one private playout, and count x repetitions of them with their means
  RolloutAgent       an ``oracle.mcts_oracle`` agent whose predict_outcome is the restated mean

tests/test_rollout_restatement.py pins run_in_slot to tests/golden/rollout_cases.json (the reference's own
simulation.py), choice_index to ``random.choice`` itself and philox4x32_10 to published vectors.
"""
import json
import os
import sys

import numpy as np

from oracle import mcts_oracle
from oracle.chess_oracle import OracleGame, board_from_fen, lib as oracle_lib, move_to_uci

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_cases.json")
SKIPPED = 0xFFFF
M32 = 0xFFFFFFFF


def load_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def case_game(case, cls=OracleGame, from_fen=board_from_fen):
    """The start of a fixture case as a game of class ``cls`` (FEN or standard start, then the move list)."""
    g = cls(board=from_fen(case["fen"])) if case["fen"] else cls()
    for u in case["start_moves"]:
        assert g.move(u), u
    return g


# ---- the choice rule -------------------------------------------------------------------------------------
def choice_index(n, next_word):
    """Index ``random.choice`` picks among n items, taking 32-bit words from ``next_word()``."""
    k = int(n).bit_length()
    r = next_word() >> (32 - k)
    while r >= n:
        r = next_word() >> (32 - k)
    return r


# ---- Philox4x32-10 ----------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """(c0, c1, c2, c3), (k0, k1) -> four 32-bit words, as the header of rollout.hpp states it."""
    c = [np.uint64(int(x) & M32) for x in counter]
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    m0, m1, lo32, s32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(M32), np.uint64(32)
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
        p0, p1 = m0 * c[0], m1 * c[2]                      # 32 x 32 -> 64 bit: exact in uint64
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & lo32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & lo32]
    return [int(x) for x in c]


class PhiloxWords(object):
    """Word stream of one private playout: key = the slot's 64-bit stream key, counter = (draw >> 2, repetition,
    simulation index, game ply of the playout's root); draw i is output i & 3 of call i >> 2."""

    def __init__(self, key, ply, sim, rep):
        self.key = (int(key) & M32, (int(key) >> 32) & M32)
        self.tail = (int(rep), int(sim), int(ply))
        self.draw, self.block = 0, None

    def __call__(self):
        i = self.draw & 3
        if i == 0:
            self.block = philox4x32_10((self.draw >> 2,) + self.tail, self.key)
        self.draw += 1
        return self.block[i]


# ---- the in-slot form ---------------------------------------------------------------------------------------
def run_in_slot(game, next_word, max_moves=100, repetitions=1):
    """The game is played on in place; returns the per-chunk results (None = still running).  Repetition r >= 1
    continues the same game; the move count never exceeds max_moves, so no chunk is turned into a draw."""
    results = []
    for _ in range(repetitions):
        n = 0
        while n < max_moves and game.get_result() is None:
            moves = game.get_legal_moves()
            game.move(moves[choice_index(len(moves), next_word)])
            n += 1
        results.append(game.get_result())
    return results


def mean_or_type_error(results):
    """np.mean of the chunk results as the reference takes it: a TypeError when a chunk was still running."""
    return np.mean(results)


# ---- the private form ---------------------------------------------------------------------------------------
def end_reason(g):
    """Which rule of Game.get_result ended the (finished) game g, in position_result's order."""
    L = oracle_lib()
    n = len(g.legal_move_ids())
    clock = (int(g.board_at(0).state) >> 12) & 255
    if clock >= 100 and n > 0:
        return "fifty"
    if n == 0:
        return "mate" if L.og_in_check(g._h) else "stalemate"
    if L.og_insufficient(g._h):
        return "insufficient"
    if g.repetitions() >= 5:
        return "fivefold"
    return "seventyfive"


def playout(root, key, sim, rep, max_moves):
    """One private playout from a copy of ``root``: (result, plies, reason)."""
    g = root.get_copy()
    words = PhiloxWords(key, len(root), sim, rep)
    L = oracle_lib()
    t = 0
    while True:
        res = g.get_result()
        if res is not None:
            return res, t, end_reason(g)
        if t >= max_moves:
            return 0, t, "cut"
        moves = g.legal_move_ids()
        assert L.og_push(g._h, moves[choice_index(len(moves), words)])
        t += 1


def private(roots, keys, repetitions, max_moves, sim=0):
    """count x repetitions playouts: (values f32 [count], results i8, plies u16, reasons)."""
    n = len(roots)
    results = np.zeros((n, repetitions), np.int8)
    plies = np.zeros((n, repetitions), np.uint16)
    reasons = [[None] * repetitions for _ in range(n)]
    for i, root in enumerate(roots):
        for r in range(repetitions):
            results[i, r], plies[i, r], reasons[i][r] = playout(root, keys[i], sim, r, max_moves)
    return mean_values(results), results, plies, reasons


def mean_values(results):
    """(float)((double)integer sum / repetitions) per row."""
    s = results.astype(np.int64).sum(axis=1)
    return (s.astype(np.float64) / np.float64(results.shape[1])).astype(np.float32)


class RolloutAgent(mcts_oracle.OracleAgent):
    """OracleAgent whose predict_outcome is the mean of ``repetitions`` private playouts of the leaf, keyed as the
    device keys them: the slot's stream key, len(leaf game), the 0-based index of the simulation, the
    repetition.  A loop that knows the index sets ``sim`` before every simulation (``tests.reroot_util.grow``).
    ``mcts_oracle.search`` does not hand the simulation index to its agent -- simulations that end on a terminal
    node do not call it at all -- so while ``sim`` is None it is read from the caller's frame (the loop variable
    ``_`` of ``search``); test infrastructure only.  ``reasons`` logs how every playout ended (``end_reason`` or
    "cut"), in the order played."""

    def __init__(self, net, key, repetitions, max_moves, **kw):
        super().__init__(net, **kw)
        self.key, self.repetitions, self.max_moves = int(key), int(repetitions), int(max_moves)
        self.n_rollouts = 0
        self.sim = None
        self.reasons = []

    def predict_outcome(self, game):
        sim = self.sim
        if sim is None:
            frame = sys._getframe(1)
            assert frame.f_code.co_name == "search", frame.f_code.co_name
            sim = frame.f_locals["_"]
        outs = [playout(game, self.key, sim, r, self.max_moves) for r in range(self.repetitions)]
        self.reasons.extend(o[2] for o in outs)
        self.n_rollouts += 1
        return float(mean_values(np.array([[o[0] for o in outs]], np.int8))[0])


def random_prefix(n_plies, seed):
    """Move ids of a seeded random walk of n_plies from the standard position (the game still running)."""
    rng = np.random.default_rng(seed)
    while True:
        g = OracleGame()
        while len(g) < n_plies and g.get_result() is None:
            lm = g.legal_move_ids()
            g.move(move_to_uci(lm[int(rng.integers(len(lm)))]))
        if g.get_result() is None:
            return [g.board.move_stack[i].m for i in range(len(g))]


# ---- the roots of the private-form test (tests/test_gpu_rollout.py) ---------------------------------------
# 14 roots played with PRIVATE_MAX_MOVES plies and two whose own history already holds four occurrences of the
# root position, played with 8, so that a fifth is within reach.  (fen or None, uci moves pushed on top.)
PRIVATE_MAX_MOVES, SHUFFLE_MAX_MOVES, PRIVATE_REPETITIONS = 40, 8, 256
BLOCKED = "k7/p7/P7/8/8/p7/P7/K7 w - - 0 1"            # both kings shuffle behind locked pawns: Kb1 and Kb8 are forced
KNIGHT_SHUFFLE = ["g1f3", "g8f6", "f3g1", "f6g8"] * 3
KING_SHUFFLE = ["a1b1", "a8b8", "b1a1", "b8a8"] * 3


def private_roots():
    """[(name, OracleGame)]: 16 roots, the last two are the shuffles."""
    def fen(f, moves=()):
        g = OracleGame(board=board_from_fen(f))
        for u in moves:
            assert g.move(u), u
        return g

    def from_ids(ids):
        g = OracleGame()
        for m in ids:
            assert g.move(move_to_uci(m))
        return g

    roots = [("start", OracleGame())]
    roots += [("midgame_%d" % n, from_ids(random_prefix(n, seed=n))) for n in (20, 40, 60, 80)]
    roots += [("kpk", fen("8/8/8/4k3/8/4P3/4K3/8 w - - 0 1")),
              ("kbkn", fen("8/8/3k4/2n5/8/3B4/3K4/8 w - - 0 1")),
              ("clock_96", fen("7k/8/4K3/8/6Q1/8/8/8 w - - 96 80")),
              ("back_rank_white", fen("6k1/5ppp/8/8/8/8/8/R5K1 w - - 0 1")),
              ("back_rank_black", fen("r5k1/8/8/8/8/8/5PPP/6K1 b - - 0 1")),
              ("stalemate_near", fen("7k/5Q2/8/6K1/8/8/8/8 w - - 0 1")),
              ("kqk", fen("7k/8/5KQ1/8/8/8/8/8 w - - 0 1")),
              ("blocked", fen(BLOCKED)),
              ("218_moves", fen("R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1")),
              ("knight_shuffle", fen("rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1", KNIGHT_SHUFFLE)),
              ("king_shuffle", fen(BLOCKED, KING_SHUFFLE))]
    assert len(roots) == 16
    return roots
