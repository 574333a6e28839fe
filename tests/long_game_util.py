"""Inputs of the long-game tests (tests/test_long_games_cpu.py, tests/test_gpu_long_games.py): games whose history
crosses the 256-entry ring of past positions (csrc/state.hpp: HIST_RING) once or twice.

TEST INFRASTRUCTURE, CPU only: seeded numpy generators through ``oracle.chess_oracle.OracleGame``; nothing is read
from a fixture.  Every builder scans a fixed seed range and keeps the first hit; the seeds the scans find are also
kept literal below, and tests/test_long_games_cpu.py asserts that scan and literal agree and that every input
satisfies what it was chosen for.

  long_prefix          a uniform-random legal walk from the start position, still running at a given ply
  straddling_fivefold  a walk running at ply L, then a four-move shuffle repeated four times: the position of ply L
                       recurs at L+4, L+8, L+12 and its fifth occurrence at L+16 ends the game as a draw
  late_roots           16 running games cut just before / after ply 256 and 512, each with the 40 plies that follow
"""
import collections
import functools

import numpy as np

from oracle.chess_oracle import OracleGame, lib as oracle_lib

RING = 256
SCAN = 200                                       # seeds a builder may try
SCAN_SECOND_WRAP = 2000                          # ... for a late root beyond ply 500: few uniform walks last that long

# L of the straddling games: the five occurrences land on ring indices 252..255, 0, 1, 2.. in every phase; the last
# two cross the second wrap.  Scans start at 7000 + L.
STRADDLE_L = (241, 244, 247, 250, 252, 253, 254, 255, 508, 511)
STRADDLE_SEEDS = {241: 7241, 244: 7244, 247: 7248, 250: 7250, 252: 7252, 253: 7254, 254: 7254, 255: 7255,
                  508: 7509, 511: 7547}

# (seed, cut) of the late roots: 12 around the first wrap, 4 around the second.  Scans start at LATE_SCAN0.
LATE_SCAN0 = 1000
LATE_CUTS = (248, 250, 252, 253, 254, 255, 257, 258, 259, 260, 261, 262, 505, 510, 513, 515)
LATE_ROOTS = ((1002, 248), (1000, 250), (1012, 252), (1001, 253), (1013, 254), (1008, 255), (1015, 257), (1011, 258),
              (1020, 259), (1014, 260), (1022, 261), (1016, 262), (1053, 505), (1202, 510), (1207, 513), (1211, 515))
LATE_EXTRA = 40                                  # plies that follow a late root (fewer where the game ends)

NATURAL_MIN = 301                                # the finished natural game of the training-batch test
NATURAL_SCAN0 = 3000
NATURAL_SEED = 3001

BOUNDARY_PLIES = 300                             # the ply-pool boundary test: a game running at this ply
BOUNDARY_SCAN0 = 5000
BOUNDARY_SEED = 5000


def ids_of(g, n=None):
    """Move ids of the first n plies of an oracle game (all by default)."""
    L = oracle_lib()
    return [int(L.og_move_at(g._h, i)) for i in range(len(g) if n is None else n)]


def replay(ids):
    """OracleGame from the start position after the move ids (each must be legal)."""
    g, L = OracleGame(), oracle_lib()
    for m in ids:
        assert L.og_push(g._h, int(m)), m
    return g


def push(g, m):
    return bool(oracle_lib().og_push(g._h, int(m)))


def clock(g):
    return (int(g.board_at(0).state) >> 12) & 255


def walk(seed, plies):
    """The seeded uniform-random legal walk from the start position: ``plies`` plies, or fewer where the game ends.
    A longer walk of the same seed begins with the shorter one."""
    rng = np.random.default_rng(seed)
    g = OracleGame()
    while len(g) < plies and g.get_result() is None:
        lm = g.legal_move_ids()
        push(g, lm[int(rng.integers(len(lm)))])
    return g


def long_prefix(seed, plies):
    """``walk(seed, plies)`` when it is still running at ``plies``, else None."""
    g = walk(seed, plies)
    return g if len(g) == plies and g.get_result() is None else None


# ---- straddling fivefold ---------------------------------------------------------------------------------------
def _quiet_piece_moves(g):
    """Legal moves of g that move no pawn and capture nothing, in legal order."""
    b = g.board_at(0)
    occ = 0
    for t in range(6):
        occ |= int(b.bb[t])
    pawns = int(b.bb[0])
    return [m for m in g.legal_move_ids() if not (m >> 12) and not (pawns >> (m & 63)) & 1 and not (occ >> ((m >> 6) & 63)) & 1]


def _back(m):
    return ((m >> 6) & 63) | ((m & 63) << 6)


def _shuffle_from(root):
    """The first (a, b) in legal order such that a, b, a^-1, b^-1 are quiet piece moves, legal in turn, and bring
    the position of ``root`` back (its second occurrence); None when there is none."""
    for a in _quiet_piece_moves(root):
        g1 = root.get_copy()
        push(g1, a)
        if g1.get_result() is not None:
            continue
        for b in _quiet_piece_moves(g1):
            g = g1.get_copy()
            ok = True
            for m in (b, _back(a), _back(b)):
                ok = ok and g.get_result() is None and m in _quiet_piece_moves(g) and push(g, m)
            if ok and g.repetitions() == root.repetitions() + 1:
                return a, b
    return None


def straddling_try(seed, L):
    """The straddling game of this seed, or None: running at every ply before L+16, drawn by the fifth occurrence
    of the position of ply L at L+16."""
    root = long_prefix(seed, L)
    if root is None or root.repetitions() != 1:
        return None
    ab = _shuffle_from(root)
    if ab is None:
        return None
    a, b = ab
    g = root.get_copy()
    for i in range(16):
        if g.get_result() is not None:
            return None
        if not push(g, (a, b, _back(a), _back(b))[i & 3]):
            return None
        if (i & 3) == 3 and g.repetitions() != 2 + (i >> 2):
            return None
    return g if g.get_result() == 0 and len(g) == L + 16 else None


def scan_straddling(L):
    """(seed, game): the first hit of the scan 7000 + L .. 7000 + L + SCAN."""
    for seed in range(7000 + L, 7000 + L + SCAN):
        g = straddling_try(seed, L)
        if g is not None:
            return seed, g
    raise LookupError("no straddling game for L = %d within %d seeds" % (L, SCAN))


@functools.lru_cache(maxsize=None)
def _straddling_ids(L):
    g = straddling_try(STRADDLE_SEEDS[L], L)
    if g is None:
        raise LookupError("seed %d gives no straddling game for L = %d" % (STRADDLE_SEEDS[L], L))
    return tuple(ids_of(g))


def straddling_fivefold(L, cut=None):
    """The straddling game for L (a fresh OracleGame each call), whole (L + 16 plies, result 0) or cut at a ply."""
    ids = _straddling_ids(L)
    return replay(ids if cut is None else ids[:cut])


# ---- the opponent's own fifth occurrence -------------------------------------------------------------------------
# A straddling game in which the built-in opponent (tests/opponent_util.py: alphabeta), asked at ply L + 14, itself
# plays the last two moves of the shuffle, at depth 1 and at depth 2: its two pushes complete the fifth occurrence,
# at ply L + 16 = 257, through ring entries on both sides of index 0.  (In the ten games above it leaves the shuffle.)
OPPONENT_L = 241
OPPONENT_SEED = 7254
OPPONENT_DEPTHS = (1, 2)


def opponent_try(seed, L=OPPONENT_L):
    from tests import opponent_util as ou
    g = straddling_try(seed, L)
    if g is None:
        return None
    ids = ids_of(g)
    for depth in OPPONENT_DEPTHS:
        c = replay(ids[:L + 14])
        for m in ids[L + 14:]:
            if c.get_result() is not None or ou.alphabeta(c, depth)[0] != m or not push(c, m):
                return None
    return g


def scan_opponent_fifth():
    """(seed, game): the first hit of the scan 7000 + OPPONENT_L .. + SCAN."""
    for seed in range(7000 + OPPONENT_L, 7000 + OPPONENT_L + SCAN):
        g = opponent_try(seed)
        if g is not None:
            return seed, g
    raise LookupError("no straddling game whose last two moves the opponent plays itself within %d seeds" % SCAN)


@functools.lru_cache(maxsize=None)
def opponent_fifth_ids():
    """Move ids of the whole game (OPPONENT_L + 16 plies, result 0)."""
    g = opponent_try(OPPONENT_SEED)
    if g is None:
        raise LookupError("seed %d gives no game whose last two moves the opponent plays itself" % OPPONENT_SEED)
    return tuple(ids_of(g))


# ---- late roots ----------------------------------------------------------------------------------------------------
LateRoot = collections.namedtuple("LateRoot", "seed cut ids")      # ids: cut + up to LATE_EXTRA move ids


def late_need(cut):
    """Plies a late root's walk must reach: the encoder test walks to cut + 10, and to 520 across the second wrap."""
    return max(cut + 10, 520) if cut > 2 * RING - 16 else cut + 10


def straddles(cut):
    """Do the eight history plies cut-1 .. cut-8 lie on both sides of a ring wrap (256 or 512)?"""
    return any(cut - 8 < w <= cut - 1 for w in (RING, 2 * RING))


@functools.lru_cache(maxsize=None)
def _walk_ids(seed):
    """(move ids, ended) of ``walk(seed, 2 * RING + 3 + LATE_EXTRA)``: what every cut of a seed is taken from."""
    g = walk(seed, LATE_CUTS[-1] + LATE_EXTRA)
    return tuple(ids_of(g)), g.get_result() is not None


def late_try(seed, cut):
    """LateRoot of this seed: the walk runs at ``cut`` and lasts at least ``late_need(cut)`` plies; else None."""
    ids, ended = _walk_ids(seed)
    if len(ids) < late_need(cut) or (len(ids) == cut and ended):
        return None
    return LateRoot(seed, cut, ids[:cut + LATE_EXTRA])


@functools.lru_cache(maxsize=None)
def late_roots():
    """The 16 late roots (LateRoot records, in the order of LATE_ROOTS)."""
    out = []
    for seed, cut in LATE_ROOTS:
        r = late_try(seed, cut)
        if r is None:
            raise LookupError("seed %d gives no late root at ply %d" % (seed, cut))
        out.append(r)
    return tuple(out)


def root_game(r):
    """The running game of a late root at its cut."""
    return replay(r.ids[:r.cut])


def scan_late_roots():
    """[(seed, cut)] in the order of LATE_CUTS: every cut takes the first seed of LATE_SCAN0 .. LATE_SCAN0 + SCAN
    (SCAN_SECOND_WRAP beyond ply 500) that no earlier cut took.  Roots 0, 2, 4, .. must have a halfmove clock >= 12
    at the cut (eight roots whose repetition scan looks back at least 12 plies; the playout test takes them), the
    others are taken as they come."""
    out, used = [], set()
    for i, cut in enumerate(LATE_CUTS):
        want = 12 if i % 2 == 0 else 0
        for seed in range(LATE_SCAN0, LATE_SCAN0 + (SCAN_SECOND_WRAP if cut > RING + LATE_EXTRA else SCAN)):
            r = None if seed in used else late_try(seed, cut)
            if r is not None and clock(replay(r.ids[:cut])) >= want:
                used.add(seed)
                out.append((seed, cut))
                break
        else:
            raise LookupError("late roots: the scan ran out of seeds at cut %d" % cut)
    return out


# ---- single games ----------------------------------------------------------------------------------------------------
def scan_natural():
    """(seed, game): the first walk from NATURAL_SCAN0 that ends by the rules after at least NATURAL_MIN plies."""
    for seed in range(NATURAL_SCAN0, NATURAL_SCAN0 + SCAN):
        g = walk(seed, 4000)
        if g.get_result() is not None and len(g) >= NATURAL_MIN:
            return seed, g
    raise LookupError("no finished natural game within %d seeds" % SCAN)


def natural_game():
    return walk(NATURAL_SEED, 4000)


def scan_boundary():
    for seed in range(BOUNDARY_SCAN0, BOUNDARY_SCAN0 + SCAN):
        if long_prefix(seed, BOUNDARY_PLIES + 1) is not None:
            return seed
    raise LookupError("no game running at ply %d within %d seeds" % (BOUNDARY_PLIES + 1, SCAN))


def boundary_game():
    """A game running at ply BOUNDARY_PLIES + 1 (so there is a legal move at BOUNDARY_PLIES), as move ids."""
    return ids_of(long_prefix(BOUNDARY_SEED, BOUNDARY_PLIES + 1))
