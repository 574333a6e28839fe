"""CPU: the inputs of tests/test_gpu_long_games.py (tests/long_game_util.py) satisfy what they were chosen for, by the
oracle alone -- lengths, results, clocks, repetition counts, where the history lies relative to the ring wrap -- and
every one of them DEPENDS on its history across the wrap: set up bare, the same position has another result or
other planes.  These are conditions on the inputs, not measurements; the seed lists are literal in long_game_util and
the scans that found them are run again here."""
import numpy as np

from oracle import encoder_oracle
from oracle.chess_oracle import OracleGame
from tests import long_game_util as lu


def bare(g):
    """The current position of g as a game without history."""
    return OracleGame(board=g.board_at(0))


def test_long_prefix_is_a_seeded_walk_that_is_still_running():
    alive = [s for s in range(1000, 1032) if lu.long_prefix(s, 330) is not None]
    assert len(alive) >= 8                                           # a scan bound of 200 seeds is ample
    g = lu.long_prefix(alive[0], 330)
    assert len(g) == 330 and g.get_result() is None
    assert lu.ids_of(lu.long_prefix(alive[0], 200)) == lu.ids_of(g, 200)      # a shorter walk is a prefix
    ended = [s for s in range(1000, 1032) if s not in alive][0]
    assert lu.walk(ended, 330).get_result() is not None and lu.long_prefix(ended, 330) is None


def test_straddling_games_end_by_the_fifth_occurrence_across_the_wrap():
    assert lu.STRADDLE_L == (241, 244, 247, 250, 252, 253, 254, 255, 508, 511)
    indices = set()
    for L in lu.STRADDLE_L:
        assert lu.scan_straddling(L)[0] == lu.STRADDLE_SEEDS[L], L          # the literal seed is the scan's first hit
        ids = lu.ids_of(lu.straddling_fivefold(L))
        assert len(ids) == L + 16
        a, b = ids[L], ids[L + 1]
        assert ids[L:] == [a, b, lu._back(a), lu._back(b)] * 4
        g = OracleGame()
        for ply, m in enumerate(ids):
            assert g.get_result() is None, (L, ply)                         # running at every ply before L + 16
            if ply >= L:
                assert m in lu._quiet_piece_moves(g), (L, ply)              # quiet, no pawn: the clock runs on
                if (ply - L) % 4 == 0:
                    assert g.repetitions() == 1 + (ply - L) // 4, (L, ply)
                    indices.add(ply % lu.RING)
            assert lu.push(g, m)
        assert g.get_result() == 0 and g.repetitions() == 5 and len(g) == L + 16
        assert lu.clock(g) < 100                                            # drawn by repetition, not by the clock
        # occurrences on both sides of a wrap, and the draw is in the history alone
        assert L < lu.RING * (1 + L // lu.RING) <= L + 16
        assert bare(g).get_result() is None
        for cut in (L + 12, L + 13, L + 14):                                # the cuts the GPU tests take
            c = lu.straddling_fivefold(L, cut)
            assert len(c) == cut and c.get_result() is None
        assert lu.straddling_fivefold(L, L + 12).repetitions() == 4
    assert indices >= {252, 253, 254, 255, 0, 1, 2, 3}                      # every phase around index 0


def test_the_opponent_itself_completes_a_fifth_occurrence_across_the_wrap():
    from tests import opponent_util as ou
    L = lu.OPPONENT_L
    assert lu.scan_opponent_fifth()[0] == lu.OPPONENT_SEED and L + 12 < lu.RING < L + 16
    ids = list(lu.opponent_fifth_ids())
    assert len(ids) == L + 16 and lu.replay(ids).get_result() == 0 and lu.replay(ids).repetitions() == 5
    assert bare(lu.replay(ids)).get_result() is None
    for depth in lu.OPPONENT_DEPTHS:
        g = lu.replay(ids[:L + 14])
        assert g.get_result() is None and ou.play_ply(g, depth) == ids[L + 14]
        assert g.get_result() is None and g.repetitions() == 4 and ou.play_ply(g, depth) == ids[L + 15]
        assert g.get_result() == 0 and g.repetitions() == 5 and lu.clock(g) < 100 and len(g) == L + 16


def test_late_roots_sit_around_the_first_and_the_second_wrap():
    roots = lu.late_roots()
    assert lu.scan_late_roots() == list(lu.LATE_ROOTS)
    assert [r.cut for r in roots] == list(lu.LATE_CUTS) and len(roots) == 16
    assert len(set(r.seed for r in roots)) == 16
    assert sum(248 <= r.cut <= 262 for r in roots) == 12 and sum(505 <= r.cut <= 515 for r in roots) == 4
    assert {253, 254, 255} <= set(r.cut for r in roots)
    clocks, differ = [], 0
    for r in roots:
        g = lu.root_game(r)
        assert len(g) == r.cut and g.get_result() is None
        assert lu.late_need(r.cut) <= len(r.ids) <= r.cut + lu.LATE_EXTRA
        assert lu.ids_of(lu.walk(r.seed, len(r.ids))) == list(r.ids)
        clocks.append(lu.clock(g))
        differ += not np.array_equal(encoder_oracle.get_game_state(g), encoder_oracle.get_game_state(bare(g)))
    assert sum(c >= 12 for c in clocks) >= 6, clocks       # the repetition scan looks back across index 0
    assert sum(c >= 8 for c in clocks[0::2]) == 8, clocks  # the playout test's eight roots
    assert sum(lu.straddles(r.cut) for r in roots) >= 6     # history planes from both sides of the wrap
    assert [lu.straddles(c) for c in (256, 257, 263, 264, 512, 513, 519, 520)] == [False, True, True, False] * 2
    assert differ >= 6


def test_single_games():
    assert lu.scan_natural()[0] == lu.NATURAL_SEED and lu.scan_boundary() == lu.BOUNDARY_SEED
    g = lu.natural_game()
    assert len(g) > 300 and g.get_result() is not None
    ids = lu.boundary_game()
    assert len(ids) == lu.BOUNDARY_PLIES + 1
    g = lu.replay(ids[:lu.BOUNDARY_PLIES])
    assert g.get_result() is None and ids[lu.BOUNDARY_PLIES] in g.legal_move_ids()
