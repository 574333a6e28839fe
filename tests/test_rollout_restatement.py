"""CPU: the restatement of the random playouts (tests/rollout_util.py) is pinned to what it restates.

* run_in_slot replays every case of tests/golden/rollout_cases.json -- the reference's own simulation.py run on
  the C oracle (tools/make_rollout_golden.py) -- move for move, chunk result for chunk result, word for word;
* choice_index consumes Mersenne-Twister outputs exactly as ``random.choice`` does;
* philox4x32_10 (restated from the header comment of csrc/rollout.hpp) gives the known answers of Philox4x32-10;
* the header, the binding and the host module exist and agree.
"""
import hashlib
import os
import random

import numpy as np
import pytest

from tests import rollout_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ru.load_cases()


def state_digest():
    return hashlib.sha256(repr(random.getstate()).encode()).hexdigest()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_replays_the_reference_fixture(case):
    g = ru.case_game(case)
    random.seed(case["seed"])
    drawn = [0]

    def next_word():
        drawn[0] += 1
        return random.getrandbits(32)

    chunks = ru.run_in_slot(g, next_word, case["max_moves"], case["repetitions"])
    assert g.get_history()["moves"] == case["final_moves"]
    assert chunks == case["chunk_results"] and g.get_result() == case["final_result"]
    assert drawn[0] == case["words"]
    assert state_digest() == case["state_sha256"]              # the stream stands where the reference left it
    if case["returned"]["type"] == "TypeError":
        assert None in chunks
        with pytest.raises(TypeError):
            ru.mean_or_type_error(chunks)
    else:
        m = ru.mean_or_type_error(chunks)
        assert type(m).__name__ == case["returned"]["type"] == "float64" and float(m) == case["returned"]["value"]


def test_fixture_covers_what_the_dropin_test_needs():
    names = [c["name"] for c in CASES]
    assert sum(c["fen"] is None and not c["start_moves"] and c["max_moves"] == 100 for c in CASES) >= 3
    assert any(c["repetitions"] == 3 and len(c["final_moves"]) > c["max_moves"] for c in CASES)   # the continuation quirk
    assert any(c["words"] == 0 and c["final_result"] is not None for c in CASES)                    # a game already over
    assert any(c["max_moves"] == 5 and c["returned"]["type"] == "TypeError" for c in CASES)
    assert any(n.startswith("mate_in_one_available") for n in names)
    assert {c["returned"]["value"] for c in CASES} >= {1.0, -1.0, 0.0, None}
    assert any(None in c["chunk_results"] and c["chunk_results"][-1] is not None for c in CASES)   # ended in a later chunk


def test_word_accounting_is_random_choice_itself():
    """10^4 choices over n in 1 .. 218: the same indices and the same final state as ``random.choice``."""
    sizes = np.random.default_rng(7).integers(1, 219, size=10000)
    assert sizes.min() == 1 and sizes.max() == 218
    random.seed(20240229)
    want = [random.choice(range(int(n))) for n in sizes]
    after = random.getstate()
    random.seed(20240229)
    got = [ru.choice_index(int(n), lambda: random.getrandbits(32)) for n in sizes]
    assert got == want
    assert random.getstate() == after


# Known answers of Philox4x32-10: two of the philox4x32 / 10-round lines of the Random123 distribution's
# kat_vectors file (counter, key -> output; D. E. Shaw Research).  No copy of that file, and no other published
# vector of the algorithm, was available when this was written, so the lines are quoted from the publication from
# memory; a generator with a wrong constant or word order does not reproduce two 128-bit outputs by chance.
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,out", PHILOX_KAT)
def test_philox_known_answers(counter, key, out):
    assert tuple(ru.philox4x32_10(counter, key)) == out


def test_philox_word_stream_layout():
    """Draw i of a playout = output i & 3 of the call with counter (i >> 2, repetition, simulation, ply) under the
    key (low word, high word) of the slot's stream key."""
    key, ply, sim, rep = 0x0123456789ABCDEF, 37, 5, 2
    w = ru.PhiloxWords(key, ply, sim, rep)
    got = [w() for _ in range(10)]
    want = []
    for blk in range(3):
        want += ru.philox4x32_10((blk, rep, sim, ply), (0x89ABCDEF, 0x01234567))
    assert got == want[:10]
    assert got != [ru.PhiloxWords(key + 1, ply, sim, rep)() for _ in range(10)]


def test_private_playouts_on_the_oracle_are_deterministic_and_independent_of_order():
    from oracle.chess_oracle import OracleGame
    roots = [OracleGame()]
    a = ru.private(roots, [5], 6, 12)
    b = ru.private(roots, [5], 6, 12)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[0].dtype == np.float32
    assert (a[2] == 12).all() and a[3][0] == ["cut"] * 6 and len(roots[0]) == 0      # the root is not touched
    assert ru.playout(roots[0], 5, 0, 3, 12)[:2] == (int(a[1][0, 3]), int(a[2][0, 3]))


def test_header_binding_and_host_module_agree():
    from chessrl_amd import _lib
    text = open(os.path.join(ROOT, "include", "chessrl_hip.h")).read()
    for name in ("crl_rollout_games", "crl_rollout"):
        assert name in _lib.SYMBOLS and ("int  %s(" % name) in text
    assert "simulation.py:19-34" in text and "mctree.py:272-274" in text
    assert "#define CRL_ABI_VERSION 9" in text and _lib.ABI_VERSION == 9
    assert (_lib.ROLLOUT_GAMES, _lib.ROLLOUT_LEAVES, _lib.ROLLOUT_SKIPPED) == (0, 1, 0xFFFF) == (0, 1, ru.SKIPPED)
    hdr = open(os.path.join(ROOT, "chessrl_amd", "csrc", "rollout.hpp")).read()
    for const in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85"):
        assert const in hdr.split("#pragma once")[0]           # the generator is stated in the header comment
    from chessrl_amd.simulation import RandomSimulation, Rollouts, rollout_values, stream_keys   # noqa: F401
    assert Rollouts(4, 16, 3) == (4, 16, 3) and Rollouts() == (1, 100, 0)
    assert [int(k) for k in stream_keys(3, 2)] == [3 << 32, (3 << 32) + 1]
    with pytest.raises(ValueError):
        Rollouts(0)
