"""The arena without a GPU: the preconditions of the GPU set (tests/test_gpu_arena.py) checked with the oracle alone,
the tally, every refusal, the command line, and the one-ply entry point in the header and the binding.

The preconditions matter because the GPU tests compare games bit for bit: a set in which the two games of a pair
coincide, or in which no game ends, would compare less than it seems to.
"""
import os

import numpy as np
import pytest

from chessrl_amd import _lib
from chessrl_amd import arena as ar
from tests import arena_util as au


# ---- the GPU set, played by the oracle ----------------------------------------------------------------------------
def test_random_pairs_differ_after_the_opening_and_run_to_max_plies():
    out = au.reference("random")
    games = out["games"]
    assert len(games) == au.RANDOM_SET["games"]
    for i in range(0, len(games), 2):
        w, k = games[i], games[i + 1]
        assert w["a_white"] is True and k["a_white"] is False
        assert w["opening"] == k["opening"] and len(w["opening"]) == au.RANDOM_SET["opening_plies"]
        assert w["moves"] != k["moves"], "pair %d: both colour assignments play the same game" % (i // 2)
    for g in games:
        assert g["result"] is None and len(g["moves"]) == au.RANDOM_SET["max_plies"]
    assert len({tuple(g["opening"]) for g in games}) == len(games) // 2       # four different openings
    assert out["unfinished"] == out["played"] == len(games) and out["score_a"] == 0.0


def test_fen_pairs_end_as_the_positions_say():
    out = au.reference("fen")
    games = out["games"]
    assert [g["opening"] for g in games] == [f for f in au.FENS for _ in range(2)]
    for pair in (0, 1):                                      # mate in one, found by A as white and by B as white
        for g in games[2 * pair:2 * pair + 2]:
            assert g["result"] == 1 and len(g["moves"]) == 1
    for pair, result in ((2, 0), (3, 0), (4, -1)):           # finished before a move
        for g in games[2 * pair:2 * pair + 2]:
            assert g["result"] == result and g["moves"] == []
    for g in games[10:12]:                                   # halfmove clock 98: two plies, then the fifty-move rule
        assert g["result"] == 0 and len(g["moves"]) == 2
    # white wins pairs 0 and 1 whoever plays white; black's win in pair 4 goes to B in game 8 and to A in game 9
    assert (out["a_won"], out["b_won"], out["drawn"], out["unfinished"]) == (3, 3, 6, 0)
    assert out["score_a"] == 0.5
    assert out["as_white"] == dict(played=6, a_won=2, b_won=1, drawn=3, unfinished=0, score_a=3.5 / 6)


def test_restated_openings_are_gen_datas_words():
    """the opening of pair g is played from row g of the first block ``opening_words`` draws from Random(seed)"""
    import random
    from chessrl_amd import gen_data as gd
    from oracle.chess_oracle import OracleGame
    from tests import rollout_util as ru
    words = gd.opening_words(random.Random(5), 3, 4)
    for g, opening in enumerate(au.random_openings(3, 4, 5)):
        game, it = OracleGame(), iter(int(w) for w in words[g])
        ru.run_in_slot(game, lambda: next(it), max_moves=4)
        assert opening == [str(m) for m in game.board.move_stack]
    assert au.random_openings(2, 0, 5) == [[], []]


# ---- the tally -------------------------------------------------------------------------------------------------------
def test_tally_on_hand_made_results():
    a_white = [True, False, True, False, True, False, True, False]
    results = [1, 1, -1, -1, 0, 0, None, None]
    out = ar.tally(a_white, results)
    assert out == dict(played=8, a_won=2, b_won=2, drawn=2, unfinished=2, score_a=(2 + 1.0) / 8,
                       as_white=dict(played=4, a_won=1, b_won=1, drawn=1, unfinished=1, score_a=1.5 / 4))
    assert out == au.tally(a_white, results)
    swept = ar.tally([True, False], [1, -1])
    assert (swept["a_won"], swept["b_won"], swept["score_a"]) == (2, 0, 1.0)
    assert ar.tally([True, False], [None, None])["score_a"] == 0.0
    assert ar.game_colours(4) == [True, False, True, False]


# ---- refusals, before any device is touched --------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(games=3), dict(games=0), dict(games=-2), dict(sims=-1),
                                dict(games=4, openings=[["e2e4"]]), dict(games=2, openings=[]),
                                dict(opening_plies=-1), dict(max_plies=0)])
def test_refusals(kw):
    args = dict(games=2, sims=4)
    args.update(kw)
    with pytest.raises(ValueError):
        ar.arena(None, None, **args)                         # (no evaluator is looked at before the arguments)


def test_openings_are_fens_or_uci_lists():
    assert ar.parse_opening(au.FENS[0]) == (au.FENS[0], [])
    fen, ids = ar.parse_opening(["e2e4", "e7e5"])
    assert fen is None and [_uci(m) for m in ids] == ["e2e4", "e7e5"]
    with pytest.raises(ValueError):
        ar.parse_opening(["e2e4", "castles"])
    with pytest.raises(ValueError):
        ar.parse_opening("e2e4")


def _uci(m):
    from chessrl_amd.game import move_to_uci
    return move_to_uci(m)


# ---- the command line ------------------------------------------------------------------------------------------------
def test_cli_parser():
    a = ar.parser().parse_args(["dirA", "b.h5"])
    assert (a.a, a.b, a.sims, a.seed, a.opening_plies, a.openings, a.max_plies, a.noise) == \
        ("dirA", "b.h5", 0, 0, 6, None, 512, False)
    assert a.games % 2 == 0
    a = ar.parser().parse_args(["A", "B", "--games", "32", "--sims", "100", "--seed", "4", "--opening-plies", "8",
                                "--openings", "o.txt", "--max-plies", "200", "--noise"])
    assert (a.games, a.sims, a.seed, a.opening_plies, a.openings, a.max_plies, a.noise) == \
        (32, 100, 4, 8, "o.txt", 200, True)
    with pytest.raises(ValueError):
        ar.main(["A", "B", "--games", "5"])                  # refused before a weight file is opened


def test_cli_files(tmp_path):
    lines = tmp_path / "o.txt"
    lines.write_text("# two pairs\n%s\ne2e4 e7e5\n\n" % au.FENS[1])
    assert ar.read_openings(str(lines)) == [au.FENS[1], ["e2e4", "e7e5"]]
    js = tmp_path / "o.json"
    js.write_text('[["d2d4"], "%s"]' % au.FENS[0])
    assert ar.read_openings(str(js)) == [["d2d4"], au.FENS[0]]
    d = tmp_path / "model"
    d.mkdir()
    for name in ("model-3.h5", "model-4.h5"):
        (d / name).write_bytes(b"")
    assert ar.weights_path(str(d)) == str(d / "model-4.h5")
    assert ar.weights_path(str(d / "model-3.h5")) == str(d / "model-3.h5")


def test_summary_names_both_weight_files():
    out = ar.tally([True, False], [1, 0])
    text = ar.summary_lines(out, "runs/model-3.h5", "runs/model-4.h5", 100, "f16", "f16x3")
    assert any("runs/model-3.h5" in t and "f16" in t for t in text)
    assert any("runs/model-4.h5" in t and "f16x3" in t for t in text)
    assert text[-1].endswith("(paired openings, no Elo claim)")


# ---- the one-ply entry point -----------------------------------------------------------------------------------------
def test_advance_one_is_declared_and_bound():
    header = open(_lib.HEADER).read()
    assert "int  crl_advance_one(crl_ctx *ctx, const int32_t *chosen /*G*/, uint16_t *bm /*G*/);" in header
    assert "#define CRL_ABI_VERSION 9" in header and _lib.ABI_VERSION == 9
    assert "crl_advance_one" in _lib.SYMBOLS
    assert callable(getattr(_lib.Context, "advance_one"))
    api = open(os.path.join(os.path.dirname(_lib.HEADER), "..", "chessrl_amd", "csrc", "api.hip")).read()
    assert "int crl_advance_one(" in api and "k_advance_one" in api


def _bare_engine(**kw):
    """a LockstepEngine that never saw a device: ``advance`` must refuse before it reaches one (``ctx`` is None)"""
    from chessrl_amd.engine import LockstepEngine
    eng = object.__new__(LockstepEngine)
    eng.ctx, eng.max_sims, eng.max_nodes, eng.threads, eng.reply = None, 8, 9, 1, None
    for k, v in kw.items():
        setattr(eng, k, v)
    return eng


def test_advance_refuses_other_plies_and_other_engines():
    chosen = np.zeros(2, np.int32)
    with pytest.raises(ValueError):
        _bare_engine().advance(chosen, plies=3)
    with pytest.raises(ValueError):
        _bare_engine().advance(chosen, plies=0)
    with pytest.raises(ValueError):
        _bare_engine(reply=object()).advance(chosen, plies=1)
    with pytest.raises(ValueError):
        _bare_engine(max_nodes=64).advance(chosen, plies=1)
    with pytest.raises(ValueError):
        _bare_engine(threads=4).advance(chosen, plies=1)
    with pytest.raises(AttributeError):                      # a plain engine gets through to its (absent) context
        _bare_engine().advance(chosen, plies=1)
