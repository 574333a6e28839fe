"""The gate without a GPU: score and verdict, the early verdict over every course four games can take, the choice rule
the device boundary rests on, the parser, ``gated_round`` with fakes, and the argument errors of the device boundary.
"""
import itertools
import json
import os

import numpy as np
import pytest

from chessrl_amd import gating as gt


def tally(a_won, b_won, drawn, unfinished):
    return dict(played=a_won + b_won + drawn + unfinished, a_won=a_won, b_won=b_won, drawn=drawn,
                unfinished=unfinished)


# ---- score and verdict ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a_won,b_won,drawn,unfinished,half,accepted", [
    (4, 0, 0, 0, 8, True),
    (0, 4, 0, 0, 0, False),
    (2, 2, 0, 0, 4, False),
    (0, 0, 4, 0, 4, False),
    (0, 0, 0, 4, 4, False),             # every game cut off: all draws, 0.5
    (5, 3, 1, 1, 12, True),             # 12 / 20 = 0.6
    (9, 7, 2, 2, 22, True),             # 22 / 40 = 0.55 exactly: >= accepts
    (10, 9, 0, 1, 21, False),           # 21 / 40 = 0.525
    (3, 2, 0, 5, 11, True),             # 11 / 20 = 0.55 with unfinished games
])
def test_score_and_verdict_table(a_won, b_won, drawn, unfinished, half, accepted):
    t = tally(a_won, b_won, drawn, unfinished)
    assert gt.gate_half_points(t) == half
    assert gt.gate_score(t) == half / (2 * t["played"])
    assert gt.verdict(half, t["played"], 0.55) is accepted
    # the rule is symmetric: what A does not score, B scores
    swapped = tally(b_won, a_won, drawn, unfinished)
    assert gt.gate_half_points(t) + gt.gate_half_points(swapped) == 2 * t["played"]


def test_default_threshold_and_float64_verdict():
    assert gt.DEFAULT_THRESHOLD == 0.55
    assert gt.verdict(11, 10) is True and gt.verdict(10, 10) is False
    assert gt.verdict(1, 1, 0.5) is True and gt.verdict(0, 1, 0.0) is True and gt.verdict(1, 1, 1.0) is False
    assert gt.results_for_a([True, False, True, False, True], [1, 1, 0, -1, None]) == [1, -1, 0, 1, None]
    assert gt.bounds([1, 0, -1, None, None]) == (3, 7)


# ---- the early verdict ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [0.55, 0.5, 0.25, 0.75, 0.0, 1.0])
def test_early_verdict_equals_the_final_one_over_every_course_of_four_games(threshold):
    answered_early = 0
    for final in itertools.product((1, 0, -1), repeat=4):
        want = gt.verdict(sum(r + 1 for r in final), 4, threshold)
        for order in itertools.permutations(range(4)):
            seen = [None] * 4
            first = None
            for step in range(5):
                if step:
                    seen[order[step - 1]] = final[order[step - 1]]
                low, high = gt.bounds(seen)
                assert low <= sum(r + 1 for r in final) <= high
                d = gt.decided(seen, threshold)
                settled = gt.verdict(low, 4, threshold) == gt.verdict(high, 4, threshold)
                assert (d is not None) == settled                    # it answers at the first such moment
                if d is not None:
                    assert d is want                                 # ... and never anything but the final verdict
                    if first is None:
                        first = step
            assert first is not None                                 # all four finished: low == high
            answered_early += first < 4
    if 0.0 < threshold < 1.0:
        assert answered_early > 0


# ---- the choice rule of the device boundary ------------------------------------------------------------------------
def test_noise_free_choice_is_the_first_maximum_of_the_visits():
    """What ``k_choose_advance_one`` computes -- the first maximum of the visits in children order -- is what
    ``choose_children(noise=False)`` chooses, at every ply count (tau) and with ties."""
    from chessrl_amd.engine import choose_children
    rng = np.random.default_rng(20)
    ply_counts = np.array([0, 29, 30, 31, 100, 511, 4095])
    rows, width, block = 100000, 218, 10000
    ties = 0
    for start in range(0, rows, block):
        nchild = rng.integers(1, width + 1, size=block)
        nchild[:4] = [1, 2, 218, 64]
        top = rng.choice([1, 2, 3, 10, 60, 900], size=block)         # small ranges tie almost everywhere
        visits = (rng.integers(0, 901, size=(block, width)) % (top[:, None] + 1)).astype(np.int32)
        cols = np.arange(width)[None, :]
        inside = cols < nchild[:, None]
        root_visits = np.where(inside, visits, 0).sum(axis=1) + 1
        visits = np.where(inside, visits, 901).astype(np.int32)      # whatever lies past nchild is not looked at
        plies = ply_counts[(start + np.arange(block)) % len(ply_counts)]
        got = choose_children(visits, nchild, root_visits, plies, noise=False)
        masked = np.where(inside, visits, -1)
        want = np.argmax(masked, axis=1)                              # np.argmax: the first maximum
        assert np.array_equal(got, want)
        ties += int(((masked == masked.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    assert ties > rows // 4
    assert visits.max() == 901 and masked.max() == 900


# ---- the parser ------------------------------------------------------------------------------------------------------
def test_gate_flags_are_refused_where_they_do_not_apply(capsys):
    from chessrl_amd import selfplay as sp
    for argv in (["d", "--rounds", "2", "--gate-games", "7"],
                 ["d", "--rounds", "2", "--gate-games", "8", "--rolling"],
                 ["d", "--rounds", "2", "--gate-games", "8", "--no-train"]):
        p = sp.build_parser()
        with pytest.raises(SystemExit):
            sp.check_gate_args(p, p.parse_args(argv))
    capsys.readouterr()


def test_parsing_without_the_gate_flags_is_what_it_was():
    from chessrl_amd import selfplay as sp
    p = sp.build_parser()
    plain = vars(sp.check_gate_args(p, p.parse_args(["d", "--rounds", "3", "--sims", "40"])))
    gate_keys = {"gate_games": 0, "gate_sims": 40, "gate_threshold": 0.55, "gate_opening_plies": 6,
                 "gate_max_plies": 512}
    for k, v in gate_keys.items():
        assert plain.pop(k) == v, k
    assert sorted(plain) == sorted(["model_dir", "games", "threads", "virtual_loss", "debug", "sims", "parallel",
                                    "blocks", "filters", "seed", "no_noise", "rounds", "no_train", "rolling",
                                    "train_mode", "trainer_share", "reuse_tree", "tree_nodes", "max_plies",
                                    "dist_timeout_min", "precision", "numpy_promotion"])
    assert (plain["rounds"], plain["sims"], plain["rolling"], plain["no_train"]) == (3, 40, False, False)
    # --rolling and --no-train stay what they were while no gate is asked for
    for extra in ("--rolling", "--no-train"):
        assert vars(sp.check_gate_args(p, p.parse_args(["d", extra])))["gate_games"] == 0
    big = vars(sp.check_gate_args(p, p.parse_args(["d", "--gate-games", "16"])))
    assert big["gate_sims"] == 100 and big["sims"] == 900            # min(--sims, 100)
    own = vars(sp.check_gate_args(p, p.parse_args(["d", "--gate-games", "16", "--gate-sims", "7",
                                                   "--gate-threshold", "0.6", "--gate-opening-plies", "2",
                                                   "--gate-max-plies", "64"])))
    assert (own["gate_sims"], own["gate_threshold"], own["gate_opening_plies"], own["gate_max_plies"]) == \
        (7, 0.6, 2, 64)


# ---- gated_round with fakes ----------------------------------------------------------------------------------------
class FakeRecord(object):
    def __init__(self, tag, result=1, moves=("e2e4",)):
        self.tag, self.result, self.moves = tag, result, list(moves)

    def get_history(self):
        return {"moves": self.moves, "result": self.result, "player_color": True, "date": None}


def fake_weights(version):
    return {"meta.blocks": np.array(1), "meta.filters": np.array(8), "w": np.full(3, float(version))}


def settings_for(tmp_path, rnd, **kw):
    return dict(dict(round=rnd, model_path=str(tmp_path / "model-0.npz"), model_dir=str(tmp_path), games=8, sims=5,
                     threshold=0.55, seed=100 + rnd, opening_plies=2, max_plies=16), **kw)


def fake_gate(accept, seen):
    def gate_fn(candidate, incumbent):
        seen.append((float(candidate["w"][0]), float(incumbent["w"][0])))
        score = 0.75 if accept else 0.5
        return dict(accepted=accept, score=score, threshold=0.55, played=8, a_won=6 if accept else 4,
                    b_won=2 if accept else 4, drawn=0, unfinished=0, games=["not for the log"], sims=5, seed=-1,
                    stopped_at_ply=3 if accept else None, seconds=0.25, precision_candidate="f16",
                    precision_incumbent="f16x3")
    return gate_fn


def test_gated_round_accepts_rejects_and_carries(tmp_path):
    from chessrl_amd import selfplay as sp
    assert sp.GATE_CARRY_ROUNDS == 4
    trained = []

    def train_fn(weights, records):
        trained.append([r.tag for r in records])
        return fake_weights(weights["w"][0] + 1), [{"loss": 1.0}]

    path = tmp_path / "model-0.npz"
    loaded, seen = [], []
    weights, carried = fake_weights(0), []
    np.savez(str(path), **weights)
    before = path.read_bytes()
    # five rejected rounds: the incumbent stays, the file stays, the carry grows to four rounds and no further
    for rnd in range(5):
        new = [FakeRecord("r%d.%d" % (rnd, i)) for i in range(2)]
        s = settings_for(tmp_path, rnd, on_accept=loaded.append)
        weights, carried, entry = sp.gated_round(weights, new, carried, s, train_fn, fake_gate(False, seen))
        assert entry["accepted"] is False and entry["candidate"] is True and weights["w"][0] == 0.0
        assert len(carried) == min(rnd + 1, 4) and [r.tag for r in carried[-1]] == ["r%d.0" % rnd, "r%d.1" % rnd]
        assert path.read_bytes() == before and loaded == []
        assert entry["trained_on"] == 2 * min(rnd + 1, 5)
    assert trained[4] == ["r%d.%d" % (r, i) for r in range(5) for i in range(2)]      # carried + new, oldest first
    assert [r.tag for r in carried[0]] == ["r1.0", "r1.1"]                             # round 0 fell out of the cap
    # an accepted round: the candidate comes back, is written and loaded, and the carry is cleared
    new = [FakeRecord("r5.0")]
    weights, carried, entry = sp.gated_round(weights, new, carried, settings_for(tmp_path, 5, on_accept=loaded.append),
                                             train_fn, fake_gate(True, seen))
    assert trained[5] == ["r%d.%d" % (r, i) for r in range(1, 5) for i in range(2)] + ["r5.0"]
    assert entry["accepted"] is True and weights["w"][0] == 1.0 and carried == []
    assert len(loaded) == 1 and loaded[0] is weights
    assert seen[-1] == (1.0, 0.0)                                   # the candidate plays as A, the incumbent as B
    assert path.read_bytes() != before
    assert float(np.load(str(path))["w"][0]) == 1.0
    # a round without a trainable game: no candidate, no gate, the weights stay
    before = path.read_bytes()
    empty = [FakeRecord("cut", result=None), FakeRecord("nothing", moves=())]
    n_trained, n_seen = len(trained), len(seen)
    weights, carried, entry = sp.gated_round(weights, empty, carried, settings_for(tmp_path, 6), train_fn,
                                             fake_gate(True, seen))
    assert entry["candidate"] is False and entry["accepted"] is False and entry["trained_on"] == 0
    assert entry["score"] is None and weights["w"][0] == 1.0 and path.read_bytes() == before
    assert (len(trained), len(seen)) == (n_trained, n_seen) and len(carried) == 1
    # one log line per round, with the named keys
    lines = [json.loads(x) for x in open(os.path.join(str(tmp_path), sp.GATE_LOG))]
    assert [x["round"] for x in lines] == list(range(7))
    assert [x["accepted"] for x in lines] == [False] * 5 + [True, False]
    for x in lines:
        assert set(x) == set(sp.GATE_LOG_KEYS)
        assert {"round", "accepted", "score", "threshold", "played", "a_won", "b_won", "drawn", "unfinished", "games",
                "sims", "seed", "stopped_at_ply", "seconds", "trained_on", "precision_candidate",
                "precision_incumbent"} <= set(x)
    assert lines[5] == dict(round=5, candidate=True, accepted=True, score=0.75, threshold=0.55, played=8, a_won=6,
                            b_won=2, drawn=0, unfinished=0, games=8, sims=5, seed=-1, stopped_at_ply=3, seconds=0.25,
                            trained_on=9, precision_candidate="f16", precision_incumbent="f16x3")
    assert lines[0]["seed"] == -1 and lines[6]["seed"] == 106      # the gate's own seed where a gate was played


def test_h5_weights_are_rewritten_as_h5(tmp_path):
    from chessrl_amd import selfplay as sp
    from chessrl_amd.keras_h5 import load_keras_h5
    from chessrl_amd.model import init_weights
    w = init_weights(1, 8, seed=4)
    path = str(tmp_path / "model-1.h5")
    sp.save_weights_file(w, path)
    back = load_keras_h5(path)
    assert sorted(back) == sorted(w) and all(np.array_equal(back[k], w[k]) for k in w)


# ---- the device boundary's argument errors -------------------------------------------------------------------------
def test_device_boundary_is_refused_before_a_device_is_touched():
    from chessrl_amd import arena as ar

    class Untouchable(object):
        def __getattr__(self, name):
            if name == "device":
                raise AttributeError(name)
            raise AssertionError("the evaluator was touched: %s" % name)

    a, b = Untouchable(), Untouchable()
    with pytest.raises(ValueError, match="noise"):
        ar.Arena(a, b, games=2, sims=8, noise=True, boundary="device")
    with pytest.raises(ValueError, match="sims=0"):
        ar.Arena(a, b, games=2, sims=0, boundary="device")
    with pytest.raises(ValueError, match="boundary"):
        ar.Arena(a, b, games=2, sims=8, boundary="graph")
    with pytest.raises(ValueError, match="noise"):
        ar.arena(a, b, games=2, sims=8, noise=True, boundary="device")

    class On(object):
        def __init__(self, device):
            self.device = device

    with pytest.raises(ValueError, match="one stream"):
        ar.Arena(On("cuda:0"), On("cuda:1"), games=2, sims=8, boundary="device")
    ar.check_boundary("host", True, 0)                               # the host boundary takes what it took
    ar.check_boundary("device", False, 8, On("cuda:0"), On("cuda:0"))


def test_gate_refuses_bad_arguments_before_a_device_is_touched():
    with pytest.raises(ValueError):
        gt.gate(None, None, 3, 8)
    with pytest.raises(ValueError):
        gt.gate(None, None, 4, 8, threshold=1.5)
    with pytest.raises(ValueError):
        gt.gate(None, None, 4, 8, boundary="graph")


def test_new_entry_points_are_declared_bound_and_exported():
    from chessrl_amd import _lib
    header = open(_lib.HEADER).read()
    for name in ("crl_advance_one_argmax", "crl_push_moves_dev"):
        assert name in _lib.SYMBOLS and ("int  %s(" % name) in header
    assert "#define CRL_ABI_VERSION 9" in " ".join(header.split()) and _lib.ABI_VERSION == 9
    assert gt.parser().parse_args(["a", "b"]).threshold == 0.55
    a = gt.parser().parse_args(["a", "b", "--games", "8", "--sims", "5", "--threshold", "0.6", "--seed", "3",
                                "--opening-plies", "2", "--max-plies", "9", "--no-early-stop", "--host-boundary"])
    assert (a.games, a.sims, a.threshold, a.seed, a.opening_plies, a.max_plies, a.no_early_stop, a.host_boundary) == \
        (8, 5, 0.6, 3, 2, 9, True, True)
