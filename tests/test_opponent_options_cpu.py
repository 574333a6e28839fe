"""No GPU: which options of the built-in opponent combine, asked of every surface that takes them.

``_lib.OpponentOptions`` is the one statement of the rules in Python; ``MinimaxPlayer``, ``Context.opponent_moves``,
``Context.sim_reply_opponent``, ``gen_data.gen_data`` and ``benchmark.benchmark`` build it from their keywords.  Over
node_budget in {None, 300} x quiescence in {0, 2} x evaluation in {"material", "positional", "pst"} x the sixteen
settings of (ordering, repetition, selective, exchange) -- 192 cases:

(a) every surface accepts the same cases, and they are the ones the rules restated here allow;
(b) a refused case raises the message of the first rule it breaks, in the constructor's order, on every surface
    (``benchmark`` words the ordering rule with its own argument names);
(c) an accepted case is what ``MinimaxPlayer``'s attributes and ``SearchMode(reply=...).key`` then hold.
"""
import itertools

import pytest

from chessrl_amd import _lib
from chessrl_amd.benchmark import benchmark
from chessrl_amd.gen_data import gen_data
from chessrl_amd.opponent import MinimaxPlayer
from chessrl_amd.searchmode import SearchMode

NAMES = ("quiescence", "node_budget", "ordering", "repetition", "evaluation", "selective", "exchange")
CASES = [dict(zip(NAMES, (q, b, o, r, e, s, x)))
         for b, q, e, (o, r, s, x) in itertools.product((None, 300), (0, 2), ("material", "positional", "pst"),
                                                        itertools.product((False, True), repeat=4))]


def first_broken_rule(quiescence, node_budget, ordering, repetition, evaluation, selective, exchange):
    """The rules restated, root first: the message of the first one the case breaks, None for a case that combines.
    (The ranges of quiescence and node_budget come first and hold in every case here.)"""
    assert 0 <= quiescence <= 6 and (node_budget is None or node_budget >= 1)
    if ordering and node_budget is None:
        return "ordering needs a node_budget"
    if repetition and node_budget is None:
        return "repetition needs a node_budget"
    if evaluation not in ("material", "positional"):
        return 'evaluation must be one of "material", "positional"'
    if evaluation == "positional" and node_budget is None:
        return "evaluation needs a node_budget"
    if selective and not ordering:
        return "selective needs ordering"
    if exchange and not ordering:
        return "exchange needs ordering"
    if exchange and quiescence < 1:
        return "exchange needs quiescence >= 1"
    return None


def past_validation(call):
    """A ``Context`` method called unbound with ``self = None``: the AttributeError of its first use of ``self``."""
    with pytest.raises(AttributeError):
        call()


def surfaces(kw, tmp_path):
    """name -> a call that takes the case through that surface."""
    return {
        "OpponentOptions": lambda: _lib.OpponentOptions(**kw),
        "MinimaxPlayer": lambda: MinimaxPlayer(False, 3, **kw),
        "opponent_moves": lambda: past_validation(lambda: _lib.Context.opponent_moves(None, [1], **kw)),
        "sim_reply_opponent": lambda: past_validation(
            lambda: _lib.Context.sim_reply_opponent(None, 0, 1000, 0, 0, 0, dev_depth_sum=0, **kw)),
        "gen_data": lambda: gen_data(str(tmp_path / "games.json"), num_games=0, **kw),
        "benchmark": lambda: benchmark(None, games=0, opponent_quiescence=kw["quiescence"],
                                       opponent_budget=kw["node_budget"],
                                       **{"opponent_" + k: kw[k] for k in NAMES[2:]}),
    }


def test_the_cases_are_the_192():
    assert len(CASES) == 192 and len({tuple(c.items()) for c in CASES}) == 192
    accepted = [c for c in CASES if first_broken_rule(**c) is None]
    # with a budget: 2 evaluations x 2 repetition x (Q = 0: 3 of (ordering, selective, exchange); Q = 2: 5); without: Q
    assert len(accepted) == 2 * 2 * (3 + 5) + 2


def test_every_surface_takes_the_same_cases_with_the_same_words(tmp_path):
    for kw in CASES:
        want = first_broken_rule(**kw)
        for name, call in surfaces(kw, tmp_path).items():
            if want is None:
                call()                                           # (a): accepted
                continue
            words = want
            if name == "benchmark" and want == "ordering needs a node_budget":
                words = "opponent_ordering needs an opponent_budget"
            with pytest.raises(ValueError) as err:               # (a): refused, and (b): with these words
                call()
            assert str(err.value) == words, (name, kw)


def test_an_accepted_case_is_what_the_player_holds():
    for kw in CASES:
        if first_broken_rule(**kw) is not None:
            continue
        p = MinimaxPlayer(False, 3, **kw)
        assert {k: getattr(p, k) for k in NAMES} == kw and p.options == _lib.OpponentOptions(**kw)
        assert p.options.kwargs == kw
        for k in NAMES:
            if k not in ("node_budget", "evaluation"):
                assert type(getattr(p, k)) is type(kw[k]), k
        assert SearchMode(reply=p).key == (1, None, (3, p.node_limit) + tuple(kw[k] for k in NAMES))
