"""CPU: the wave schedule (``threads`` > 1 with virtual loss) restated in tests/wave_util.py equals
tests/golden/wave_cases.json -- the reference's own select / simulate / backprop driven in that schedule -- bit for
bit, and with one thread it IS the sequential search of oracle/mcts_oracle.py.  Plus the host-side refusals of the
wave mode that need no GPU."""
import numpy as np
import pytest

from oracle import mcts_oracle
from tests import wave_util as wu

CASES = wu.load_cases()
KEYS = ("visits", "values", "priors", "moves", "replies", "root_visits", "n_nodes", "waves", "policy", "chosen", "bm", "am")


@pytest.mark.parametrize("ci", range(len(CASES)), ids=["%s-%s" % (c["name"], c["mode"]) for c in CASES])
def test_restatement_equals_the_reference_driven_in_the_wave_schedule(ci):
    c = CASES[ci]
    assert [r["threads"] for r in c["runs"]] == list(wu.THREADS)
    g = wu.case_game(c)
    for r in c["runs"]:
        agent = mcts_oracle.OracleAgent(wu.case_net(c), widen_priors=(c["mode"] == "legacy"))
        _, st = wu.wave_search(g, agent, c["sims"], r["threads"], c["mode"])
        for k in KEYS:
            assert st[k] == r[k], (c["name"], c["mode"], r["threads"], k)
        assert sum(r["waves"]) == c["sims"] and r["root_visits"] == c["sims"] + 1


def test_every_event_class_occurs_in_the_fixture():
    ev = {}
    for c in CASES:
        for r in c["runs"]:
            for k, v in r["events"].items():
                ev[k] = ev.get(k, 0) + v
    assert set(ev) == {"short_waves", "partial_last_wave", "visits0_sibling_scored",
                       "terminal_child_scored_with_vloss", "parent_full_mid_wave"}
    assert all(v > 0 for v in ev.values()), ev
    for c in CASES:                                                     # short waves at T = 64 everywhere
        assert c["runs"][-1]["events"]["short_waves"] > 0
        assert c["runs"][1]["events"]["visits0_sibling_scored"] > 0     # a visits-0 sibling is scored at T = 6


@pytest.mark.parametrize("ci", [0, 6, 10], ids=lambda i: "%s-%s" % (CASES[i]["name"], CASES[i]["mode"]))
def test_one_thread_is_the_sequential_search(ci):
    c = CASES[ci]
    g = wu.case_game(c)
    wide = c["mode"] == "legacy"
    _, st = wu.wave_search(g, mcts_oracle.OracleAgent(wu.case_net(c), widen_priors=wide), 60, 1, c["mode"])
    ref = mcts_oracle.search(g, mcts_oracle.OracleAgent(wu.case_net(c), widen_priors=wide), 60, noise=False, mode=c["mode"])
    assert st["waves"] == [1] * 60
    assert st["visits"] == ref.visits and st["root_visits"] == ref.root_visits and st["n_nodes"] == ref.n_nodes
    assert st["values"] == [wu.f64hex(v) for v in ref.values] and st["priors"] == [wu.f32hex(p) for p in ref.priors]
    assert st["moves"] == ref.child_moves and st["chosen"] == ref.chosen
    assert (st["bm"], st["am"]) == tuple(ref.moves)
    assert st["policy"] == [wu.f64hex(p) for p in ref.policy]


def test_more_threads_give_another_tree():
    """A test at T > 1 cannot pass on a search that ignores ``threads``."""
    for c in CASES:
        if c["name"] == "one_move_root":
            continue
        seq = mcts_oracle.search(wu.case_game(c), mcts_oracle.OracleAgent(wu.case_net(c), widen_priors=(c["mode"] == "legacy")),
                                 c["sims"], noise=False, mode=c["mode"])
        for r in c["runs"]:
            assert (r["visits"], r["values"]) != (seq.visits, [wu.f64hex(v) for v in seq.values]), (c["name"], r["threads"])


# ---- host refusals that need no GPU -------------------------------------------------------------------------------
def test_engine_refuses_what_waves_do_not_support_before_touching_the_gpu():
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.simulation import Rollouts
    net = object()
    with pytest.raises(ValueError, match="threads must lie in"):
        LockstepEngine(net, n_games=4, max_sims=10, threads=0)
    with pytest.raises(ValueError, match="threads must lie in"):
        LockstepEngine(net, n_games=4, max_sims=10, threads=65)
    with pytest.raises(ValueError, match="rollouts"):
        LockstepEngine(net, n_games=4, max_sims=10, threads=6, simulate=Rollouts(repetitions=2, max_moves=10, seed=1))
    with pytest.raises(ValueError, match="legal_priors"):
        LockstepEngine(net, n_games=4, max_sims=10, threads=6, legal_priors=True)
    with pytest.raises(ValueError, match="raw_priors"):
        LockstepEngine(net, n_games=4, max_sims=10, threads=6, raw_priors=True)
    with pytest.raises(ValueError, match="max_nodes"):
        LockstepEngine(net, n_games=4, max_sims=10, threads=6, max_nodes=40)


def test_runner_and_tree_refuse_wave_combinations_on_the_host():
    from chessrl_amd.mctree import Node, SelfPlayTree
    from chessrl_amd.selfplay import SelfPlayRunner
    from chessrl_amd.simulation import Rollouts
    with pytest.raises(ValueError, match="reuse_tree"):
        SelfPlayRunner(object(), n_parallel=4, sims=10, threads=6, reuse_tree=True, tree_nodes=40)
    with pytest.raises(ValueError, match="threads"):
        SelfPlayRunner(object(), n_parallel=4, sims=10, threads=0)
    kept = Node(None, 3, 0.5, 0.1, "e2e4", "e7e5", tree=object(), index=0)
    kept._state = object()
    with pytest.raises(ValueError, match="virtual_loss"):
        SelfPlayTree(kept, threads=6, virtual_loss=True)
    with pytest.raises(ValueError, match="rollouts"):
        SelfPlayTree(kept, threads=6, virtual_loss=True, simulate=Rollouts(repetitions=2, max_moves=10, seed=1))


def test_cli_flag_makes_threads_effective():
    from chessrl_amd import selfplay
    p = selfplay.build_parser()
    a = p.parse_args(["models"])
    assert a.virtual_loss is False
    b = p.parse_args(["models", "--threads", "6", "--virtual-loss"])
    assert b.virtual_loss is True and b.threads == 6
    assert selfplay.effective_threads(a) == 1 and selfplay.effective_threads(b) == 6
    assert "virtual-loss" in p.format_help()
