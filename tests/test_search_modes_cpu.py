"""``chessrl_amd.searchmode``: the one statement of which search options combine, and every layer that asks it.

No device is touched: the net is ``object()``, engines whose methods are driven come from ``__new__``.
"""
import pytest

from chessrl_amd import selfplay
from chessrl_amd.agent import Agent
from chessrl_amd.engine import (LockstepEngine, REPLY_REFUSED, StampRing, STAMP_REPLIED, STAMP_ROLLOUT, STAMP_S1_DONE,
                                STAMP_SELECTED, STAMP_STEP)
from chessrl_amd.mctree import Node, SelfPlayTree, Tree
from chessrl_amd.opponent import MinimaxPlayer
from chessrl_amd.searchmode import COVERS, REFUSED, SearchMode
from chessrl_amd.selfplay import SelfPlayRunner
from chessrl_amd.simulation import Rollouts

KINDS = ("leaf", "wave", "opponent")
CAPABILITIES = ("tree_reuse", "stamps", "legal_priors", "raw_priors", "rollouts")
HOWS = {"tree_reuse": ("max_nodes", "keep_root", "reroot", "node", "reuse_tree"), "stamps": ("set_stamps",),
        "legal_priors": ("legal_priors",), "raw_priors": ("raw_priors",), "rollouts": ("simulate",)}
ROLL = Rollouts(repetitions=2, max_moves=10, seed=1)
PLAYER = MinimaxPlayer(False, 2)
MODE_ARGS = {"leaf": {}, "wave": {"threads": 6}, "opponent": {"reply": PLAYER}}

LEAF_PLAN = [(STAMP_STEP, "phase_select_expand"), (STAMP_SELECTED, "phase_tower_s1"), (STAMP_S1_DONE, "phase_reply"),
             (STAMP_REPLIED, "phase_tower_s2")]
LEAF_ROLLOUT_PLAN = [(STAMP_STEP, "phase_select_expand"), (STAMP_SELECTED, "phase_tower_s1"), (STAMP_S1_DONE, "phase_reply"),
                     (STAMP_REPLIED, "phase_tower_s2"), (STAMP_ROLLOUT, "phase_rollout")]
WAVE_PLAN = [(STAMP_STEP, "phase_select_expand"), (STAMP_SELECTED, "phase_tower_s1"), (STAMP_S1_DONE, "phase_reply"),
             (STAMP_REPLIED, "phase_tower_s2")]
OPPONENT_PLAN = [(STAMP_STEP, "phase_select_expand"), (STAMP_S1_DONE, "phase_reply_opponent"),
                 (STAMP_REPLIED, "phase_tower_s2")]
ONE_LEAF = ("sim_select_expand", "sim_reply", "sim_backup")


def test_the_table_is_the_one_the_design_states():
    assert set(COVERS) == set(KINDS)
    assert COVERS["leaf"] == set(CAPABILITIES) and COVERS["wave"] == set()
    assert COVERS["opponent"] == {"legal_priors", "raw_priors"}
    assert REPLY_REFUSED["threads"].startswith("reply= cannot be combined with threads > 1")
    assert all(REFUSED["opponent", how] is text for how, text in REPLY_REFUSED.items() if how != "threads")


@pytest.mark.parametrize("args, kind, plan, kernels, rows", [
    ({}, "leaf", LEAF_PLAN, ONE_LEAF, 1),
    ({"simulate": ROLL}, "leaf", LEAF_ROLLOUT_PLAN, ONE_LEAF, 1),
    ({"threads": 2}, "wave", WAVE_PLAN, ("wave_select", "wave_reply", "wave_backup"), 2),
    ({"threads": 64}, "wave", WAVE_PLAN, ("wave_select", "wave_reply", "wave_backup"), 64),
    ({"reply": PLAYER}, "opponent", OPPONENT_PLAN, ONE_LEAF, 1),
])
def test_plan_kernels_and_rows_of_every_kind(args, kind, plan, kernels, rows):
    mode = SearchMode(**args)
    assert mode.kind == kind and mode.plan == plan and mode.kernels == kernels
    assert mode.rows_per_game == mode.threads == rows
    assert mode.plan is not mode.plan                    # a fresh list: nobody edits another engine's step


def bare_engine(kind):
    """An engine of that kind with no device behind it: what its methods read before they touch one."""
    eng = LockstepEngine.__new__(LockstepEngine)
    eng.reply, eng.threads, eng.max_sims = MODE_ARGS[kind].get("reply"), MODE_ARGS[kind].get("threads", 1), 10
    return eng


def kept_node(tree=None):
    node = Node(None, 3, 0.5, 0.1, "e2e4", "e7e5", tree=tree or object(), index=0)
    node._state = object()
    return node


def node_held_by(kind):
    """A Node whose tree was last searched by an engine of that kind (a bare holder, as the tree reads it)."""
    class Holder(object):
        pass
    src, eng = Holder(), Holder()
    src._engine, eng._tree_owner = eng, src
    eng.reply, eng.threads = MODE_ARGS[kind].get("reply"), MODE_ARGS[kind].get("threads", 1)
    return kept_node(src)


def engine(kind, **kw):
    return LockstepEngine(object(), n_games=4, max_sims=10, **dict(MODE_ARGS[kind], **kw))


def tree_args(kind):
    return {"wave": {"threads": 6, "virtual_loss": True}, "opponent": {"reply": PLAYER}}[kind]


# (capability, the wording asked for) -> every entry that can ask a kind for it
ENTRIES = {
    ("tree_reuse", "max_nodes"): [lambda kind: engine(kind, max_nodes=40)],
    ("tree_reuse", "keep_root"): [lambda kind: bare_engine(kind).search_begin(keep_root=True),
                                  lambda kind: bare_engine(kind).search(10, keep_root=True)],
    ("tree_reuse", "reroot"): [lambda kind: bare_engine(kind).reroot([0, 0, 0, 0], 10)],
    ("tree_reuse", "node"): [lambda kind: Tree(node_held_by(kind))._continue_on_device(10)],
    ("tree_reuse", "tree:node"): [lambda kind: SelfPlayTree(kept_node(), **tree_args(kind))],
    ("stamps", "set_stamps"): [lambda kind: bare_engine(kind).set_stamps(StampRing.__new__(StampRing))],
    ("legal_priors", "legal_priors"): [lambda kind: engine(kind, legal_priors=True)],
    ("raw_priors", "raw_priors"): [lambda kind: engine(kind, raw_priors=True)],
    ("rollouts", "simulate"): [lambda kind: engine(kind, simulate=ROLL),
                               lambda kind: Agent(True, model=object()).engine_for(10, simulate=ROLL, **MODE_ARGS[kind])],
    ("rollouts", "tree:simulate"): [lambda kind: SelfPlayTree(kept_node(), simulate=ROLL, **tree_args(kind))],
}
REFUSED_CELLS = [(kind, cap) for kind in KINDS for cap in CAPABILITIES if cap not in COVERS[kind]]


@pytest.mark.parametrize("kind, capability", REFUSED_CELLS)
def test_every_entry_refuses_a_cell_the_table_refuses_with_the_table_s_message(kind, capability):
    asked = 0
    for (cap, how), calls in ENTRIES.items():
        if cap != capability:
            continue
        # the tree words the two wave refusals its own way; everything else is the (kind, how) message
        text = REFUSED.get((kind, how)) or REFUSED[kind, how.split(":")[-1]]
        for call in calls:
            with pytest.raises(ValueError) as e:
                call(kind)
            assert str(e.value) == text, (kind, how)
            asked += 1
    assert asked
    for how in HOWS[capability]:
        if (kind, how) in REFUSED:
            with pytest.raises(ValueError) as e:
                SearchMode(**MODE_ARGS[kind]).require(capability, how)
            assert str(e.value) == REFUSED[kind, how]


def test_the_tree_keeps_its_own_wording_for_waves():
    for how in ("node", "tree:node", "tree:simulate"):
        assert "virtual_loss" in REFUSED["wave", how]
    assert "fresh tree" in REFUSED["wave", "node"] and "fresh tree" in REFUSED["wave", "tree:node"]
    assert "rollouts" in REFUSED["wave", "tree:simulate"]
    assert REFUSED["wave", "simulate"].startswith("threads > 1 cannot be combined with rollouts")


def test_runner_and_cli_refuse_waves_with_tree_reuse(capsys):
    with pytest.raises(ValueError) as e:
        SelfPlayRunner(object(), n_parallel=4, sims=10, threads=6, reuse_tree=True, tree_nodes=40)
    assert str(e.value) == REFUSED["wave", "reuse_tree"]
    with pytest.raises(ValueError, match="threads must lie in"):
        SelfPlayRunner(object(), n_parallel=4, sims=10, threads=65)
    with pytest.raises(SystemExit) as e:
        selfplay.main(["models", "--virtual-loss", "--reuse-tree"])
    assert e.value.code == 2
    assert "--virtual-loss cannot be combined with --reuse-tree" in capsys.readouterr().err


@pytest.mark.parametrize("kind, capability", [(k, c) for k in KINDS for c in CAPABILITIES if c in COVERS[k]])
def test_require_returns_for_every_cell_the_table_allows(kind, capability):
    mode = SearchMode(**MODE_ARGS[kind])
    assert mode.covers(capability)
    for how in HOWS[capability] + ("tree:node", "tree:simulate"):
        assert mode.require(capability, how) is None


def test_allowed_entries_pass_the_refusals():
    """The same calls on a leaf mode get past the mode: they end at the first thing that needs a device."""
    assert SelfPlayTree(kept_node(), simulate=ROLL).mode.kind == "leaf"
    assert SelfPlayTree(kept_node(), threads=6).mode.kind == "leaf"          # threads without virtual_loss: one worker
    assert SelfPlayTree(kept_node(), threads=99).mode.threads == 1           # ... and not range-checked
    with pytest.raises(ValueError, match="threads must lie in"):
        SelfPlayTree(kept_node(), threads=99, virtual_loss=True)
    with pytest.raises(AttributeError):                                      # past the refusal: no ctx on a bare engine
        bare_engine("leaf").reroot([0, 0, 0, 0], 10)


def test_key_tells_apart_what_the_agent_s_cache_told_apart():
    key = lambda **kw: SearchMode(**kw).key
    hash(key(reply=PLAYER, threads=1))
    assert key(reply=MinimaxPlayer(False, 2)) == key(reply=MinimaxPlayer(True, 2))
    assert key(reply=MinimaxPlayer(False, 2, quiescence=2)) == key(reply=MinimaxPlayer(True, 2, quiescence=2))
    base = key(reply=MinimaxPlayer(False, 2, node_limit=1000, quiescence=1))
    assert base != key(reply=MinimaxPlayer(False, 3, node_limit=1000, quiescence=1))
    assert base != key(reply=MinimaxPlayer(False, 2, node_limit=1001, quiescence=1))
    assert base != key(reply=MinimaxPlayer(False, 2, node_limit=1000, quiescence=2))
    assert key() != key(threads=2) != key(threads=3)
    assert key() != key(reply=PLAYER)
    assert key(simulate=ROLL) == key(simulate=Rollouts(2, 10, 1))
    assert key() != key(simulate=ROLL) != key(simulate=Rollouts(2, 10, 2))
    assert key(simulate=ROLL) != key(simulate=Rollouts(3, 10, 1))
    assert key(simulate=ROLL) != key(simulate=Rollouts(2, 11, 1))


def test_a_call_that_breaks_several_rules_raises_the_first_as_before():
    for build in (SearchMode, lambda **kw: LockstepEngine(object(), n_games=4, max_sims=10, **kw),
                  lambda **kw: Agent(True, model=object()).engine_for(10, **kw)):
        with pytest.raises(ValueError) as e:
            build(reply=PLAYER, threads=2, simulate=ROLL)
        assert str(e.value) == REPLY_REFUSED["threads"]
        with pytest.raises(TypeError, match="MinimaxPlayer"):
            build(reply="stockfish", threads=2, simulate=ROLL)
        with pytest.raises(ValueError) as e:
            build(reply=PLAYER, simulate="playouts")                         # reply x simulate before simulate's type
        assert str(e.value) == REPLY_REFUSED["simulate"]
        with pytest.raises(TypeError, match="Rollouts"):
            build(threads=99, simulate="playouts")                           # simulate's type before the threads range
        with pytest.raises(ValueError, match="threads must lie in"):
            build(threads=0, simulate=ROLL)
        with pytest.raises(ValueError, match="threads must lie in"):
            build(threads=65, simulate=ROLL)
    with pytest.raises(ValueError) as e:                                     # the constructor's own order: priors, then nodes
        LockstepEngine(object(), n_games=4, max_sims=10, threads=6, legal_priors=True, raw_priors=True, max_nodes=40)
    assert str(e.value) == REFUSED["wave", "legal_priors"]
