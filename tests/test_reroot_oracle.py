"""CPU: the continuation oracle of tests/reroot_util.py against tests/golden/reroot_cases.json -- the reference's
own ``SelfPlayTree(Node)`` runs (tools/make_golden_reroot.py) -- and the C-ABI of the re-rooting entry points."""
import os
import re

import numpy as np

from oracle import mcts_oracle
from oracle.make_golden import f64hex
from tests import reroot_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_holds_the_cases_the_feature_is_judged_on():
    cases = ru.load_cases()
    assert len(cases) >= 16 and {c["mode"] for c in cases} == {"nep50", "legacy"}
    hops = [s for c in cases for s in c["stages"][1:]]
    assert sum(len(c["stages"]) == 3 for c in cases) >= 8                        # two successive hops
    assert any(s["kept_children"] < s["kept_legal_moves"] for s in hops)         # into a child not fully expanded
    assert any(s["kept_children"] < s["kept_legal_moves"] and s["root_fully_expanded"] for s in hops)   # ... filled up after
    assert any(s["kept_terminal_on_our_move"] and s["kept_terminal_after_reply"] for s in hops)  # both terminal kinds kept
    assert any(s["noise_seed"] is not None for s in hops)
    assert any(s["policy_sum"] > 1.5 for s in hops)                              # the compute_policy quirk is in the data
    by_name = {}
    for c in cases:
        by_name.setdefault(c["name"], {})[c["mode"]] = [s["visits"] for s in c["stages"]]
    assert any(v["nep50"] != v["legacy"] for v in by_name.values())              # the promotion mode matters somewhere


def test_continuation_oracle_equals_the_reference_on_every_case():
    """Bit for bit: visits, value sums, priors, moves, replies, root visits, node counts, the un-normalised
    policy and the child it selects, over one and two hops."""
    for c in ru.load_cases():
        agent = mcts_oracle.OracleAgent(ru.case_net(c), widen_priors=(c["mode"] == "legacy"))
        root = ru.new_root(ru.case_game(c))
        for i, st in enumerate(c["stages"]):
            if i:
                root = ru.reroot(root, c["stages"][i - 1]["chosen"])
                assert ru.count(root) == st["kept_nodes"] and len(root.kids) == st["kept_children"]
                assert root.visits == 1
            ru.grow(root, agent, st["sims"], c["mode"])
            got = ru.root_stats(root)
            for k in ("visits", "values", "priors", "moves", "replies", "root_visits", "n_nodes"):
                assert got[k] == st[k], (c["name"], c["mode"], i, k)
            assert len(root.state) == st["root_plies"]
            pol = ru.stage_policy(got, st["root_plies"], st["noise_seed"])
            assert [f64hex(p) for p in pol] == st["policy"], (c["name"], c["mode"], i)
            assert int(np.argmax(pol)) == st["chosen"]


def test_keep_or_fresh_rule_reuses_and_falls_back_on_the_whole_game_inputs():
    """The inputs of the whole-game GPU test, agent as white from the standard position, S = 60, 121 nodes:
    the oracle keeps the tree on most moves and falls back on some (both must happen for the GPU test to mean
    anything)."""
    from oracle.fakenet import FakeNet
    r = ru.play_game_reuse(mcts_oracle.OracleAgent(FakeNet(seed=9, prior_shift=24)), 60, 121, moves=24)
    assert (r["kept"], r["fell_back"]) == (17, 7)
    assert all(k + 60 <= 121 for k in r["kept_nodes"])


def test_library_exports_the_reroot_entry_points():
    from chessrl_amd import _lib
    text = open(os.path.join(ROOT, "include", "chessrl_hip.h")).read()
    L = _lib.lib()
    for name in ("crl_reroot", "crl_reroot_fetch", "crl_search_begin_kept", "crl_copy_game_tree", "crl_fetch_tree"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.crl_abi_version() == _lib.ABI_VERSION == 9
    assert int(re.search(r"#define CRL_ABI_VERSION (\d+)", text).group(1)) == 9
