"""The restatement of the built-in opponent's selective search (tests/selective_util.py; csrc/opponent.hpp SELECTIVE)
held to the existing restatements and to its own rule, without a GPU.

1. with ``selective`` off it is the search of ``evaluation_util`` / ``repetition_util`` / ``ordering_util``, output for
   output;
2. with a maximum depth <= 2 no node has r >= 3 and none below the root r >= 2: every output, the node count included,
   equals the ordered search without the section;
3. the cases of the GPU test reach every branch of the rule, the hand-made roots the branches they were made for;
4. every budget from 1 up to the whole search of two small positions gives a legal move, a consistent flag and
   completed depth, and never more nodes than the budget;
5. the node sums over the 19 roots of ``ordering_util.games()`` at depths 3 and 4, pinned.
"""
import pytest

from tests import evaluation_util as ev
from tests import opponent_util as ou
from tests import ordering_util as od
from tests import selective_util as su

BIG = su.UNREACHED
NAMES = [name for name, _ in su.games()]


def named(name):
    return dict(su.games())[name]


# ---- 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,quiescence,budget,repetition,evaluation",
                         [(2, 0, 200, False, "material"), (3, 2, 300, True, "positional"),
                          (3, 0, 150, True, "material"), (3, 2, 200, False, "positional")])
def test_selective_off_is_the_existing_restatement(depth, quiescence, budget, repetition, evaluation):
    assert len(su.games()) == 28 + len(su.HAND_MADE)
    cut = 0
    for name, g in su.games():
        mine = su.search(g, depth, budget, quiescence, repetition, evaluation, selective=False)
        theirs = ev.search(g, depth, budget, quiescence, True, repetition, evaluation)
        assert mine == theirs, name
        cut += mine[3] == ou.CUT
    assert 0 < cut < len(su.games())                            # budgets that cut and budgets that do not


# ---- 2 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quiescence", [0, 2])
@pytest.mark.parametrize("evaluation", ["material", "positional"])
@pytest.mark.parametrize("repetition", [False, True])
def test_shallow_depths_do_not_change(quiescence, evaluation, repetition):
    finished = 0
    for name, g in su.games():
        budget = 250 if name == su.BIG_ROOT or quiescence else BIG         # (an unreached budget where that is quick)
        for depth in (1, 2):
            counts = su.new_counts()
            on = su.search(g, depth, budget, quiescence, repetition, evaluation, counts=counts)
            off = ev.search(g, depth, budget, quiescence, True, repetition, evaluation)
            assert on == off, (name, depth)
            taken = [k for k, v in counts.items() if v and "refused" not in k]
            assert not taken, (name, depth, taken)              # no null move, no reduction
            finished += on[3] == 0
    assert finished >= len(su.games())


# ---- 3 ---------------------------------------------------------------------------------------------------------
def test_the_gpu_set_reaches_every_branch():
    total = su.new_counts()
    nodes = 0
    assert len(su.CASES) >= 8 and {c[0] for c in su.CASES} == {3, 4, 5}
    assert {(q > 0, rep, kind) for _, q, _, rep, kind in su.CASES} == {
        (q, rep, kind) for q in (False, True) for rep in (False, True) for kind in ("material", "positional")}
    for case in su.CASES:
        depth, quiescence, budget, repetition, evaluation = case
        rows, counts = su.reference(*case)
        for (name, g), row in zip(su.games(), rows):
            assert (row is None) == (not su.in_case(name, case)), name
            if row is None:
                continue
            move, score, n, flag, done = row
            assert move in g.legal_move_ids() and n <= budget and (flag == ou.CUT) == (done < depth), name
        nodes += sum(r[2] for r in rows if r is not None)
        for k, v in counts.items():
            total[k] += v
        print(case, counts)
    print("nodes of the GPU set:", nodes, total)
    assert nodes < 60000                                        # a few ten thousand nodes in all
    for branch in su.BRANCHES:
        assert total[branch] > 0, branch
    assert total["null_cut"] > total["null_cut_capped"] and total["reduction_holds"] > total["reduction_researched"]


def test_hand_made_roots_reach_what_they_are_for():
    c = su.new_counts()
    su.search(named("pawns_only"), 4, BIG, 0, False, "material", counts=c)
    assert c["null_refused_no_piece"] > 0 and c["null_cut"] == c["null_failed"] == 0
    c = su.new_counts()
    row = su.search(named("mate_window"), 3, BIG, 0, False, "material", counts=c)
    assert row[1] == ou.MATE - 1 and c["null_refused_mate_beta"] > 0
    c = su.new_counts()
    g = named("capped_cut")
    depth, quiescence, budget, repetition, evaluation = su.CAPPED_CASE
    assert su.CAPPED_CASE in su.CASES and su.in_case("capped_cut", su.CAPPED_CASE)
    row = su.search(g, depth, budget, quiescence, repetition, evaluation, counts=c)
    print("capped_cut", row, c)
    assert row[3:] == (0, depth) and row[2] < budget            # the case's budget lets it finish
    assert c["null_cut_capped"] == 1 and c["null_cut"] > 1


# ---- 4 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,depth,quiescence,evaluation", [("fen_2", 4, 0, "material"), ("kbkn", 3, 2, "positional")])
def test_every_budget_of_a_small_position(name, depth, quiescence, evaluation):
    g = named(name)
    legal = g.legal_move_ids()
    counts = su.new_counts()
    whole = su.search(g, depth, BIG, quiescence, True, evaluation, counts=counts)
    total, last_done = whole[2], 0
    assert 50 < total < 400 and whole[3:] == (0, depth)
    assert counts["null_cut"] + counts["null_failed"] > 0 and counts["reduction_holds"] > 0
    for budget in range(1, total + 2):
        move, score, nodes, flag, done = su.search(g, depth, budget, quiescence, True, evaluation)
        assert move in legal and nodes == min(budget, total), budget
        assert last_done <= done <= depth, budget
        assert (flag == ou.CUT) == (done < depth) == (budget < total), budget
        if budget >= total:
            assert (move, score, nodes, flag, done) == whole
        last_done = done
    assert su.search(g, depth, 1, quiescence, True, evaluation) == (legal[0], -ou.INF, 1, ou.CUT, 0)


# ---- 5 ---------------------------------------------------------------------------------------------------------
# nodes over the 19 roots of ``ordering_util.games()`` with the material evaluation, no quiescence, no repetition rule
# and a budget nothing reaches: (full width, selective), as this restatement measured them
NODE_SUMS = {3: (18717, 4559), 4: (61088, 27133)}


@pytest.mark.parametrize("depth", [3, 4])
def test_node_sums(depth):
    assert len(od.games()) == 19
    full = selective = 0
    for name, g in od.games():
        a = su.search(g, depth, 10 ** 7, selective=False)
        b = su.search(g, depth, 10 ** 7)
        assert a[3:] == b[3:] == (0, depth), name
        if depth == 3:
            assert a == od.ordered(g, depth, 10 ** 7), name
        full, selective = full + a[2], selective + b[2]
    print("depth", depth, "full width", full, "selective", selective)
    assert (full, selective) == NODE_SUMS[depth]
    assert selective < full                                     # (at depth 4: the point of the rules)
