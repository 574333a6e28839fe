"""The cells of tests/test_gpu_search_combinations.py, as far as they can be checked without a GPU:

1. the generated cells are the askable subsets of ``chessrl_amd.searchmode.COVERS`` -- nothing hand-written;
2. every combination of capabilities is either parametrised into the GPU file or refused by ``SearchMode``;
3. the oracle runs the cells are compared with are complete (8 slots x 3 moves, no game ends early) and satisfy the
   conditions that keep a cell from passing vacuously: kept trees and fall-backs, a terminal node inside a kept
   subtree, a playout from a kept-tree leaf that ends on the fifth occurrence of a position of the root's own
   history, rollout trees that differ from value-head trees in every slot, a quarter of the playouts ended by a rule;
4. ``LegalFakeNet`` expands plane bitboards to the planes they stand for.
"""
import collections
import itertools

import numpy as np
import pytest

from chessrl_amd.searchmode import COVERS, SearchMode
from tests import combination_util as cu
from tests.test_search_modes_cpu import CAPABILITIES, HOWS

EVERY_CAPABILITY = sorted(set(CAPABILITIES) | set(cu.HELD) | set().union(*COVERS.values()))


def subsets(names):
    names = sorted(names)
    return [frozenset(c) for n in range(len(names) + 1) for c in itertools.combinations(names, n)]


def gpu_cells():
    """The cells tests/test_gpu_search_combinations.py::test_cell_equals_the_oracle is parametrised with."""
    from tests import test_gpu_search_combinations as gpu
    marks = [m for m in gpu.test_cell_equals_the_oracle.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[0] == "cell"
    return list(marks[0].args[1])


# ---- 1, 2 --------------------------------------------------------------------------------------------------------
def test_the_generated_cells_are_the_askable_subsets_of_the_table():
    for kind, covered in COVERS.items():
        want = {s for s in subsets(covered) if "raw_priors" not in s or "legal_priors" in s}
        got = cu.cells(kind)
        assert len(got) == len(set(got)) == len(want)
        assert {c.caps for c in got} == want and all(c.kind == kind for c in got)
        assert got[0].caps == frozenset()                        # the bare mode
    assert len({cu.cell_id(c) for c in cu.all_cells()}) == len(cu.all_cells())


def test_every_combination_is_parametrised_into_the_gpu_file_or_refused():
    placed = gpu_cells()
    assert len(placed) == len(set(placed))
    for kind in COVERS:
        mode = SearchMode(**cu.mode_args(kind))
        assert mode.kind == kind
        for caps in subsets(EVERY_CAPABILITY):
            refused = []
            for cap in caps:
                try:
                    mode.require(cap, HOWS[cap][0])
                except ValueError:
                    refused.append(cap)
            assert sorted(refused) == sorted(caps - COVERS[kind])
            if refused or not cu.askable(caps):
                assert cu.Cell(kind, caps) not in placed
            else:
                assert cu.Cell(kind, caps) in placed, "no GPU test for %s" % cu.cell_id(cu.Cell(kind, caps))
    for cell in placed:                                          # ... and each placed cell is one the runner can ask for
        assert not cu.unheld(cell), "no test holds %s to the oracle yet" % cu.unheld(cell)
        assert cu.oracle_key(cell)[0] in ("leaf", "wave", "opponent")
    formats = [cu.bitplanes_of(c) for c in placed]
    assert formats == [bool(i & 1) for i in range(len(placed))]  # the plane formats alternate


# ---- 3 -----------------------------------------------------------------------------------------------------------
RUNS = sorted({cu.oracle_key(c) for c in cu.all_cells()})


def test_the_roots_are_what_they_were_chosen_for():
    roots = cu.roots()
    assert len(roots) == cu.G and all(g.get_result() is None for g in roots)
    assert [len(g) for g in roots[:cu.N_PREFIX]] == [0, 30, 60]
    shuffle = roots[cu.SHUFFLE_SLOT]
    assert shuffle.repetitions() == 4 and len(shuffle.legal_move_ids()) == 3
    assert (len(roots[cu.CLAIM_SLOT]), cu.clock(roots[cu.CLAIM_SLOT])) == (0, 94)
    assert [cu.clock(roots[i]) for i in cu.CLOCK_SLOTS] == list(cu.QUIET_CLOCKS)
    assert all(len(roots[i]) >= cu.clock(roots[i]) >= 88 for i in cu.CLOCK_SLOTS)      # the history is the game's own
    assert len(roots[cu.CLOCK_SLOTS[0]]) > 200


@pytest.mark.parametrize("key", RUNS, ids=lambda k: "%s-reuse%d-rollouts%d" % (k[0], k[1], k[2]))
def test_the_oracle_run_is_complete_and_not_vacuous(key):
    kind, reuse, rollouts = key
    run = cu.oracle_run(*key)
    # no slot and no move is skipped: the comparison covers 8 slots x 3 moves
    assert all(st is not None and len(st["visits"]) > 0 for row in run["stats"] for st in row)
    assert all(pair is not None for row in run["pairs"] for pair in row)
    assert run["sims"] == cu.G * cu.MOVES * cu.SIMS
    kept = [n for row in run["kept"] for n in row]
    if not reuse:
        assert not any(kept)
    else:
        assert any(kept) and not all(kept)                       # slots that keep their tree and slots that fall back
        assert any(0 < n < cu.SIMS for n in kept)
        assert run["kept_terminal"]                              # a terminal node inside a kept subtree
    if rollouts:
        plain = cu.oracle_run(kind, reuse, False)
        assert cu.differing_slots(run, plain) == list(range(cu.G))
        assert all(run["stats"][0][i] != plain["stats"][0][i] for i in range(cu.G))
        ended = collections.Counter(r for row in run["reasons"] for slot in row for r in slot)
        total = sum(ended.values())
        assert total > 0 and 4 * (total - ended["cut"]) >= total, ended
        assert ended["fifty"] and ended["mate"] and ended["fivefold"] and ended["insufficient"], ended
    if reuse and rollouts:
        # a playout from a leaf of a KEPT tree ends on a fifth occurrence: four of them are in the root's own history
        s = cu.SHUFFLE_SLOT
        assert any(run["kept"][mv - 1][s] and "fivefold" in run["reasons"][mv][s] for mv in range(1, cu.MOVES))


# ---- 4 -----------------------------------------------------------------------------------------------------------
def test_legal_fakenet_expands_plane_bitboards():
    import torch
    from tests.test_gpu_search import _bits_from_planes
    rng = np.random.default_rng(5)
    planes = torch.from_numpy((rng.random((5, 8, 8, 128)) < 0.3).astype(np.float16))
    planes[0, 0, 0, :] = 1                                       # square 56: bit 63 of every plane but the padding
    planes[..., 127] = 0
    net = cu.LegalFakeNet(cu.fakenet(), bitplanes=True)
    assert net.accepts_bitplanes and net.accepts_legal_labels and not hasattr(net, "raw_priors_supported")
    back = net._planes(_bits_from_planes(planes))
    assert back.shape == planes.shape and torch.equal(back, planes.to(torch.int64))
    pol, val = net(_bits_from_planes(planes))
    ref_pol, ref_val = cu.fakenet()(planes)
    assert torch.equal(pol, ref_pol) and torch.equal(val, ref_val)
    assert net._planes(planes) is planes                         # fp16 planes pass through
