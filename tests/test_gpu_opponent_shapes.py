"""GPU: every shape of the budgeted opponent kernels once -- the 32 legal (QS, ORD, REP, POS, SEL, EXC) instantiations
of ``k_opponent_moves_id`` and ``k_reply_opponent_id`` (csrc/opponent.hpp, ``opp_shape_legal``) -- each against the CPU
restatement its own test file uses: ``evaluation_util.search`` for the sixteen full-width shapes,
``selective_util.search`` for SEL without EXC, ``exchange_util.search`` for EXC.

1. ``Context.opponent_moves`` on four roots, maximum depth 3 under 200 nodes, 2 quiescence plies where QS: two roots
   with a history (REP has something to read) and two hand-made exchange positions (SEL / EXC have something to prune);
   the five output arrays equal the restatement, element for element.
2. ``LockstepEngine(reply=MinimaxPlayer(...))``, eager, 8 simulations on 4 roots: the trees and the three accumulators
   equal ``oracle.mcts_oracle.search`` whose mover is the shape's ``ReplyAgent*`` restatement.
Without a GPU: the roots are searched (no row is skipped) and the options reach them.  Integer work: all exact.
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import mcts_oracle
from tests import evaluation_util as ev
from tests import exchange_util as xu
from tests import opponent_reply_util as u
from tests import opponent_util as ou
from tests import repetition_util as rp
from tests import selective_util as su

DEPTH, Q, BUDGET, SIMS = 3, 2, 200, 8
FLAGS = ("QS", "ORD", "REP", "POS", "SEL", "EXC")
# the rule restated: SEL needs ORD, EXC needs ORD and QS
SHAPES = [s for s in itertools.product((False, True), repeat=6)
          if (s[1] or not s[4]) and ((s[1] and s[0]) or not s[5])]
HISTORY_ROOTS = ("kqk_black", "kqk_white")
EXCHANGE_ROOTS = ("xrays_both_sides", "king_may_not_capture")
# a random prefix of 9 plies (a history), the two promotion races and the fifty-move claim: few pieces, so that the
# restated positional evaluation of 32 replies per shape stays within a few seconds
REPLY_ROOTS = (1, u.FEN0 + 2, u.FEN0 + 3, u.FEN0 + 5)


def shape_id(shape):
    return "-".join(n for n, on in zip(FLAGS, shape) if on) or "plain"


def keywords(shape):
    """The keywords of ``Context.opponent_moves`` / ``MinimaxPlayer`` that launch this shape."""
    qs, ordering, rep, pos, sel, exc = shape
    return dict(quiescence=Q if qs else 0, node_budget=BUDGET, ordering=ordering, repetition=rep,
                evaluation="positional" if pos else "material", selective=sel, exchange=exc)


@functools.lru_cache(maxsize=None)
def roots():
    named = dict(rp.history_games() + xu.hand_made_games())
    return tuple(named[n] for n in HISTORY_ROOTS + EXCHANGE_ROOTS)


def restated(shape, game):
    """(move, score, nodes, flag, depth_done) of the shape's search of ``game`` by the restatement of its rule set."""
    kw = keywords(shape)
    if kw["exchange"]:
        return xu.search(game, DEPTH, BUDGET, kw["quiescence"], kw["repetition"], kw["evaluation"], kw["selective"], True)
    if kw["selective"]:
        return su.search(game, DEPTH, BUDGET, kw["quiescence"], kw["repetition"], kw["evaluation"], True)
    return ev.search(game, DEPTH, BUDGET, kw["quiescence"], kw["ordering"], kw["repetition"], kw["evaluation"])


@functools.lru_cache(maxsize=None)
def reference(shape):
    """The restated rows of the four roots: computed once, never changed."""
    return tuple(restated(shape, g) for g in roots())


def reply_agent(shape):
    kw = keywords(shape)
    if kw["exchange"]:
        return xu.ReplyAgentExc(u.net(), DEPTH, BUDGET, kw["quiescence"], kw["repetition"], kw["evaluation"],
                                kw["selective"], True)
    if kw["selective"]:
        return su.ReplyAgentSel(u.net(), DEPTH, BUDGET, kw["quiescence"], kw["repetition"], kw["evaluation"], True)
    return ev.ReplyAgentEv(u.net(), DEPTH, BUDGET, kw["quiescence"], kw["ordering"], kw["repetition"], kw["evaluation"])


def test_the_shapes_and_their_roots():
    """No GPU.  32 shapes; every root has a row in all of them; each flag changes the row of some root."""
    assert len(SHAPES) == 32 and len(set(SHAPES)) == 32
    for shape in SHAPES:
        for row in reference(shape):
            assert row is not None and row[0] != ou.NO_MOVE and row[2] > 0 and row[3] != ou.SKIPPED, shape_id(shape)
            assert row[2] <= BUDGET
    for bit in range(6):                                        # the flag's two settings differ where both are legal
        pairs = [(s, s[:bit] + (False,) + s[bit + 1:]) for s in SHAPES if s[bit]]
        assert any(off in SHAPES and reference(on) != reference(off) for on, off in pairs), FLAGS[bit]


@pytest.fixture(scope="module")
def ctx4():
    from chessrl_amd import _lib
    ctx = _lib.Context(len(roots()), 1, max_plies=64)
    u.load_games(ctx, roots())
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_opponent_moves_of_the_shape_equals_its_restatement(ctx4, shape):
    got = ctx4.opponent_moves(np.full(len(roots()), DEPTH, np.int32), push=False, **keywords(shape))
    assert len(got) == 5
    want = reference(shape)
    for k, (arr, dtype) in enumerate(zip(got, (np.uint16, np.int32, np.int64, np.uint8, np.int32))):
        assert arr.dtype == dtype
        assert [int(x) for x in arr] == [row[k] for row in want], (shape_id(shape), k)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_reply_trees_of_the_shape_equal_its_restatement(shape):
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.opponent import MinimaxPlayer
    games = [u.roots()[i] for i in REPLY_ROOTS]
    eng = LockstepEngine(u.net().to("cuda:0"), n_games=len(games), max_sims=SIMS,
                         reply=MinimaxPlayer(False, DEPTH, **keywords(shape)), numpy_promotion="nep50", use_graph=False)
    try:
        u.load_games(eng.ctx, games)
        eng.search(SIMS)
        rc = eng.root_children()
        nodes, cuts, depth_sum = eng.reply_stats()
    finally:
        eng.close()
    for i, g in enumerate(games):
        agent = reply_agent(shape)
        r = mcts_oracle.search(g, agent, SIMS, noise=False, mode="nep50")
        u.assert_tree_equal(rc, i, r, shape_id(shape))
        log = agent.log
        want = (sum(e[2] for e in log), sum(1 for e in log if e[3] == ou.CUT), sum(e[4] for e in log))
        assert (int(nodes[i]), int(cuts[i]), int(depth_sum[i])) == want, (shape_id(shape), i)
