"""GPU: games beyond ply 256 -- the wrap of the 256-entry ring of past positions (csrc/state.hpp: HIST_RING, read
through past_ref by the repetition rule, the encoder and the playouts) -- and the boundary of the move record
(max_plies), through every kernel that meets them at real game lengths: replay, push, rules, encoder, training
batches, copies, one-leaf search with advance and reroot, waves, playouts, the built-in opponent.

Inputs: tests/long_game_util.py (seeded walks, games that end by a fifth occurrence astride the wrap, late roots);
tests/test_long_games_cpu.py asserts what they were chosen for.  References: the CPU oracle and the CPU restatements
(tests/wave_util.py, tests/reroot_util.py, tests/rollout_util.py, tests/opponent_util.py).  Every comparison is
equality of ints, bit patterns or lists.  The comparisons are functions that RETURN what differs: the tests demand
an empty list, and the negative control -- the same positions loaded without their history -- demands that the same
functions report differences, so that the tests are known to read the ring and not only the current board.
"""
import collections
import functools

import numpy as np
import pytest

from oracle import encoder_oracle, mcts_oracle
from oracle.chess_oracle import NULL_MOVE, OracleGame, move_to_uci
from oracle.fakenet import FakeNet
from tests import long_game_util as lu
from tests import opponent_util as ou
from tests import reroot_util as rr
from tests import rollout_util as ru
from tests import wave_util as wu
from tests.util import oracle_row

pytestmark = pytest.mark.gpu

NO_MOVE, RESULT_NONE = 0xFFFF, 2
MODE = "nep50"
NET = FakeNet(seed=42, prior_shift=31)             # deep trees; the seed is one whose trees meet the fifth occurrence
SIMS, WAVE_SIMS, THREADS, STEP_SIMS = 120, 60, 6, 60
CAPACITY = r"\(-3\): game longer than max_plies"   # CRL_ERR_CAPACITY and the device error's name


def res_of(g):
    r = g.get_result()
    return RESULT_NONE if r is None else r


def hexes(a, kind):
    a = np.asarray(a)
    return [format(int(x), "016x" if kind == "f64" else "08x") for x in a.view(np.uint64 if kind == "f64" else np.uint32)]


def device_stats(rc, i):
    n = int(rc["nchild"][i])
    return {"visits": [int(v) for v in rc["visits"][i, :n]], "values": hexes(rc["values"][i, :n], "f64"),
            "priors": hexes(rc["priors"][i, :n], "f32"), "moves": [move_to_uci(m) for m in rc["moves"][i, :n]],
            "replies": [None if m == NO_MOVE else move_to_uci(m) for m in rc["replies"][i, :n]],
            "root_visits": int(rc["root_visits"][i])}


# ---- loading ---------------------------------------------------------------------------------------------------
def load(ctx, id_lists):
    """Slot i replays id_lists[i] from the start position in ONE crl_push_sequences launch; the other slots of the
    window stay at the start position."""
    ctx.reset_games()
    tbl = np.full((ctx.G, max(1, max(len(m) for m in id_lists))), NO_MOVE, np.uint16)
    cnt = np.zeros(ctx.G, np.int32)
    for i, m in enumerate(id_lists):
        tbl[i, :len(m)] = m
        cnt[i] = len(m)
    assert list(ctx.push_sequences(tbl, cnt)) == list(cnt)


def load_bare(ctx, games):
    """Slot i becomes the current position of games[i] WITHOUT its history (the negative control)."""
    ctx.reset_games()
    ctx.set_positions(np.stack([oracle_row(g) for g in games]))


def straddling_cut(extra):
    """The straddling games cut at L + extra: [(move ids loaded, move ids that follow)]."""
    out = []
    for L in lu.STRADDLE_L:
        ids = lu.ids_of(lu.straddling_fivefold(L))
        out.append((ids[:L + extra], ids[L + extra:]))
    return out


def late_cut():
    return [(list(r.ids[:r.cut]), list(r.ids[r.cut:])) for r in lu.late_roots()]


# ---- 1. replay and rules -----------------------------------------------------------------------------------------
def rules_differences(ctx, pairs, bare=False):
    """Slots 0 .. len(pairs)-1 hold the games after pairs[i][0] (``bare``: their positions only); pairs[i][1] is then
    pushed ply by ply.  At every ply: crl_results, crl_legal_moves (set and order), crl_get_positions rows and
    crl_records against the oracle.  Returns ([(slot, ply, what)], device results per step)."""
    games = [lu.replay(head) for head, _ in pairs]
    if bare:
        load_bare(ctx, games)
    else:
        load(ctx, [head for head, _ in pairs])
    record = [[] if bare else list(head) for head, _ in pairs]
    steps = max(len(tail) for _, tail in pairs)
    bad, trace = [], []
    for k in range(steps + 1):
        moves, counts = ctx.legal_moves()
        res, pos = ctx.results(), ctx.get_positions()
        rec, plies, rec_res = ctx.records()
        trace.append(res.copy())
        for i, g in enumerate(games):
            at = (i, len(g))
            if list(moves[i, :counts[i]]) != g.legal_move_ids():
                bad.append(at + ("legal moves",))
            if res[i] != res_of(g) or rec_res[i] != res_of(g):
                bad.append(at + ("result",))
            if not np.array_equal(pos[i], oracle_row(g)):
                bad.append(at + ("position",))
            if list(rec[i, :plies[i]]) != record[i]:
                bad.append(at + ("record",))
        if k == steps:
            break
        push = np.full(ctx.G, NO_MOVE, np.uint16)
        for i, (_, tail) in enumerate(pairs):
            if k < len(tail):
                push[i] = tail[k]
        ok = ctx.push_moves(push)
        for i, g in enumerate(games):
            if push[i] != NO_MOVE:
                if not (lu.push(g, push[i]) and ok[i] == 1):
                    bad.append((i, len(g), "push"))
                record[i].append(int(push[i]))
            elif ok[i] != 0:
                bad.append((i, len(g), "push of no move"))
    return bad, trace


@pytest.fixture(scope="module")
def ctx():
    from chessrl_amd._lib import Context
    c = Context(max_games=32, max_sims=1, max_plies=1024)
    yield c
    c.close()


def test_replay_and_rules_of_the_straddling_games(ctx):
    """Lists of 254 .. 524 moves in one crl_push_sequences launch, then the last three plies one by one: the result
    is 2 up to L + 15 and 0 at L + 16."""
    pairs = straddling_cut(13)
    assert sorted(len(h) + len(t) for h, t in pairs) == sorted(L + 16 for L in lu.STRADDLE_L) and min(len(h) for h, _ in pairs) == 254
    bad, trace = rules_differences(ctx, pairs)
    assert bad == []
    n = len(pairs)
    assert len(trace) == 4 and all((trace[k][:n] == RESULT_NONE).all() for k in range(3)) and (trace[3][:n] == 0).all()


def test_replay_and_rules_of_the_late_roots_played_on(ctx):
    pairs = late_cut()
    assert len(pairs) == 16 and max(len(t) for _, t in pairs) == lu.LATE_EXTRA
    bad, _ = rules_differences(ctx, pairs)
    assert bad == []


# ---- 2. the encoder ------------------------------------------------------------------------------------------------
def decode_bitplanes(raw):
    """uint64 [n][128] plane bitboards -> float32 [n, 8, 8, 128] (row 0 = rank 8), the decoding of
    test_encoder_matches_the_reference_encoder_vectors for all squares at once."""
    n = raw.shape[0]
    bits = (raw[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)          # [n][ch][sq]
    return bits.reshape(n, 128, 8, 8)[:, :, ::-1, :].transpose(0, 2, 3, 1).astype(np.float32)


class BothFormats(object):
    """crl_encode of a context's window in both plane formats."""

    def __init__(self, ctx):
        import torch
        self.ctx, dev = ctx, torch.device("cuda", 0)
        self.f16 = torch.zeros((ctx.G, 8, 8, 128), dtype=torch.float16, device=dev)
        self.bits = torch.zeros((ctx.G, 128), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)

    def read(self):
        self.ctx.set_plane_format(False)
        self.ctx.encode(self.f16.data_ptr())
        self.ctx.set_plane_format(True)
        self.ctx.encode(self.bits.data_ptr())
        self.ctx.set_plane_format(False)
        self.ctx.sync()
        return {"f16": self.f16.float().cpu().numpy(), "bits": decode_bitplanes(self.bits.cpu().numpy().view(np.uint64))}


def encoder_span(r):
    """Plies at which a late root is encoded: cut-8 .. cut+10, and 504 .. 520 across the second wrap."""
    return (min(r.cut - 8, 504), max(r.cut + 10, 520)) if r.cut > 500 else (r.cut - 8, r.cut + 10)


def plane_differences(ctx, pairs, bare=False):
    """As rules_differences, for crl_encode in both plane formats against encoder_oracle.get_game_state."""
    games = [lu.replay(head) for head, _ in pairs]
    if bare:
        load_bare(ctx, games)
    else:
        load(ctx, [head for head, _ in pairs])
    enc = BothFormats(ctx)
    steps = max(len(tail) for _, tail in pairs)
    bad = []
    for k in range(steps + 1):
        got = enc.read()
        for i, g in enumerate(games):
            want = encoder_oracle.get_game_state(g).astype(np.float32)
            for fmt, planes in got.items():
                if not np.array_equal(planes[i, :, :, :127], want) or planes[i, :, :, 127].any():
                    bad.append((i, len(g), fmt))
        if k == steps:
            break
        push = np.full(ctx.G, NO_MOVE, np.uint16)
        for i, (_, tail) in enumerate(pairs):
            if k < len(tail):
                push[i] = tail[k]
        ok = ctx.push_moves(push)
        assert all(lu.push(g, push[i]) and ok[i] == 1 for i, g in enumerate(games) if push[i] != NO_MOVE)
    return bad


def encoder_pairs():
    out = []
    for r in lu.late_roots():
        lo, hi = encoder_span(r)
        out.append((list(r.ids[:lo]), list(r.ids[lo:hi])))
    return out


def test_encoder_across_the_wrap_in_both_plane_formats(ctx):
    """Every late root from eight plies before its cut to ten plies after it: the eight history planes come from
    ring entries before the wrap, astride it and after it."""
    pairs = encoder_pairs()
    spans = [(len(h), len(h) + len(t)) for h, t in pairs]
    assert sum(lo <= 257 and hi >= 263 for lo, hi in spans) >= 8 and sum(lo <= 504 and hi >= 520 for lo, hi in spans) == 4
    assert plane_differences(ctx, pairs) == []


# ---- 3. training batches ---------------------------------------------------------------------------------------------
def oracle_samples(ids):
    """dataset.py:21-43 on the oracle: planes before every move and the label of the move played."""
    labels = {u: i for i, u in enumerate(encoder_oracle.get_uci_labels())}
    g, planes, idx = OracleGame(), [], []
    for m in ids:
        planes.append(encoder_oracle.get_game_state(g))
        idx.append(labels[move_to_uci(m)])
        assert lu.push(g, m)
    return np.stack(planes), np.array(idx), g.get_result()


@pytest.mark.parametrize("which", ["straddling", "natural"])
def test_training_batches_of_a_long_game(which):
    """DatasetGame + DataGameSequence(batch_size=1): every prefix of the game replayed in one k_push_seq launch and
    encoded; the samples beyond ply 256 read a ring that has wrapped."""
    import torch
    from chessrl_amd.dataset import DatasetGame
    from chessrl_amd.netencoder import DataGameSequence
    from chessrl_amd.records import GameRecord
    ids = lu.ids_of(lu.straddling_fivefold(241) if which == "straddling" else lu.natural_game())
    planes, idx, result = oracle_samples(ids)
    assert result is not None and len(ids) >= (257 if which == "straddling" else 301)
    n = len(ids)
    seq = DataGameSequence(DatasetGame([GameRecord(0, ids, result, True)]), batch_size=1)
    assert len(seq) == 1
    x, y, z = seq.device_batch(0)
    assert x.shape == (n, 8, 8, 128) and x.dtype == torch.float16 and not x[..., 127].any()
    got = x[..., :127].float().cpu().numpy()
    assert [i for i in range(n) if not np.array_equal(got[i], planes[i])] == []
    assert np.array_equal(y.cpu().numpy(), idx) and np.array_equal(z.cpu().numpy(), np.full(n, result, np.float32))
    xs, (yp, yv) = seq[0]
    assert xs.dtype == np.float64 and np.array_equal(xs, planes)
    assert np.array_equal(yp.argmax(1), idx) and (yp.sum(1) == 1).all() and np.array_equal(yv, np.full(n, float(result)))
    xf, (ypf, _) = DataGameSequence(seq.dataset, batch_size=1, random_flips=1.0)[0]
    assert np.array_equal(xf, np.stack([np.rot90(a, k=2) for a in planes])) and np.array_equal(ypf, yp)


# ---- 4. copies ---------------------------------------------------------------------------------------------------------
def copy_pairs():
    """A straddling game cut at L + 13 and a late root beyond the wrap, with what is played after the copy."""
    L = 250
    ids = lu.ids_of(lu.straddling_fivefold(L))
    r = lu.late_roots()[8]
    assert r.cut == 259
    return [(ids[:L + 13], ids[L + 13:]), (list(r.ids[:r.cut]), list(r.ids[r.cut:r.cut + 12]))]


def slot_differences(c, slots, games, records, planes=True):
    """Position, result, legal moves, record and planes of the given slots against oracle games."""
    bad = []
    moves, counts = c.legal_moves()
    res, pos = c.results(), c.get_positions()
    rec, plies, _ = c.records()
    got = BothFormats(c).read() if planes else None
    for s, g, want in zip(slots, games, records):
        if list(moves[s, :counts[s]]) != g.legal_move_ids() or res[s] != res_of(g) or not np.array_equal(pos[s], oracle_row(g)):
            bad.append((s, len(g), "state"))
        if list(rec[s, :plies[s]]) != list(want):
            bad.append((s, len(g), "record"))
        if planes and not all(np.array_equal(p[s, :, :, :127], encoder_oracle.get_game_state(g).astype(np.float32))
                              for p in got.values()):
            bad.append((s, len(g), "planes"))
    return bad


def test_copies_within_a_context_and_into_another_play_on_like_the_oracle(ctx):
    from chessrl_amd._lib import Context
    pairs = copy_pairs()
    src_slots, same_slots, other_slots = (5, 3), (9, 30), (2, 6)
    heads = [[]] * 32
    for s, (head, _) in zip(src_slots, pairs):
        heads[s] = head
    load(ctx, heads)
    other = Context(max_games=8, max_sims=1, max_plies=600)            # another max_plies: another record stride
    for s, d in zip(src_slots, same_slots):
        ctx.copy_game(d, s)
    for s, d in zip(src_slots, other_slots):
        other.copy_game_from(d, ctx, s)
    games = [lu.replay(head) for head, _ in pairs]
    records = [list(head) for head, _ in pairs]
    assert slot_differences(ctx, src_slots + same_slots, games + games, records + records) == []
    assert slot_differences(other, other_slots, games, records) == []
    # the copies play on, each in its own context; the sources stay where they were
    for c, slots in ((ctx, same_slots), (other, other_slots)):
        played = [lu.replay(head) for head, _ in pairs]
        rec = [list(head) for head, _ in pairs]
        for k in range(max(len(t) for _, t in pairs)):
            push = np.full(c.G, NO_MOVE, np.uint16)
            for s, g, r, (_, tail) in zip(slots, played, rec, pairs):
                if k < len(tail):
                    push[s] = tail[k]
                    assert lu.push(g, tail[k])
                    r.append(tail[k])
            ok = c.push_moves(push)
            assert np.array_equal(ok, (push != NO_MOVE).astype(np.uint8))
            assert slot_differences(c, slots, played, rec, planes=(k % 4 == 0)) == []
        assert played[0].get_result() == 0 and played[0].repetitions() == 5 and c.results()[slots[0]] == 0
    assert slot_differences(ctx, src_slots, games, records) == []
    other.close()


def test_get_copy_of_a_long_dropin_game():
    """Game.get_copy (crl_copy_game in the arena) of a game beyond ply 256: the copy meets the fifth occurrence after
    three more plies, the original stays a running game."""
    from chessrl_amd.game import Game
    (head, tail), _ = copy_pairs()
    o = lu.replay(head)
    g = Game()
    for m in head:
        assert g.move(move_to_uci(m))
    c = g.get_copy()
    assert len(c) == len(head) and c.get_history()["moves"] == o.get_history()["moves"] and c.get_result() is None
    for m in tail:
        assert c.get_result() is None and c.get_legal_moves() == o.get_legal_moves()
        assert c.move(move_to_uci(m)) and lu.push(o, m)
        assert np.array_equal(c.board_row(), oracle_row(o))
    assert c.get_result() == 0 == o.get_result() and len(c) == len(head) + 3
    assert len(g) == len(head) and g.get_result() is None and list(g.move_ids()) == list(head)
    again = c.get_copy()                                                  # a finished game copies as finished
    assert again.get_result() == 0 and len(again) == len(c)
    for x in (again, c, g):
        x.free()


# ---- 5. one-leaf search ------------------------------------------------------------------------------------------------
def terminal_hits(n):
    """Simulations that ended on an existing terminal node (the device's terminal_hits counter)."""
    return (max(0, n.visits - 1) if n.result is not None else 0) + sum(terminal_hits(k) for k in n.kids)


def fivefold_nodes(n):
    """(terminal nodes of the tree that are a fifth occurrence, simulations that ended on one of them again)."""
    mine = n.result is not None and n.state.repetitions() >= 5
    nodes, hits = int(mine), max(0, n.visits - 1) if mine else 0
    for k in n.kids:
        kn, kh = fivefold_nodes(k)
        nodes, hits = nodes + kn, hits + kh
    return nodes, hits


@functools.lru_cache(maxsize=None)
def search_roots():
    """The 16 late roots, then the straddling games cut at L + 13 (their first two once more: 28 slots)."""
    late = [lu.root_game(r) for r in lu.late_roots()]
    cut = [lu.replay(head) for head, _ in straddling_cut(13)]
    return tuple(late + cut + cut[:2])


@functools.lru_cache(maxsize=None)
def search_reference():
    """(stats, terminal hits, (fifth-occurrence nodes, hits on them)) of the oracle's tree of every root after SIMS
    simulations.  26 trees of 120 simulations cost the Python oracle several seconds (more than any device call of
    this file): computed once, shared by both graph modes and the negative control."""
    out, seen = [], {}
    for g in search_roots():
        key = tuple(lu.ids_of(g))
        if key not in seen:
            root = rr.new_root(g)
            rr.grow(root, mcts_oracle.OracleAgent(NET), SIMS, MODE)
            st = rr.root_stats(root)
            del st["n_nodes"]
            seen[key] = (st, terminal_hits(root), fivefold_nodes(root))
        out.append(seen[key])
    return tuple(out)


def tree_differences(graph, bare=False):
    """One search of SIMS simulations from every root (``bare``: from its position alone) against the oracle's search
    from the game WITH its history: ([slots whose root statistics differ], the context's counters)."""
    from chessrl_amd.engine import LockstepEngine
    games = search_roots()
    eng = LockstepEngine(NET.to("cuda:0"), n_games=len(games), max_sims=SIMS, numpy_promotion=MODE, use_graph=graph,
                         max_plies=1024)
    if bare:
        eng.reset()
        load_bare(eng.ctx, games)
    else:
        eng.load_moves([lu.ids_of(g) for g in games])
    eng.search(SIMS)
    rc = eng.root_children()
    cnt = eng.ctx.counters()
    eng.close()
    return [i for i, (st, _, _) in enumerate(search_reference()) if device_stats(rc, i) != st], cnt


@pytest.mark.parametrize("graph", [False, True])
def test_search_from_late_roots_matches_the_oracle(graph):
    """Visits, value sums as float64 bit patterns, priors, moves and replies of every root child.  In the straddling
    slots the tree's repetition scan runs over tree path + ring across index 0 and meets fifth occurrences: by the
    oracle, several of those trees hold a node that IS a fifth occurrence (not a fifty-move draw) and simulations come
    back to such a node, so the device's terminal hits, equal to the oracle's, include hits found through the ring."""
    ref = search_reference()
    fifth = [ff for _, _, ff in ref[16:26]]
    assert sum(nodes > 0 for nodes, _ in fifth) >= 4 and sum(hits for _, hits in fifth) > 0, fifth
    bad, cnt = tree_differences(graph)
    assert bad == []
    assert cnt["sims"] == len(ref) * SIMS
    assert cnt["terminal_hits"] == sum(hits for _, hits, _ in ref) > 0


THREE_ROOTS = (3, 4, 5)                           # the late roots at plies 253, 254 and 255


@functools.lru_cache(maxsize=None)
def three_move_reference(reuse):
    """The oracle's three moves and fourth search from every root of THREE_ROOTS, once per mode: per root a list of
    (stats of the search, chosen child, (bm, am), move ids of the game after the move, its result), and the number of
    subtrees kept (tests/reroot_util.py: the chosen child keeps its subtree where it fits)."""
    S, cap = STEP_SIMS, 3 * STEP_SIMS + 1
    agent = mcts_oracle.OracleAgent(NET)
    out, kept = [], 0
    for r in [lu.late_roots()[i] for i in THREE_ROOTS]:
        g = lu.root_game(r)
        tree, rows = rr.new_root(g), []
        for move in range(4):
            assert g.get_result() is None                                # (a condition on the inputs)
            rr.grow(tree, agent, S, MODE)
            st = rr.root_stats(tree)
            del st["n_nodes"]
            chosen = int(np.argmax(mcts_oracle.compute_policy(st["visits"], st["root_visits"], len(g), noise=False)))
            ch = tree.kids[chosen]
            if move < 3:
                assert g.move(ch.move) and (ch.reply == NULL_MOVE or g.move(ch.reply))
                if reuse and ch.result is None and rr.count(ch) + S <= cap:
                    tree = rr.reroot(tree, chosen)
                    kept += 1
                else:
                    tree = rr.new_root(g)
            rows.append((st, chosen, (ch.move, ch.reply), lu.ids_of(g), res_of(g)))
        out.append(rows)
    return out, kept


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("reuse", [False, True])
def test_three_moves_across_the_wrap_by_advance_and_by_reroot(reuse, graph):
    """Roots at plies 253, 254 and 255: search -> advance (or reroot, keeping the subtree) three times, so that the two
    plies of every move are written at ring indices 254 .. 5, then a fourth search: records and every search against
    the oracle game."""
    from chessrl_amd.engine import LockstepEngine, compute_policy
    roots = [lu.late_roots()[i] for i in THREE_ROOTS]
    assert [r.cut for r in roots] == [253, 254, 255]
    ref, kept = three_move_reference(reuse)
    assert (kept > 0) == reuse and all(len(rows[3][3]) > lu.RING + 2 for rows in ref)
    S = STEP_SIMS
    eng = LockstepEngine(NET.to("cuda:0"), n_games=4, max_sims=S, max_nodes=3 * S + 1 if reuse else None, numpy_promotion=MODE,
                         use_graph=graph, max_plies=1024)
    eng.load_moves([list(r.ids[:r.cut]) for r in roots] + [[]])
    for move in range(4):
        eng.search(S, keep_root=reuse and move > 0)
        rc = eng.root_children()
        _, plies, _ = eng.ctx.records(with_moves=False)
        chosen = np.full(4, -1, np.int32)
        for i, rows in enumerate(ref):
            st = rows[move][0]
            assert device_stats(rc, i) == st, (move, i)
            chosen[i] = int(np.argmax(compute_policy(st["visits"], st["root_visits"], plies[i], noise=False)))
            assert chosen[i] == rows[move][1]
        if move == 3:
            break
        bm, am = eng.reroot(chosen, S) if reuse else eng.advance(chosen)
        rec, plies, res = eng.ctx.records()
        pos = eng.ctx.get_positions()
        for i, rows in enumerate(ref):
            _, _, pair, ids, result = rows[move]
            assert (move_to_uci(bm[i]), NULL_MOVE if am[i] == NO_MOVE else move_to_uci(am[i])) == pair, (move, i)
            assert list(rec[i, :plies[i]]) == ids and res[i] == result, (move, i)
            assert np.array_equal(pos[i], oracle_row(lu.replay(ids))), (move, i)
    eng.close()


# ---- 6. waves ----------------------------------------------------------------------------------------------------------
def test_waves_of_six_threads_from_late_roots_match_the_restatement():
    from chessrl_amd.engine import LockstepEngine
    games = search_roots()
    eng = LockstepEngine(NET.to("cuda:0"), n_games=len(games), max_sims=WAVE_SIMS, numpy_promotion=MODE, threads=THREADS,
                         max_plies=1024)
    eng.load_moves([lu.ids_of(g) for g in games])
    eng.search(WAVE_SIMS)
    rc = eng.root_children()
    ws = eng.ctx.wave_stats()
    nodes = [eng.ctx.fetch_tree(i)[2]["n_nodes"] for i in range(len(games))]
    eng.close()
    seen = {}
    for i, g in enumerate(games):
        key = tuple(lu.ids_of(g))
        if key not in seen:
            seen[key] = wu.wave_search(g, mcts_oracle.OracleAgent(NET), WAVE_SIMS, THREADS, MODE)[1]
        st = seen[key]
        got = device_stats(rc, i)
        assert [k for k in got if got[k] != st[k]] == [], i
        assert (nodes[i], int(ws["waves"][i]), int(ws["leaves"][i])) == (st["n_nodes"], len(st["waves"]), WAVE_SIMS), i


# ---- 7. playouts ---------------------------------------------------------------------------------------------------------
PLAYOUT_REPS, PLAYOUT_MAX_MOVES = 32, 40


def playout_roots():
    """The eight late roots with a clock >= 8, then every straddling game cut at L + 12 and L + 13: the reversible
    history the kernel copies from the ring holds four occurrences of the root, on both sides of index 0."""
    roots = [lu.root_game(r) for r in lu.late_roots()[0::2]]
    assert all(lu.clock(g) >= 8 for g in roots)
    for (h12, _), (h13, _) in zip(straddling_cut(12), straddling_cut(13)):
        roots += [lu.replay(h12), lu.replay(h13)]
    return roots


def test_playouts_from_late_roots_equal_the_restatement_bit_for_bit():
    import torch
    from chessrl_amd import _lib
    roots = playout_roots()
    n, R = len(roots), PLAYOUT_REPS
    keys = np.array([(0xC0FFEE << 32) + 3 * i + 1 for i in range(n)], np.uint64)
    want_v, want_r, want_p, reasons = ru.private(roots, keys, R, PLAYOUT_MAX_MOVES)
    ended = collections.Counter(w for row in reasons[8:] for w in row)
    assert ended["fivefold"] >= 8 and ended["fifty"] >= 8, ended       # (the restatement alone) the history decides playouts
    dev = torch.device("cuda", 0)
    c = _lib.Context(32, 1, max_plies=1024)
    load(c, [lu.ids_of(g) for g in roots])
    before = (c.get_positions().copy(), [a.copy() for a in c.records()])
    dkeys = torch.from_numpy(keys.view(np.int64)).to(dev)
    value = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    results = torch.full((n, R), 9, dtype=torch.int8, device=dev)
    plies = torch.full((n, R), -3, dtype=torch.int16, device=dev)
    torch.cuda.synchronize(dev)
    c.set_window(0, n)
    c.rollout(_lib.ROLLOUT_GAMES, R, PLAYOUT_MAX_MOVES, dkeys.data_ptr(), value.data_ptr(), results.data_ptr(), plies.data_ptr())
    c.set_window(0, 32)
    c.sync()
    got_r, got_p = results.cpu().numpy(), plies.cpu().numpy().view(np.uint16)
    assert [i for i in range(n) if not np.array_equal(got_r[i], want_r[i]) or not np.array_equal(got_p[i], want_p[i])] == []
    assert np.array_equal(value.cpu().numpy().view(np.uint32), want_v.view(np.uint32))
    assert np.array_equal(c.get_positions(), before[0]) and all(np.array_equal(a, b) for a, b in zip(c.records(), before[1]))
    c.close()


# ---- 8. the built-in opponent ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", lu.OPPONENT_DEPTHS)
def test_opponent_moves_pushed_from_late_roots_equal_the_restatement(depth):
    """Two plies of crl_opponent_moves(push=1) on the late roots, on the straddling games cut at L + 14 and, in the
    last slot, on the game of long_game_util.opponent_fifth_ids cut at L + 14: there the opponent's own two moves
    are the last two of the shuffle, so its second push completes the fifth occurrence at ply 257 -- running after
    the first push, drawn after the second (the FORCED_FIFTH case of tests/test_gpu_opponent.py beyond ply 256).  The
    opponent's search hands the rules a repetition count of 1 (csrc/opponent.hpp); what reads the ring is the push."""
    from chessrl_amd import _lib
    L, fifth = lu.OPPONENT_L, list(lu.opponent_fifth_ids())
    pairs = late_cut() + straddling_cut(14) + [(fifth[:L + 14], fifth[L + 14:])]
    games = [lu.replay(head) for head, _ in pairs]
    n = len(games)
    last = n - 1
    c = _lib.Context(32, 1, max_plies=1024)
    load(c, [head for head, _ in pairs])
    row = np.zeros(32, np.int32)
    row[:n] = depth
    for ply in range(2):
        want = [ou.alphabeta(g, depth) for g in games]
        moves, scores, nodes, flags = c.opponent_moves(row, push=True)
        got = [(int(moves[i]), int(scores[i]), int(nodes[i]), int(flags[i])) for i in range(n)]
        assert [i for i in range(n) if got[i] != want[i]] == [], ply
        for g, w in zip(games, want):
            assert w[0] == NO_MOVE or lu.push(g, w[0])
        rec, plies, res = c.records()
        pos = c.get_positions()
        for i, g in enumerate(games):
            assert list(rec[i, :plies[i]]) == lu.ids_of(g) and res[i] == res_of(g), (ply, i)
            assert np.array_equal(pos[i], oracle_row(g)), (ply, i)
        assert (moves[n:] == NO_MOVE).all() and (plies[n:] == 0).all()
        # the opponent's own fifth occurrence, stated without the oracle
        assert (int(moves[last]), int(flags[last])) == (fifth[L + 14 + ply], 0)
        assert (int(c.results()[last]), int(plies[last])) == ((RESULT_NONE, L + 15), (0, L + 16))[ply]
    assert list(rec[last, :L + 16]) == fifth and games[last].repetitions() == 5
    moves, _, _, flags = c.opponent_moves(row)                              # the drawn game is skipped
    assert (int(moves[last]), int(flags[last])) == (NO_MOVE, ou.SKIPPED)
    c.close()


# ---- 9. the negative control ---------------------------------------------------------------------------------------------
def test_without_their_history_the_same_checks_report_differences(ctx):
    """The straddling games cut at L + 13 and the late roots, loaded as bare positions, through the comparisons of
    items 1, 2 and 5 against the oracle WITH history: the result at the final ply, the planes and the trees differ."""
    pairs = straddling_cut(13)
    n = len(pairs)
    bad, trace = rules_differences(ctx, pairs, bare=True)
    for i, (head, tail) in enumerate(pairs):
        assert (i, len(head) + len(tail), "result") in bad                  # the fifth occurrence is not seen
    assert (trace[3][:n] == RESULT_NONE).all()
    assert not [b for b in bad if b[2] in ("legal moves", "position", "push")]
    for heads in ([h for h, _ in late_cut()], [h for h, _ in pairs]):
        bad = plane_differences(ctx, [(h, []) for h in heads], bare=True)
        assert sorted(bad) == sorted((i, len(h), fmt) for i, h in enumerate(heads) for fmt in ("f16", "bits"))   # every root, both formats
    slots, _ = tree_differences(False, bare=True)
    assert len(slots) >= 1


# ---- 10. the ply-pool boundary ---------------------------------------------------------------------------------------------
M = lu.BOUNDARY_PLIES
SLOT = 7                                          # the slot under test: never the last one


def boundary_ids():
    ids = lu.boundary_game()
    assert len(ids) == M + 1
    return ids


def test_a_record_of_exactly_max_plies_fits_and_one_more_move_is_a_capacity_error():
    from chessrl_amd._lib import Context, HipLibraryError
    ids = boundary_ids()
    c = Context(32, 1, max_plies=M)
    heads = [ids[:(41 * i) % M] for i in range(32)]
    heads[SLOT] = ids[:M]
    load(c, heads)
    games = [lu.replay(h) for h in heads]
    rec, plies, res = c.records()
    assert rec.shape == (32, M) and plies[SLOT] == M and res[SLOT] == RESULT_NONE
    assert slot_differences(c, range(32), games, heads) == []
    push = np.full(32, NO_MOVE, np.uint16)
    push[SLOT] = ids[M]
    assert ids[M] in games[SLOT].legal_move_ids()
    with pytest.raises(HipLibraryError, match=CAPACITY):
        c.push_moves(push)
    c.close()


def small_context(plies, max_plies=M):
    """Context of 8 slots whose slot 3 holds the boundary game after ``plies`` plies; the others shorter games."""
    from chessrl_amd._lib import Context
    ids = boundary_ids()
    c = Context(8, 1, max_plies=max_plies)
    heads = [ids[:29 * i] for i in range(8)]
    heads[3] = ids[:plies]
    load(c, heads)
    return c, lu.replay(ids[:plies])


@pytest.mark.parametrize("plies", [M, M - 1])
def test_greedy_push_at_the_boundary(plies):
    import torch
    from chessrl_amd._lib import HipLibraryError
    c, g = small_context(plies)
    pol = np.random.default_rng(5).random((8, 1968), dtype=np.float32)
    dpol = torch.from_numpy(pol).to("cuda:0")
    torch.cuda.synchronize()
    mask = np.zeros(8, np.uint8)
    mask[3] = 1
    if plies == M:
        with pytest.raises(HipLibraryError, match=CAPACITY):
            c.greedy_moves(dpol.data_ptr(), mask=mask, push=True)
    else:
        labels = {u: i for i, u in enumerate(encoder_oracle.get_uci_labels())}
        legal = g.legal_move_ids()
        want = legal[int(np.argmax([pol[3, labels[move_to_uci(m)]] for m in legal]))]
        moves = c.greedy_moves(dpol.data_ptr(), mask=mask, push=True)
        assert moves[3] == want and (np.delete(moves, 3) == NO_MOVE).all() and lu.push(g, want)
        assert slot_differences(c, [3], [g], [lu.ids_of(g)]) == [] and len(g) == M
    c.close()


@pytest.mark.parametrize("plies", [M, M - 1])
def test_opponent_push_at_the_boundary(plies):
    from chessrl_amd._lib import HipLibraryError
    c, g = small_context(plies)
    row = np.zeros(8, np.int32)
    row[3] = 1
    if plies == M:
        with pytest.raises(HipLibraryError, match=CAPACITY):
            c.opponent_moves(row, push=True)
    else:
        want = ou.alphabeta(g, 1)
        moves, scores, nodes, flags = c.opponent_moves(row, push=True)
        assert (int(moves[3]), int(scores[3]), int(nodes[3]), int(flags[3])) == want and lu.push(g, want[0])
        assert slot_differences(c, [3], [g], [lu.ids_of(g)]) == [] and len(g) == M
    c.close()


@pytest.mark.parametrize("plies", [M - 1, M - 2])
@pytest.mark.parametrize("how", ["advance", "reroot"])
def test_a_two_ply_move_at_the_boundary(how, plies):
    """crl_advance / crl_reroot of a child that holds our move and the reply: from ply M - 1 the record would need
    M + 1 entries, from M - 2 it fills the last one."""
    from chessrl_amd._lib import HipLibraryError
    from chessrl_amd.engine import LockstepEngine, compute_policy
    ids = boundary_ids()
    S = 20
    g = lu.replay(ids[:plies])
    r = mcts_oracle.search(g, mcts_oracle.OracleAgent(NET), S, noise=False, mode=MODE)
    assert NULL_MOVE not in r.moves                                       # the chosen child is two plies long
    eng = LockstepEngine(NET.to("cuda:0"), n_games=4, max_sims=S, max_nodes=2 * S + 1 if how == "reroot" else None,
                         numpy_promotion=MODE, max_plies=M)
    eng.load_moves([ids[:50], ids[:plies], ids[:100], []])
    eng.search(S)
    rc = eng.root_children()
    n = int(rc["nchild"][1])
    assert list(rc["visits"][1, :n]) == r.visits
    chosen = np.full(4, -1, np.int32)
    chosen[1] = int(np.argmax(compute_policy(rc["visits"][1, :n], rc["root_visits"][1], plies, noise=False)))
    assert chosen[1] == r.chosen
    step = (lambda: eng.reroot(chosen, S)) if how == "reroot" else (lambda: eng.advance(chosen))
    if plies == M - 1:
        with pytest.raises(HipLibraryError, match=CAPACITY):
            step()
    else:
        bm, am = step()
        assert (move_to_uci(bm[1]), move_to_uci(am[1])) == r.moves and g.move(r.moves[0]) and g.move(r.moves[1])
        assert slot_differences(eng.ctx, [1], [g], [lu.ids_of(g)], planes=False) == [] and len(g) == M
    eng.close()


@pytest.mark.parametrize("room", [M - 1, M])
def test_copy_game_from_into_a_shorter_record(room):
    """include/chessrl_hip.h: "The record must fit ctx's max_plies (CRL_ERR_CAPACITY otherwise)"."""
    from chessrl_amd._lib import Context, HipLibraryError
    src, g = small_context(M)
    dst = Context(8, 1, max_plies=room)
    if room < M:
        with pytest.raises(HipLibraryError, match=CAPACITY):
            dst.copy_game_from(2, src, 3)
    else:
        dst.copy_game_from(2, src, 3)
        assert slot_differences(dst, [2], [g], [lu.ids_of(g)]) == []
        assert slot_differences(src, [3], [g], [lu.ids_of(g)]) == []
    dst.close()
    src.close()
