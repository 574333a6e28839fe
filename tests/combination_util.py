"""The yes cells of ``chessrl_amd.searchmode.COVERS``, held to the CPU oracle (tests/test_gpu_search_combinations.py;
what concerns the oracle alone is asserted without a GPU in tests/test_search_combinations_cpu.py).

TEST INFRASTRUCTURE.

  cells            every subset of COVERS[kind] that can be asked for, generated from the table
  LegalFakeNet     ``oracle.fakenet.FakeNet`` on the device with the surface the engine looks for: priors by label list
                   (``forward_legal_into``) and, optionally, plane bitboards as input
  roots            the 8 games every cell is played from
  oracle_run       the expected trees, decisions and moves of 3 moves x 8 slots, by the oracle alone; one run per
                   (kind, tree_reuse, rollouts), cached
  device_run       the same 3 moves on the device for one cell -> a log of the same shape
  assert_same      two such logs are equal, bit for bit, slot by slot and move by move
"""
import collections
import functools
import itertools

import numpy as np

from chessrl_amd.searchmode import COVERS
from oracle import mcts_oracle
from oracle.chess_oracle import NULL_MOVE, OracleGame, board_from_fen, move_to_uci
from oracle.fakenet import FakeNet
from oracle.make_golden import f32hex, f64hex
from tests import opponent_reply_util as oru
from tests import reroot_util as ru
from tests import rollout_util as rou
from tests import wave_util as wu

NO_MOVE, RESULT_NONE = 0xFFFF, 2
G, MOVES, SIMS = 8, 3, 40
ROLLOUTS = (4, 12, 4)                            # repetitions, plies, seed
# node budget of a tree with reuse: a chosen child is kept while its subtree holds at most 40 nodes.  After the first
# move (41 nodes) every slot keeps; the second re-rooting meets trees of up to 80 nodes, and the slots whose search
# went down one line fall back
MAX_NODES = 80
MODE = "nep50"
NET_SEED, NET_SHIFT = 11, 29
WAVE_THREADS = 6
REPLY_DEPTH = 1
N_PREFIX, SHUFFLE_SLOT, CLAIM_SLOT, CLOCK_SLOTS = 3, 3, 4, (5, 6, 7)
CLAIM_FEN = "8/8/8/4k3/8/8/4K3/7R w - - 94 80"
QUIET_CLOCKS = (90, 88, 90)
ENDINGS = ("8/8/3k4/8/8/3K4/8/7R w - - 0 1", "8/8/3k4/8/8/2BKN3/8/8 w - - 0 1")
PREFIX_SEED = 42


# ---- the cells ---------------------------------------------------------------------------------------------------
# what the device runner below knows how to ask an engine for: a capability COVERS gains later is in none of them,
# and its cells fail (``unheld``) until someone holds them to the oracle
HELD = ("tree_reuse", "stamps", "legal_priors", "raw_priors", "rollouts")
Cell = collections.namedtuple("Cell", "kind caps")


def askable(caps):
    """raw_priors is a way of reading legal priors: it cannot be asked for without them."""
    return "raw_priors" not in caps or "legal_priors" in caps


def cells(kind):
    """Every askable subset of COVERS[kind] as a Cell, in a fixed order (the bare mode first)."""
    names = sorted(COVERS[kind], key=lambda c: (HELD.index(c) if c in HELD else len(HELD), c))
    out = []
    for bits in itertools.product((False, True), repeat=len(names)):
        caps = frozenset(c for c, b in zip(names, bits) if b)
        if askable(caps):
            out.append(Cell(kind, caps))
    return out


def all_cells():
    return [c for kind in sorted(COVERS) for c in cells(kind)]


def cell_id(cell):
    names = [c for c in HELD if c in cell.caps] + sorted(cell.caps - set(HELD))
    return "%s-%s" % (cell.kind, "+".join(names) if names else "bare")


def unheld(cell):
    return sorted(cell.caps - set(HELD))


def priors_of(cell):
    return "raw" if "raw_priors" in cell.caps else "legal" if "legal_priors" in cell.caps else "full"


def oracle_key(cell):
    """The oracle run a cell is compared with: stamps, plane format and policy format do not change the tree."""
    return cell.kind, "tree_reuse" in cell.caps, "rollouts" in cell.caps


def bitplanes_of(cell):
    """The plane format a cell runs in: alternating by its index among all cells."""
    return bool(all_cells().index(cell) & 1)


# ---- the net -----------------------------------------------------------------------------------------------------
def fakenet():
    return FakeNet(seed=NET_SEED, prior_shift=NET_SHIFT)


class _DeviceArray(object):
    """A raw device address as something ``torch.as_tensor`` understands."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


class LegalFakeNet(object):
    """FakeNet on the device behind the evaluator surface of the HIP heads.

    ``forward_legal_into`` evaluates the full FakeNet policy and writes ``priors_out[row, j] = policy[row, label[row,
    j]]`` for ``j < count[row]``, reading the search kernels' own label (u16 [rows][256]) and count (i32 [rows]) lists
    at the addresses the engine hands over: what the CPU oracle computes by masking the full vector, so the oracle
    drives a search that reads priors by label list.  Torch operations on the current stream only, the views of the
    lists built once per address: a captured step replays it.  ``stats_out`` (CRL_POLICY_LEGAL_RAW) is not implemented
    and ``raw_priors_supported`` not advertised: the raw format normalises with ``__expf`` on the device.

    ``bitplanes``: also take the encoder's [rows,128] int64 plane bitboards (bit sq of plane c is the plane value at
    rank row 7 - sq // 8, file sq % 8).  ``swap``: read ``label[row, j ^ 1]`` instead -- the negative control."""

    accepts_legal_labels = True

    def __init__(self, net, bitplanes=False, swap=False):
        import torch
        self.net, self.swap = net, swap
        self.accepts_bitplanes = bool(bitplanes)
        self.device = net.device
        self._views = {}
        self.legal_calls = 0
        sq = torch.arange(64, device=self.device) ^ 56                 # the square shown at spatial index p
        self._shift = sq.view(1, 64, 1)
        self._col = torch.arange(256, device=self.device).view(1, 256)
        self._src = (self._col ^ 1) if swap else self._col

    def _planes(self, planes):
        import torch
        if planes.dtype != torch.int64:
            return planes
        bits = (planes.view(-1, 1, 128) >> self._shift) & 1            # [rows, p, c]
        return bits.view(-1, 8, 8, 128)

    def __call__(self, planes):
        return self.net(self._planes(planes))

    def view(self, ptr, shape, typestr):
        import torch
        key = (int(ptr), tuple(shape), typestr)
        v = self._views.get(key)
        if v is None:
            v = self._views[key] = torch.as_tensor(_DeviceArray(ptr, shape, typestr), device=self.device)
        return v

    def forward_legal_into(self, planes, labels_ptr, counts_ptr, priors_out, val_out, stats_out=None):
        import torch
        if stats_out is not None:
            raise NotImplementedError("LegalFakeNet writes probabilities, not logits and slice statistics")
        rows = planes.shape[0]
        labels = self.view(labels_ptr, (rows, 256), "<i2")             # (u16 labels < 1968: the same bits)
        counts = self.view(counts_ptr, (rows,), "<i4")
        pol, val = self(planes)
        idx = (labels.to(torch.int64) & 0xFFFF).clamp_(max=pol.shape[1] - 1)    # (entries past the count are stale)
        got = torch.gather(pol, 1, idx.gather(1, self._src.expand(rows, 256)))
        priors_out.copy_(torch.where(self._col < counts.view(rows, 1), got, priors_out))
        if val_out is not None:
            val_out.copy_(val)
        self.legal_calls += 1


# ---- the roots ---------------------------------------------------------------------------------------------------
def clock(g):
    return (int(g.board_at(0).state) >> 12) & 255


def quiet_on(g, want, seed):
    """A copy of ``g`` played on by seeded quiet piece moves (no pawn move, no capture) until its halfmove clock is
    ``want``; still running."""
    from tests.long_game_util import _quiet_piece_moves, push
    rng = np.random.default_rng(seed)
    g = g.get_copy()
    while clock(g) < want:
        quiet = _quiet_piece_moves(g)
        assert push(g, quiet[int(rng.integers(len(quiet)))])
        assert g.get_result() is None
    return g


@functools.lru_cache(maxsize=None)
def roots():
    """8 running games.  Slots 0-2: random prefixes of 0, 30 and 60 plies.  SHUFFLE_SLOT: the king shuffle behind the
    locked pawns of tests/rollout_util.py, entered one move later: three legal moves at the root, and the game's own
    history holds the root position and the one two plies before it four times each.  CLAIM_SLOT: a rook ending set
    up at halfmove clock 94 with no history -- the fifty-move claim is three, two, one ply below the roots of the three
    moves.  CLOCK_SLOTS: the long quiet game of tests/test_gpu_search.py with the highest clock, played on quietly
    to clock 90 (a middlegame: its playouts mostly reset the clock), and two pawnless endings played quietly from
    clock 0 to 88 and 90: every playout from their leaves meets the claim within its 12 plies and scans up to 99
    plies of the game's history on the way."""
    from tests.test_gpu_search import long_quiet_games, random_prefix_games
    games = list(random_prefix_games(N_PREFIX, 60, seed=PREFIX_SEED))
    shuffle = OracleGame(board=board_from_fen(rou.BLOCKED))
    for u in rou.KING_SHUFFLE + rou.KING_SHUFFLE[:2]:
        assert shuffle.move(u), u
    games += [shuffle, OracleGame(board=board_from_fen(CLAIM_FEN))]
    games.append(quiet_on(max(long_quiet_games(10), key=clock), QUIET_CLOCKS[0], seed=QUIET_CLOCKS[0]))
    games += [quiet_on(OracleGame(board=board_from_fen(f)), want, seed=want) for f, want in zip(ENDINGS, QUIET_CLOCKS[1:])]
    assert len(games) == G
    return tuple(games)


# ---- the oracle --------------------------------------------------------------------------------------------------
def stats_of(root):
    st = ru.root_stats(root)
    del st["n_nodes"]
    return st


def holds_terminal(node):
    return any(k.result is not None or holds_terminal(k) for k in node.kids)


def choose(stats, plies):
    pol = mcts_oracle.compute_policy(stats["visits"], stats["root_visits"], plies, noise=False)
    return int(np.argmax(pol))


def _agent(kind, rollouts, slot):
    from chessrl_amd.simulation import stream_keys
    if kind == "opponent":
        return oru.ReplyAgent(fakenet(), REPLY_DEPTH, log_greedy=False)
    if rollouts:
        reps, plies, seed = ROLLOUTS
        return rou.RolloutAgent(fakenet(), stream_keys(seed, G)[slot], reps, plies)
    return mcts_oracle.OracleAgent(fakenet())


@functools.lru_cache(maxsize=None)
def oracle_run(kind, tree_reuse=False, rollouts=False):
    """The expected log of 3 moves from ``roots()``: per move and slot the root children (``stats``), the child chosen
    (``chosen``), our move and the stored reply (``pairs``); per re-rooting and slot the kept node count, 0 = fell back
    (``kept``); the number of simulations (``sims``).  A slot whose game has ended holds None.  Beside it what the
    conditions of the CPU test read: ``kept_terminal`` (re-rooting, slot) pairs whose kept subtree holds a terminal
    node, and ``reasons`` [move][slot] = how the playouts of that search ended."""
    log = {"stats": [[None] * G for _ in range(MOVES)], "chosen": [[-1] * G for _ in range(MOVES)],
           "pairs": [[None] * G for _ in range(MOVES)], "kept": [[0] * G for _ in range(MOVES - 1)], "sims": 0,
           "kept_terminal": [], "reasons": [[[] for _ in range(G)] for _ in range(MOVES)]}
    for slot, start in enumerate(roots()):
        agent = _agent(kind, rollouts, slot)
        game = start.get_copy()
        root = ru.new_root(game)
        for mv in range(MOVES):
            seen = len(getattr(agent, "reasons", ()))
            if kind == "wave":
                wu.grow_waves(root, agent, SIMS, WAVE_THREADS, MODE)
            else:
                ru.grow(root, agent, SIMS, MODE)
            log["sims"] += SIMS
            st = log["stats"][mv][slot] = stats_of(root)
            k = log["chosen"][mv][slot] = choose(st, len(game))
            ch = root.kids[k]
            log["pairs"][mv][slot] = (ch.move, None if ch.reply == NULL_MOVE else ch.reply)
            log["reasons"][mv][slot] = list(getattr(agent, "reasons", ())[seen:])
            assert game.move(ch.move)
            if ch.reply != NULL_MOVE:
                assert game.move(ch.reply)
            if ch.result is not None or mv + 1 == MOVES:
                break
            if tree_reuse and ru.count(ch) + SIMS <= MAX_NODES:          # the device's keep-or-fresh rule
                log["kept"][mv][slot] = ru.count(ch)
                if holds_terminal(ch):
                    log["kept_terminal"].append((mv, slot))
                root = ru.reroot(root, k)
            else:
                root = ru.new_root(game)
    return log


# ---- the device --------------------------------------------------------------------------------------------------
def hexes(a, kind):
    a = np.ascontiguousarray(a)
    return [(f64hex if kind == "f64" else f32hex)(x) for x in a]


def device_stats(rc, i):
    n = int(rc["nchild"][i])
    return {"visits": [int(v) for v in rc["visits"][i, :n]], "values": hexes(rc["values"][i, :n], "f64"),
            "priors": hexes(rc["priors"][i, :n], "f32"), "moves": [move_to_uci(m) for m in rc["moves"][i, :n]],
            "replies": [None if m == NO_MOVE else move_to_uci(m) for m in rc["replies"][i, :n]],
            "root_visits": int(rc["root_visits"][i])}


def mode_args(kind):
    """What makes a ``SearchMode`` / ``LockstepEngine`` of that kind."""
    from chessrl_amd.opponent import MinimaxPlayer
    from tests.opponent_util import NODE_LIMIT
    return {"leaf": {}, "wave": {"threads": WAVE_THREADS},
            "opponent": {"reply": MinimaxPlayer(False, search_depth=REPLY_DEPTH, node_limit=NODE_LIMIT)}}[kind]


def engine_for(cell, net, use_graph=True, bitplanes=False, legal=None, raw=None):
    """The engine of a cell over ``net`` with the roots loaded; ``legal`` / ``raw`` override the cell's policy format."""
    import torch
    from chessrl_amd.engine import LockstepEngine, StampRing
    from chessrl_amd.simulation import Rollouts
    assert not unheld(cell), "no test holds %s to the oracle yet (tests/combination_util.py)" % unheld(cell)
    pri = priors_of(cell)
    kw = {"legal_priors": pri != "full" if legal is None else legal, "raw_priors": pri == "raw" if raw is None else raw}
    if cell.kind == "wave":                      # (reads full policy vectors: the engine has no such switch to set)
        kw = {}
    kw.update(mode_args(cell.kind))
    if "rollouts" in cell.caps:
        kw["simulate"] = Rollouts(*ROLLOUTS)
    if "tree_reuse" in cell.caps:
        kw["max_nodes"] = MAX_NODES
    eng = LockstepEngine(net, n_games=G, max_sims=SIMS, numpy_promotion=MODE, use_graph=use_graph, bitplanes=bitplanes, **kw)
    assert eng.bitplanes == bitplanes and eng.use_graph == use_graph
    assert eng.STEPS_PER_GRAPH == LockstepEngine.STEPS_PER_GRAPH                   # the default
    if cell.kind != "wave":
        assert eng.legal_priors == kw["legal_priors"] and eng.raw_priors == bool(kw["raw_priors"])
    if "stamps" in cell.caps:
        eng.set_stamps(StampRing(16 * MOVES * SIMS, torch.device("cuda", 0)))
    oru.load_games(eng.ctx, list(roots()))
    return eng


def expected_stamps(eng, searches):
    """The stamp ids the engine's own phases write over ``searches`` searches of SIMS steps: the plan once per step,
    the end-of-graph stamp behind every replayed graph."""
    from chessrl_amd.engine import STAMP_GRAPH_END
    plan = [sid for sid, _ in eng.mode.plan]
    if not eng.use_graph:
        return plan * (SIMS * searches)
    K, n, one = eng.STEPS_PER_GRAPH, SIMS, []
    while K > 1 and n >= K:
        one += plan * K + [STAMP_GRAPH_END]
        n -= K
    one += (plan + [STAMP_GRAPH_END]) * n
    return one * searches


def device_run(cell, net, use_graph=True, **kw):
    """3 moves of the cell on the device -> a log shaped like ``oracle_run``'s (``stats``, ``chosen``, ``pairs``,
    ``kept``, ``sims``), plus ``stamps`` (the engine's own stamp ids as read from the ring, or None)."""
    from chessrl_amd.engine import STAMP_TRUNK, compute_policy
    eng = engine_for(cell, net, use_graph=use_graph, **kw)
    reuse = "tree_reuse" in cell.caps
    log = {"stats": [[None] * G for _ in range(MOVES)], "chosen": [[-1] * G for _ in range(MOVES)],
           "pairs": [[None] * G for _ in range(MOVES)], "kept": [[0] * G for _ in range(MOVES - 1)], "stamps": None}
    for mv in range(MOVES):
        eng.search(SIMS, keep_root=reuse and mv > 0)
        rc = eng.root_children()
        _, plies, results = eng.ctx.records(with_moves=False)
        chosen = np.full(G, -1, dtype=np.int32)
        for i in range(G):
            assert (rc["nchild"][i] > 0) == (results[i] == RESULT_NONE), (mv, i)   # only a finished game has no tree
            if rc["nchild"][i]:
                st = log["stats"][mv][i] = device_stats(rc, i)
                chosen[i] = log["chosen"][mv][i] = int(np.argmax(
                    compute_policy(st["visits"], st["root_visits"], plies[i], noise=False)))
        if reuse and mv + 1 < MOVES:
            bm, am = eng.reroot(chosen, SIMS)
            for i in range(G):
                info = eng.ctx.fetch_tree(i)[2]
                assert info["kept"] == (info["n_nodes"] > 0)
                log["kept"][mv][i] = info["n_nodes"]
        else:
            bm, am = eng.advance(chosen)
        for i in range(G):
            if chosen[i] >= 0:
                log["pairs"][mv][i] = (move_to_uci(bm[i]), None if am[i] == NO_MOVE else move_to_uci(am[i]))
    log["sims"] = eng.ctx.counters()["sims"]
    if eng.stamps is not None:
        trunk = {sid for pair in STAMP_TRUNK.values() for sid in pair}             # (a real tower stamps its trunk launches)
        log["stamps"] = [sid for sid, _ in eng.stamps.read() if sid not in trunk]
        assert log["stamps"] == expected_stamps(eng, MOVES)
        eng.set_stamps(None)                     # (a shared evaluator must not go on stamping into this ring)
    eng.close()
    return log


COMPARED = ("stats", "chosen", "pairs", "kept", "sims")


def assert_same(got, want, what):
    """Every slot of every move, then the decisions of every re-rooting and the simulation count."""
    for mv in range(MOVES):
        for i in range(G):
            a, b = got["stats"][mv][i], want["stats"][mv][i]
            assert (a is None) == (b is None), (what, mv, i)
            if a is not None:
                for k in b:
                    assert a[k] == b[k], (what, "move %d slot %d" % (mv, i), k)
    for k in COMPARED[1:]:
        assert got[k] == want[k], (what, k)


def differing_slots(a, b):
    return [i for i in range(G) if any(a["stats"][mv][i] != b["stats"][mv][i] for mv in range(MOVES))]
