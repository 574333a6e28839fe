"""Arena: two weight sets play each other in lockstep, and the score says which is better.

``selfplay --rounds`` trains and swaps weights in; ``benchmark`` measures a net against the built-in opponent, where
two nets that both lose look the same.  ``arena(model_a, model_b, games=N, sims=S)`` plays A against B directly.

GAMES AND COLOURS.  Games ``2i`` and ``2i + 1`` are a PAIR: they share an opening, A is white in ``2i`` and black in
``2i + 1``.  A search here is deterministic, so without openings every game of one colour assignment would be the
same game; with them, a pair is the same opening seen from both sides.

OPENINGS.  ``openings=None``: every pair plays ``opening_plies`` random plies, drawn as ``gen_data`` draws them
(``gen_data.opening_words`` from ``random.Random(seed)``, played by ``Context.rollout_games``), once per pair, read
back with ``records()`` and loaded into every engine that holds the pair.  A pair whose opening already has a result
is kept and counts with that result.  ``openings=[...]``: one entry per pair, a list of UCI moves from the standard
position or a FEN string.

ENGINES (``sims`` > 0).  W = the games in which A is white, K = the others.  Four plain leaf-mode ``LockstepEngine``s,
each with ONE evaluator for life -- (A, W), (B, W), (B, K), (A, K) -- so that no evaluator is ever swapped under a
captured hipGraph.  The two engines of a set are MIRRORS: the same games in the same slots.  Per ply and set, the
engine of the side to move runs ``search(sims)``, ``root_children()``, ``choose_children(noise=...)`` and
``advance(chosen, plies=1)`` -- the one-ply boundary, ``crl_advance_one`` -- and its ``bm`` is pushed into the mirror
with ``ctx.push_moves`` (a ``NO_MOVE`` slot is left alone).  A set whose games are not all on the same side to move
(FEN openings may differ) does this once for either engine, each for its own slots.  A game is searched while it runs
and has played fewer than ``max_plies`` plies after its opening.  No refill, no compaction, no tree reuse, no stamps.

GREEDY ARENA (``sims=0``): the reference's ``best_move(real_game=True)`` on both sides -- one context per set, the
tower of the side to move, ``greedy_moves(policy, mask, push=True)`` as ``benchmark`` does on the agent's plies.

DEVICE BOUNDARY (``boundary="device"``, ``sims`` > 0, no noise).  Per ply and set the mover runs ``search(sims)`` and
``advance_argmax`` -- ``k_choose_advance_one``: the first maximum of the root children's visits in children order,
which is what ``choose_children(noise=False)`` chooses at every ply count, and the one-ply advance, in one kernel --
and the mirror takes ``bm`` from device memory (``push_moves_dev``).  The only host round trip of a ply is the
``records(with_moves=False)`` that the termination test reads.  ``boundary="host"`` (default) is the path above.

EARLY END.  ``Arena.play(until=f)`` calls ``f(results by game number)`` after every ply of both sets; a true return
ends the play, and the games still running are reported as unfinished (``gating`` stops a decided gate so).

NOISE.  Off by default.  ``noise=True``: game ``i`` draws its Dirichlet rows from ``np.random.default_rng([seed, i])``,
one row per searched ply, whichever side searches.

The result is a score over paired openings, not an Elo.
"""
import argparse
import json
import os
import random

import numpy as np

from . import _lib
from .game import board_row_from_fen, move_to_uci, uci_to_move

START_FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"


def check_arguments(games, sims, openings, opening_plies, max_plies):
    """Every refusal of ``arena``, before any device is touched."""
    if int(games) != games or games <= 0 or games % 2:
        raise ValueError("games must be positive and even: games 2i and 2i + 1 are a pair")
    if int(sims) != sims or sims < 0:
        raise ValueError("sims must be 0 (the greedy arena) or the number of simulations per move")
    if openings is not None and len(openings) != games // 2:
        raise ValueError("openings: one entry per pair (%d), got %d" % (games // 2, len(openings)))
    if opening_plies < 0:
        raise ValueError("opening_plies must not be negative")
    if max_plies < 1:
        raise ValueError("max_plies must be at least 1")


BOUNDARIES = ("host", "device")


def check_boundary(boundary, noise, sims, model_a=None, model_b=None):
    """The refusals of ``Arena(..., boundary=...)``, before any device is touched.  The device boundary plays the first
    maximum of the visits, which is the noise-free choice only; it belongs to the searching arena; and the two engines
    of a set hand their moves over in device memory in stream order, so both must sit on one device's stream."""
    if boundary not in BOUNDARIES:
        raise ValueError("boundary must be one of %s" % (BOUNDARIES,))
    if boundary == "host":
        return
    if noise:
        raise ValueError('boundary="device" chooses the most visited child: not with noise=True')
    if sims == 0:
        raise ValueError('boundary="device" is the boundary of a search: not with sims=0 (the greedy arena)')
    dev_a, dev_b = getattr(model_a, "device", None), getattr(model_b, "device", None)
    if dev_a is not None and dev_b is not None and str(dev_a) != str(dev_b):
        raise ValueError('boundary="device": the two engines of a set must be on one stream, the evaluators are on '
                         "%s and %s" % (dev_a, dev_b))


def game_colours(games):
    """A is white in the even games and black in the odd ones."""
    return [i % 2 == 0 for i in range(games)]


def tally(a_white, results):
    """Counts of per-game (A is white, result for white or None).  A game without a result is played, unfinished and
    scored as nothing (``benchmark``'s rule); ``as_white``: the same counts over A's white games only."""
    def count(rows):
        a = sum(1 for c, r in rows if r is not None and r != 0 and (r == 1) == bool(c))
        b = sum(1 for c, r in rows if r is not None and r != 0 and (r == 1) != bool(c))
        d = sum(1 for _, r in rows if r == 0)
        n = len(rows)
        return dict(played=n, a_won=a, b_won=b, drawn=d, unfinished=n - a - b - d,
                    score_a=(a + d / 2) / n if n else 0.0)
    rows = list(zip(a_white, results))
    out = count(rows)
    out["as_white"] = count([x for x in rows if x[0]])
    return out


def parse_opening(entry):
    """One ``openings`` entry -> (fen or None, [move ids]): a FEN string, or a list of UCI moves."""
    if isinstance(entry, str):
        if "/" not in entry:
            raise ValueError("an opening is a FEN string or a list of UCI moves: %r" % (entry,))
        return entry, []
    ids = [uci_to_move(u) for u in entry]
    if any(m is None for m in ids):
        raise ValueError("not a UCI move in opening %r" % (list(entry),))
    return None, ids


def random_openings(pairs, opening_plies, seed, device=0):
    """``pairs`` move-id lists of ``opening_plies`` random plies each (shorter where the game ended), as ``gen_data``
    draws them."""
    if opening_plies == 0:
        return [[] for _ in range(pairs)]
    from .gen_data import opening_words
    rng = random.Random(seed)
    ctx = _lib.Context(pairs, 1, max_plies=max(opening_plies, 2), device=device)
    try:
        played = np.zeros(pairs, np.int32)
        while True:
            words = opening_words(rng, pairs, opening_plies)
            played, _, res = ctx.rollout_games(words, np.full(pairs, words.shape[1], np.int32), 1, opening_plies,
                                               played=played)
            if ((played >= opening_plies) | (res[:, 0] != _lib.RESULT_NONE)).all():
                break
        moves, plies, _ = ctx.records()
        return [[int(m) for m in moves[i, :plies[i]]] for i in range(pairs)]
    finally:
        ctx.close()


def _load(ctx, specs):
    """Slot i of ``ctx`` becomes opening ``specs[i]`` = (fen or None, move ids)."""
    rows = np.stack([board_row_from_fen(fen or START_FEN) for fen, _ in specs])
    ctx.set_positions(rows)
    n = max(len(ids) for _, ids in specs)
    if n == 0:
        return
    table = np.full((len(specs), n), _lib.NO_MOVE, dtype=np.uint16)
    counts = np.zeros(len(specs), dtype=np.int32)
    for g, (_, ids) in enumerate(specs):
        table[g, :len(ids)] = ids
        counts[g] = len(ids)
    pushed = ctx.push_sequences(table, counts)
    for g, (_, ids) in enumerate(specs):
        if pushed[g] != len(ids):
            raise ValueError("illegal move %s in opening %d" % (move_to_uci(ids[int(pushed[g])]), g))


class _Set(object):
    """The games of one colour assignment: their mirrors (or with ``sims=0`` their one context), game numbers,
    per-game generators."""

    def __init__(self, a_white, numbers):
        self.a_white, self.numbers = a_white, numbers
        self.engines = {}                    # "a" / "b" -> LockstepEngine (sims > 0)
        self.ctx = None                      # sims = 0
        self.planes = None
        self.rngs = None
        self.ply_limit = None                # boundary="device": int32 per slot on the device

    def main_ctx(self):
        return self.ctx if self.ctx is not None else self.engines["a"].ctx


class Arena(object):
    """``arena`` as an object, so that a caller can look at the engines after the last ply (``sets``: the set of A's
    white games, then of its black games; ``sets[k].engines["a"] / ["b"]`` are mirrors).  ``play()`` returns what
    ``arena`` returns; ``close()`` frees the device state."""

    def __init__(self, model_a, model_b, games=2, sims=0, seed=0, opening_plies=6, openings=None, max_plies=512,
                 noise=False, use_graph=True, device=None, boundary="host"):
        check_arguments(games, sims, openings, opening_plies, max_plies)
        check_boundary(boundary, noise, sims, model_a, model_b)
        import torch
        self.models = {"a": model_a, "b": model_b}
        self.games, self.sims, self.seed, self.noise = int(games), int(sims), seed, bool(noise)
        self.max_plies, self.use_graph, self.boundary = int(max_plies), use_graph, boundary
        self.plies_played = 0                    # plies of the play so far (both sets have played that many)
        pairs = self.games // 2
        specs = None if openings is None else [parse_opening(o) for o in openings]
        if device is None:
            device = getattr(model_a, "device", None) or torch.device("cuda", 0)
        self.dev = torch.device(device)
        if self.dev.type != "cuda" or not torch.cuda.is_available():
            raise _lib.HipLibraryError("the arena needs an MI355X: no CPU fallback exists")
        index = self.dev.index or 0
        if specs is None:
            specs = [(None, ids) for ids in random_openings(pairs, int(opening_plies), seed, device=index)]
        self.specs = specs
        pool = max(len(ids) for _, ids in specs) + self.max_plies
        self.sets = []
        try:
            for a_white in (True, False):
                s = _Set(a_white, [2 * i + (0 if a_white else 1) for i in range(pairs)])
                self.sets.append(s)
                if self.noise:
                    s.rngs = [np.random.default_rng([seed, i]) for i in s.numbers]
                if self.sims > 0:
                    from .engine import LockstepEngine
                    for who in ("a", "b"):
                        s.engines[who] = LockstepEngine(self.models[who], pairs, self.sims, device=index,
                                                        max_plies=max(pool, 2), use_graph=use_graph)
                        _load(s.engines[who].ctx, specs)
                    if boundary == "device":     # a game is searched while it has played fewer plies than this
                        limit = np.array([len(ids) + self.max_plies for _, ids in specs], dtype=np.int32)
                        s.ply_limit = torch.from_numpy(limit).to(self.dev)
                else:
                    s.ctx = _lib.Context(pairs, 1, max_plies=max(pool, 2), device=index)
                    s.ctx.set_stream(torch.cuda.current_stream(self.dev).cuda_stream)
                    s.planes = torch.zeros((pairs, 8, 8, _lib.PLANES), dtype=torch.float16, device=self.dev)
                    _load(s.ctx, specs)
        except Exception:
            self.close()
            raise

    def close(self):
        for s in self.sets:
            for eng in s.engines.values():
                eng.close()
            s.engines = {}
            if s.ctx is not None:
                s.ctx.close()
                s.ctx = None

    # ---- one ply of one set ----------------------------------------------------------------------------------
    def _movers(self, s, live, white_to_move):
        """who -> mask of the slots of set ``s`` in which that side is to move and the game is searched"""
        a_moves = white_to_move == s.a_white
        return {"a": live & a_moves, "b": live & ~a_moves}

    def _search_ply(self, s, movers, plies):
        from .engine import choose_children
        for who, other in (("a", "b"), ("b", "a")):
            mask = movers[who]
            if not mask.any():
                continue
            eng = s.engines[who]
            eng.search(self.sims)
            rc = eng.root_children()
            nchild = np.where(mask, rc["nchild"], 0)         # the other slots choose nothing and draw no noise
            chosen = choose_children(rc["visits"], nchild, rc["root_visits"], plies, noise=self.noise, rngs=s.rngs)
            bm = eng.advance(chosen, plies=1)
            s.engines[other].ctx.push_moves(bm)              # the mirror follows; NO_MOVE slots are left alone

    def _search_ply_device(self, s, movers):
        """``_search_ply`` without the host between search and move: the choice and the advance are one kernel
        (``LockstepEngine.advance_argmax``) and the mirror takes the moves from device memory, in stream order."""
        for who, other in (("a", "b"), ("b", "a")):
            if not movers[who].any():
                continue
            eng = s.engines[who]
            eng.search(self.sims)
            bm, _ = eng.advance_argmax(s.a_white == (who == "a"), s.ply_limit)
            mirror = s.engines[other]
            mirror._bind_stream()
            mirror.ctx.push_moves_dev(bm)

    def _greedy_ply(self, s, movers):
        s.ctx.encode(s.planes.data_ptr())
        for who in ("a", "b"):
            mask = movers[who]
            if mask.any():
                policy = self.models[who](s.planes)[0].float().contiguous()
                s.ctx.greedy_moves(policy.data_ptr(), mask=mask, push=True, want_moves=False)

    def play(self, until=None):
        """Plays the games out and returns the report.  ``until``: called after every ply of both sets with the
        results by game number (1 / 0 / -1 for white, None for a running game); a true return ends the play, and the
        games still running are reported as unfinished.  ``plies_played`` counts the plies."""
        state = []
        for s in self.sets:
            ctx = s.main_ctx()
            _, plies, results = ctx.records(with_moves=False)
            white = (ctx.get_positions()[:, 7] & np.uint64(1)).astype(bool)
            state.append([plies, results, white])
        for _ in range(self.max_plies):
            if not any((st[1] == _lib.RESULT_NONE).any() for st in state):
                break
            for s, st in zip(self.sets, state):                          # both sets in the same ply, one after the other
                plies, results, white = st
                live = results == _lib.RESULT_NONE
                if not live.any():
                    continue
                movers = self._movers(s, live, white)
                if self.sims > 0 and self.boundary == "device":
                    self._search_ply_device(s, movers)
                elif self.sims > 0:
                    self._search_ply(s, movers, plies)
                else:
                    self._greedy_ply(s, movers)
                _, st[0], st[1] = s.main_ctx().records(with_moves=False)
                st[2] = np.where(live, ~white, white)
            self.plies_played += 1
            if until is not None and until(self._results_by_number(state)):
                break
        if self.boundary == "device":            # the mirrors' own device errors (a refused move) surface here
            for s in self.sets:
                s.engines["b"].ctx.sync()
        return self._report()

    def _results_by_number(self, state):
        out = [None] * self.games
        for s, st in zip(self.sets, state):
            for slot, number in enumerate(s.numbers):
                r = int(st[1][slot])
                out[number] = None if r == _lib.RESULT_NONE else r
        return out

    def _report(self):
        games = [None] * self.games
        for s in self.sets:
            moves, plies, results = s.main_ctx().records()
            for slot, number in enumerate(s.numbers):
                fen, ids = self.specs[slot]
                r = int(results[slot])
                games[number] = dict(a_white=s.a_white,
                                     opening=fen if fen is not None else [move_to_uci(m) for m in ids],
                                     moves=[move_to_uci(m) for m in moves[slot, len(ids):plies[slot]]],
                                     result=None if r == _lib.RESULT_NONE else r)
        out = tally([g["a_white"] for g in games], [g["result"] for g in games])
        out["games"] = games
        return out


def arena(model_a, model_b, games=2, sims=0, seed=0, opening_plies=6, openings=None, max_plies=512, noise=False,
          use_graph=True, device=None, boundary="host"):
    """Plays ``games`` games (even: pairs on a shared opening, colours exchanged) between the ready evaluators
    ``model_a`` and ``model_b`` with ``sims`` simulations per move (0: both sides greedy) and returns
    ``dict(played, a_won, b_won, drawn, unfinished, score_a, as_white, games)``: ``score_a = (a_won + drawn / 2) /
    played``, ``as_white`` the same counts over A's white games, ``games`` a list of ``dict(a_white, opening, moves,
    result)`` -- the opening as UCI moves or its FEN, the moves played after it as UCI strings, the result 1 / 0 / -1
    for white or None.  A game still running after ``max_plies`` plies past its opening is played, unfinished and
    scored as nothing.  ``boundary="device"``: the noise-free move boundary without the host.  Module docstring: pairs,
    openings, engines, noise, boundary."""
    check_arguments(games, sims, openings, opening_plies, max_plies)
    check_boundary(boundary, noise, sims, model_a, model_b)
    ar = Arena(model_a, model_b, games=games, sims=sims, seed=seed, opening_plies=opening_plies, openings=openings,
               max_plies=max_plies, noise=noise, use_graph=use_graph, device=device, boundary=boundary)
    try:
        return ar.play()
    finally:
        ar.close()


# ---- command line -----------------------------------------------------------------------------------------------
def weights_path(where):
    """A model directory (its newest weights, ``selfplay.get_model_path``) or a weights file."""
    if os.path.isdir(where):
        from .selfplay import get_model_path
        return get_model_path(where)
    return where


def read_openings(path):
    """An openings file: a JSON list (entries: FEN strings or lists of UCI moves), or one opening per line -- a FEN,
    or UCI moves separated by blanks."""
    with open(path) as f:
        text = f.read()
    if text.lstrip().startswith("["):
        return json.loads(text)
    out = []
    for line in text.splitlines():
        line = line.strip()
        if line and not line.startswith("#"):
            out.append(line if "/" in line else line.split())
    return out


def parser():
    p = argparse.ArgumentParser(prog="python -m chessrl_amd.arena",
                                description="Plays two weight sets against each other on paired openings and prints "
                                            "the score.")
    p.add_argument("a", metavar="A", help="model directory (newest weights) or weights file of side A")
    p.add_argument("b", metavar="B", help="model directory (newest weights) or weights file of side B")
    p.add_argument("--games", type=int, default=16, help="number of games (even: pairs with the colours exchanged)")
    p.add_argument("--sims", type=int, default=0, help="simulations per move (0: both sides play their greedy move)")
    p.add_argument("--seed", type=int, default=0, help="seed of the random openings and of the noise")
    p.add_argument("--opening-plies", type=int, default=6, help="random plies in front of every pair")
    p.add_argument("--openings", metavar="FILE", default=None,
                   help="openings file, one per pair: a JSON list, or lines of a FEN or of UCI moves")
    p.add_argument("--max-plies", type=int, default=512, help="plies searched per game after its opening")
    p.add_argument("--noise", action="store_true", help="Dirichlet noise on the move choice (per-game streams)")
    return p


def summary_lines(out, path_a, path_b, sims, precision_a=None, precision_b=None):
    def named(path, precision):
        return "%s%s" % (path, " (%s)" % precision if precision else "")
    w = out["as_white"]
    return ["##################### SUMMARY ###################",
            "A: %s" % named(path_a, precision_a),
            "B: %s" % named(path_b, precision_b),
            "both sides: %s" % ("MCTS, %d simulations per move" % sims if sims > 0 else "greedy move"),
            "Games played: %d" % out["played"],
            "Games won by A: %d" % out["a_won"],
            "Games won by B: %d" % out["b_won"],
            "Games drawn: %d" % out["drawn"],
            "Games unfinished: %d" % out["unfinished"],
            "A as white: %d won, %d lost, %d drawn of %d" % (w["a_won"], w["b_won"], w["drawn"], w["played"]),
            "Score of A: %.3f (paired openings, no Elo claim)" % out["score_a"]]


def main(argv=None):
    a = parser().parse_args(argv)
    openings = None if a.openings is None else read_openings(a.openings)
    check_arguments(a.games, a.sims, openings, a.opening_plies, a.max_plies)
    from .model import ChessModel
    path_a, path_b = weights_path(a.a), weights_path(a.b)
    model_a, model_b = ChessModel(weights=path_a), ChessModel(weights=path_b)
    out = arena(model_a, model_b, games=a.games, sims=a.sims, seed=a.seed, opening_plies=a.opening_plies,
                openings=openings, max_plies=a.max_plies, noise=a.noise)
    print("\n".join(summary_lines(out, path_a, path_b, a.sims, model_a.precision, model_b.precision)))
    return out


if __name__ == "__main__":
    main()
