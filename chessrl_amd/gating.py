"""Gate: a trained weight set replaces the one it was trained from only if it beats it in the arena.

``gate(candidate, incumbent, games=N, sims=S)`` plays the noise-free ``Arena(candidate, incumbent)`` -- A is the
candidate -- and answers ``accepted``: the candidate's score is at least ``threshold``.  ``selfplay --rounds
--gate-games N`` asks it once per round (``selfplay.gated_round``).  The score is over paired openings; no Elo is
claimed.

SCORE.  ``gate_half_points = 2 * a_won + drawn + unfinished`` and ``gate_score = gate_half_points / (2 * played)``: a
game cut off at ``max_plies`` counts as a DRAW.  (The arena's ``score_a`` counts it for nobody, so that A's score and
B's do not sum to 1; a gate's rule has to be symmetric: ``gate_half_points`` of A against B and of B against A sum to
``2 * played``.)

VERDICT.  ``verdict(half_points, played, threshold)`` is ``half_points / (2 * played) >= threshold`` in float64.  The
default threshold 0.55 is the customary 55 %: a parameter, not a measurement.

EARLY STOP.  While games run, the final half points lie in ``bounds(results) = (low, high)``: a running game adds 0
to ``low`` and 2 to ``high``.  ``decided`` answers as soon as ``verdict(low) == verdict(high)``.  It is the SAME
expression as the final verdict, and it is monotone in the half points, which lie between the bounds whatever the
running games still do -- so stopping early can never change the verdict.  The games still running are reported as
unfinished and, in the score that is printed, count as draws.

Everything above ``gate`` is pure: it imports without a GPU and without the HIP library.
"""
import argparse
import sys
import time

DEFAULT_THRESHOLD = 0.55
DEFAULT_BOUNDARY = "device"


# ---- the pure parts ---------------------------------------------------------------------------------------------
def gate_half_points(tally):
    """Half points of A in an arena tally: a win 2, a draw 1, a game cut off at ``max_plies`` 1."""
    return 2 * int(tally["a_won"]) + int(tally["drawn"]) + int(tally["unfinished"])


def gate_score(tally):
    return gate_half_points(tally) / (2 * int(tally["played"]))


def verdict(half_points, played, threshold=DEFAULT_THRESHOLD):
    """Accepted?  One expression for the final verdict and for the early one."""
    return bool(float(half_points) / float(2 * played) >= float(threshold))


def results_for_a(a_white, results):
    """Per-game results for white (1 / 0 / -1 or None) -> for A (1 won, 0 drawn, -1 lost, None running)."""
    return [None if r is None else (int(r) if c else -int(r)) for c, r in zip(a_white, results)]


def bounds(results):
    """(low, high) half points of A over per-game results for A; a running game (None) may still be lost or won."""
    low = high = 0
    for r in results:
        if r is None:
            high += 2
        else:
            low += r + 1
            high += r + 1
    return low, high


def decided(results, threshold=DEFAULT_THRESHOLD):
    """True / False once the running games can no longer change the verdict, else None."""
    low, high = bounds(results)
    n = len(results)
    lo, hi = verdict(low, n, threshold), verdict(high, n, threshold)
    return lo if lo == hi else None


# ---- the gate ---------------------------------------------------------------------------------------------------
def _evaluator(what, device):
    """A ready evaluator as it is; a weight dict or a weights file as a ``ChessModel`` that lives for the gate."""
    if isinstance(what, (str, dict)):
        from .model import ChessModel
        kw = {} if device is None else {"device": str(device)}
        return ChessModel(weights=what, **kw)
    return what


def gate(candidate, incumbent, games, sims, threshold=DEFAULT_THRESHOLD, seed=0, opening_plies=6, max_plies=512,
         early_stop=True, boundary=DEFAULT_BOUNDARY, device=None, use_graph=True, openings=None):
    """Plays ``Arena(candidate, incumbent, games, sims, noise=False)`` and returns ``dict(accepted, score, threshold,
    half_points, low, high, stopped_at_ply, plies_played, played, a_won, b_won, drawn, unfinished, score_a, as_white,
    games, seconds, boundary, sims, seed, precision_candidate, precision_incumbent)``.  ``candidate`` / ``incumbent``:
    ready evaluators (what ``arena`` takes), weight dicts or weight files.  ``early_stop``: the play ends at the first
    ply after which ``decided`` answers while games still run -- ``stopped_at_ply`` is that ply, counted from 1 after
    the openings, None when the games were played out.  ``boundary``: the arena's move boundary; ``sims=0`` (the greedy
    arena) always takes the host path.  ``openings``: the arena's, one entry per pair, instead of random plies."""
    from .arena import Arena, check_arguments, check_boundary, game_colours
    check_arguments(games, sims, openings, opening_plies, max_plies)
    if sims == 0:
        boundary = "host"
    check_boundary(boundary, False, sims)
    if not 0.0 <= float(threshold) <= 1.0:
        raise ValueError("threshold must lie in [0, 1]")
    cand = _evaluator(candidate, device)
    inc = cand if incumbent is candidate else _evaluator(incumbent, device)
    colours = game_colours(games)
    stopped = [None]
    t0 = time.perf_counter()
    ar = Arena(cand, inc, games=games, sims=sims, seed=seed, opening_plies=opening_plies, openings=openings,
               max_plies=max_plies, noise=False, use_graph=use_graph, device=device, boundary=boundary)
    try:
        def until(results):
            mine = results_for_a(colours, results)
            if any(r is None for r in mine) and decided(mine, threshold) is not None:
                stopped[0] = ar.plies_played
                return True
            return False
        out = ar.play(until=until if early_stop else None)
        plies_played = ar.plies_played
    finally:
        ar.close()
    seconds = time.perf_counter() - t0
    low, high = bounds(results_for_a(colours, [g["result"] for g in out["games"]]))
    half = gate_half_points(out)
    out.update(accepted=verdict(half, out["played"], threshold), score=gate_score(out), threshold=float(threshold),
               half_points=half, low=low, high=high, stopped_at_ply=stopped[0], plies_played=plies_played,
               seconds=seconds, boundary=boundary, sims=int(sims), seed=seed,
               precision_candidate=getattr(cand, "precision", None),
               precision_incumbent=getattr(inc, "precision", None))
    del ar, cand, inc
    return out


# ---- command line -----------------------------------------------------------------------------------------------
def parser():
    p = argparse.ArgumentParser(prog="python -m chessrl_amd.gating",
                                description="Plays a candidate weight set against the incumbent and accepts it if its "
                                            "score reaches the threshold (exit status 0 accepted, 1 rejected).")
    p.add_argument("candidate", metavar="CANDIDATE", help="model directory (newest weights) or weights file")
    p.add_argument("incumbent", metavar="INCUMBENT", help="model directory (newest weights) or weights file")
    p.add_argument("--games", type=int, default=64, help="number of games (even: pairs with the colours exchanged)")
    p.add_argument("--sims", type=int, default=100, help="simulations per move (0: both sides play their greedy move)")
    p.add_argument("--threshold", type=float, default=DEFAULT_THRESHOLD,
                   help="accepted iff (wins + draws / 2) / games reaches this; a game cut off counts as a draw")
    p.add_argument("--seed", type=int, default=0, help="seed of the random openings")
    p.add_argument("--opening-plies", type=int, default=6, help="random plies in front of every pair")
    p.add_argument("--max-plies", type=int, default=512, help="plies searched per game after its opening")
    p.add_argument("--no-early-stop", action="store_true", help="play every game out although the verdict is decided")
    p.add_argument("--host-boundary", action="store_true",
                   help="choose the moves on the host (the arena's default path) instead of on the device")
    return p


def main(argv=None):
    from .arena import check_arguments, summary_lines, weights_path
    a = parser().parse_args(argv)
    check_arguments(a.games, a.sims, None, a.opening_plies, a.max_plies)
    from .model import ChessModel
    path_c, path_i = weights_path(a.candidate), weights_path(a.incumbent)
    cand, inc = ChessModel(weights=path_c), ChessModel(weights=path_i)
    out = gate(cand, inc, a.games, a.sims, threshold=a.threshold, seed=a.seed, opening_plies=a.opening_plies,
               max_plies=a.max_plies, early_stop=not a.no_early_stop,
               boundary="host" if a.host_boundary else DEFAULT_BOUNDARY)
    print("\n".join(summary_lines(out, path_c, path_i, a.sims, cand.precision, inc.precision)))
    if out["stopped_at_ply"] is not None:
        print("Stopped after ply %d: the games still running cannot change the verdict" % out["stopped_at_ply"])
    print("Gate: %s (score %.3f against threshold %.3f)" % ("ACCEPTED" if out["accepted"] else "REJECTED",
                                                            out["score"], out["threshold"]))
    return out


if __name__ == "__main__":
    sys.exit(0 if main()["accepted"] else 1)
