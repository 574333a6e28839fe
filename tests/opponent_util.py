"""CPU restatement of the built-in opponent (chessrl_amd/csrc/opponent.hpp) over ``oracle.chess_oracle.OracleGame``.

TEST INFRASTRUCTURE, written from the header comment of opponent.hpp alone.  Pure Python integers:

  evaluate     the static evaluation from the bitboards of ``board_at(0)``
  terminal     position_result with a repetition count of 1: (is over, side to move is mated)
  tactical     the class of a move for the order below the root
  alphabeta    the search as specified: move order, node count, node limit -> (move id, score, nodes, flag)
  minimax      no pruning, generation order everywhere, first maximum -> (move id, score)
  play_ply     the move a side of depth d plays, pushed
"""
from oracle.chess_oracle import lib as oracle_lib, move_to_uci

MAX_DEPTH, INF, MATE = 5, 32000, 30000
CUT, SKIPPED = 1, 2
NO_MOVE = 0xFFFF
NODE_LIMIT = 200000
MATERIAL = (100, 320, 330, 500, 900, 0)          # P N B R Q K


def ring(sq):
    f, r = sq & 7, sq >> 3
    return min(f, 7 - f, r, 7 - r)


def evaluate(game):
    b = game.board_at(0)
    total = 0
    for pt in range(6):
        bb = int(b.bb[pt])
        for sq in range(64):
            if not (bb >> sq) & 1:
                continue
            white = (int(b.white) >> sq) & 1
            rg, rank = ring(sq), sq >> 3
            bonus = (5 * rg + 6 * ((rank - 1) if white else (6 - rank)), 10 * rg, 5 * rg, 0, 2 * rg, -10 * rg)[pt]
            total += (MATERIAL[pt] + bonus) * (1 if white else -1)
    return total if int(b.state) & 1 else -total


def terminal(game, n_legal):
    """(over, mated) of the position as position_result(b, n, in_check, 1) decides it: no repetition."""
    L = oracle_lib()
    clock = (int(game.board_at(0).state) >> 12) & 255
    if clock >= 100 and n_legal > 0:
        return True, False                                   # the fifty-move claim
    if n_legal == 0:
        return True, bool(L.og_in_check(game._h))
    if L.og_insufficient(game._h) or clock >= 150:
        return True, False
    return False, False


def tactical(game, m):
    b = game.board_at(0)
    occ = 0
    for pt in range(6):
        occ |= int(b.bb[pt])
    own = int(b.white) if int(b.state) & 1 else occ & ~int(b.white)
    frm, to, promo = m & 63, (m >> 6) & 63, (m >> 12) & 7
    if promo:
        return True
    if (occ & ~own) >> to & 1:
        return True
    return bool((int(b.bb[0]) >> frm) & 1 and (frm & 7) != (to & 7) and not (occ >> to) & 1)


def child(game, m):
    g = game.get_copy()
    assert oracle_lib().og_push(g._h, m)
    return g


class _Cut(Exception):
    pass


def alphabeta(game, depth, node_limit=NODE_LIMIT):
    """(move id, score, nodes, flag) of the search of ``game``'s current position, as opponent.hpp states it."""
    assert 1 <= depth <= MAX_DEPTH and node_limit >= 1
    if game.get_result() is not None:
        return NO_MOVE, 0, 0, SKIPPED
    st = {"nodes": 0, "best": (NO_MOVE, -INF), "first": NO_MOVE}

    def node(g, k, alpha, beta):
        if st["nodes"] >= node_limit:
            raise _Cut()
        moves = g.legal_move_ids()
        st["nodes"] += 1
        over, mated = terminal(g, len(moves))
        if over:
            return -(MATE - k) if mated else 0
        if k == depth:
            return evaluate(g)
        if k > 0:
            moves = [m for m in moves if tactical(g, m)] + [m for m in moves if not tactical(g, m)]
        else:
            st["first"] = moves[0]
        best = -INF
        for m in moves:
            sc = -node(child(g, m), k + 1, -beta, -alpha)
            if sc > best:
                best = sc
                if k == 0:
                    st["best"] = (m, sc)
            alpha = max(alpha, sc)
            if alpha >= beta:
                break
        return best

    try:
        score = node(game, 0, -INF, INF)
    except _Cut:
        m, sc = st["best"]
        return (m if m != NO_MOVE else st["first"]), sc, st["nodes"], CUT
    return st["best"][0], score, st["nodes"], 0


def minimax(game, depth):
    """(move id, score): plain minimax, generation order, the first maximum."""
    def node(g, k):
        moves = g.legal_move_ids()
        over, mated = terminal(g, len(moves))
        if over:
            return NO_MOVE, (-(MATE - k) if mated else 0)
        if k == depth:
            return NO_MOVE, evaluate(g)
        best, bm = None, NO_MOVE
        for m in moves:
            sc = -node(child(g, m), k + 1)[1]
            if best is None or sc > best:
                best, bm = sc, m
        return bm, best

    return node(game, 0)


def play_ply(game, depth, node_limit=NODE_LIMIT):
    """The built-in player of ``depth`` moves in ``game``; returns the move id (NO_MOVE on a finished game)."""
    m = alphabeta(game, depth, node_limit)[0]
    if m != NO_MOVE:
        assert game.move(move_to_uci(m))
    return m
