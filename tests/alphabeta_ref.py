"""Host reference of the depth-limited heuristic search (rvz_alphabeta) and the inputs its tests
share.

Everything here runs on the CPU oracle (oracle/oracle.py: legal / make_move follow board.py and
game.py literally, quirks included), so it is independent of the HIP kernel under test.

negamax(g, depth, weights, bs)    the unpruned definition of include/rvz.h's rvz_alphabeta:
                                  (score, move, nodes)
alphabeta(g, depth, weights, bs)  the same score and move by fail-soft alpha-beta with full-window
                                  root children (for depths brute force is too slow for)
default_table(bs)                 the table DESIGN.md documents, written out here by hand (the
                                  package's alphabeta_weights() is checked against it)
asymmetric_table(bs)              a seeded random table without any symmetry: a kernel that
                                  transposes or mirrors square indices cannot pass with it
playouts(bs)                      64 opening and midgame playout positions; late(bs) the late ones
"""
import functools
import random

import solve_ref as R
from oracle import oracle as O

WIN = 20000          # RVZ_AB_WIN
HEUR_MAX = 16000     # RVZ_AB_HEUR_MAX
MAX_DEPTH = 12       # RVZ_AB_MAX_DEPTH
INF = 10 ** 6


def default_table(bs: int):
    """Corners 100, X-squares -50, C-squares -20, edges 10 / 5, second ring -2, centre -1;
    mobility 10."""
    if bs == 8:
        rows = [[100, -20, 10, 5, 5, 10, -20, 100],
                [-20, -50, -2, -2, -2, -2, -50, -20],
                [10, -2, -1, -1, -1, -1, -2, 10],
                [5, -2, -1, -1, -1, -1, -2, 5]]
    else:
        rows = [[100, -20, 10, 10, -20, 100],
                [-20, -50, -2, -2, -50, -20],
                [10, -2, -1, -1, -2, 10]]
    rows = rows + rows[::-1]
    return tuple(x for r in rows for x in r) + (10,)


def asymmetric_table(bs: int):
    rng = random.Random(1000 + bs)
    return tuple(rng.randrange(-90, 91) for _ in range(bs * bs)) + (7,)


def table_bound(weights, bs: int) -> int:
    nsq = bs * bs
    return sum(abs(x) for x in weights[:nsq]) + nsq * abs(weights[nsq])


def terminal(g) -> int:
    d = R.discs_diff(g)
    return WIN + d if d > 0 else (d - WIN if d < 0 else 0)


def heuristic(g, weights, bs: int) -> int:
    P, Q = (g.black, g.white) if g.side == 1 else (g.white, g.black)
    h = weights[bs * bs] * (bin(O.legal(P, Q, bs)).count("1") - bin(O.legal(Q, P, bs)).count("1"))
    for s in R.squares(P):
        h += weights[s]
    for s in R.squares(Q):
        h -= weights[s]
    return h


def negamax(g, depth: int, weights, bs: int = 8):
    """(score, move, nodes) of the definition: move is a square, -1 for the pass, None when g is
    over or a frontier node; nodes counts every position visited, g included."""
    if g.over:
        return terminal(g), None, 1
    if depth == 0:
        return heuristic(g, weights, bs), None, 1
    M = R.mover_mask(g, bs)
    if not M:                                  # the pass costs no depth
        c = g.copy()
        assert O.make_move(c, -1, bs) and c.side != g.side
        v, _, k = negamax(c, depth, weights, bs)
        return -v, -1, 1 + k
    best, best_sq, nodes = -INF, None, 1
    for sq in R.squares(M):
        c = g.copy()
        assert O.make_move(c, sq, bs)
        v, _, k = negamax(c, depth - 1, weights, bs)
        nodes += k
        if c.side != g.side:
            v = -v
        if v > best:
            best, best_sq = v, sq
    return best, best_sq, nodes


def _ab(g, depth, weights, bs, alpha, beta):
    if g.over:
        return terminal(g)
    if depth == 0:
        return heuristic(g, weights, bs)
    M = R.mover_mask(g, bs)
    if not M:
        c = g.copy()
        O.make_move(c, -1, bs)
        return -_ab(c, depth, weights, bs, -beta, -alpha)
    best = -INF
    for sq in R.squares(M):
        c = g.copy()
        O.make_move(c, sq, bs)
        if c.side == g.side:
            v = _ab(c, depth - 1, weights, bs, alpha, beta)
        else:
            v = -_ab(c, depth - 1, weights, bs, -beta, -alpha)
        if v > best:
            best = v
            if best > alpha:
                alpha = best
            if alpha >= beta:
                break
    return best


def alphabeta(g, depth: int, weights, bs: int = 8):
    """(score, move) of the definition; every root child is searched with the full window, so
    its value is exact and the strict comparison keeps the first maximum."""
    if g.over:
        return terminal(g), None
    M = R.mover_mask(g, bs)
    if not M:
        c = g.copy()
        O.make_move(c, -1, bs)
        return -_ab(c, depth, weights, bs, -INF, INF), -1
    best, best_sq = -INF, None
    for sq in R.squares(M):
        c = g.copy()
        O.make_move(c, sq, bs)
        v = _ab(c, depth - 1, weights, bs, -INF, INF)
        if c.side != g.side:
            v = -v
        if v > best:
            best, best_sq = v, sq
    return best, best_sq


def expected_move(g, move, bs: int) -> int:
    """The host move in rvz_alphabeta's encoding."""
    return R.expected_move(g, move, bs)


TABLES = {"default": default_table, "asymmetric": asymmetric_table}


def playouts(bs: int):
    """64 opening and midgame positions: seeded playouts stopped at a spread of disc counts,
    from the second move to 14 empty squares."""
    nsq = bs * bs
    stops = [nsq - 5, nsq - 8, nsq - 14, nsq - 20, nsq // 2 + 2, nsq // 2 - 4, 18, 14]
    return [R.position(s, stops[s % len(stops)], bs)[0] for s in range(64)]


def late(bs: int):
    """Late positions: 9, 7, 5 and 3 empty squares, three seeds each (at most 9: a search of
    RVZ_AB_MAX_DEPTH plies reaches the end of the game)."""
    return [R.position(s, e, bs)[0] for e in (9, 7, 5, 3) for s in (1, 2, 3)]


@functools.lru_cache(maxsize=None)
def host_negamax(bs: int, table: str, depth: int):
    """negamax of playouts(bs) + late(bs), computed once per session and shared:
    ((score, move in rvz_alphabeta's encoding, nodes), ...)."""
    wt = TABLES[table](bs)
    out = []
    for g in playouts(bs) + late(bs):
        s, m, k = negamax(g, depth, wt, bs)
        out.append((s, expected_move(g, m, bs), k))
    return tuple(out)
