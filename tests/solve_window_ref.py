"""Host reference of the windowed endgame solve (rvz_solve_window), on top of tests/solve_ref.py
and the CPU oracle.

window_ab(g, bs, alpha, beta)  fail-soft alpha-beta in increasing square order with the kernel's
                  root rule (children searched with (max(best, alpha), beta), a pass root's child
                  with the negated window) and the kernel's node counting (every position made by
                  make_move counts one, the root included): (r, move, nodes), move in
                  rvz_solve_window's encoding (-2 over, S*S forced pass, -6 fail low).
                  alpha = -INF, beta = INF is rvz_solve's own search.
child_values(g, bs)  {square: exact value of that root move, from the root's side} by the
                  unpruned solve_ref.negamax.
"""
import functools

import solve_ref as R

O = R.O
INF = R.INF


def _search(g, bs, alpha, beta, count):
    """Fail-soft value of the live position g within (alpha, beta), and its best square."""
    M = R.mover_mask(g, bs)
    best, best_sq = -INF, None
    for sq in (list(R.squares(M)) if M else [-1]):
        c = g.copy()
        assert O.make_move(c, sq, bs)
        count[0] += 1
        a = max(alpha, best)
        if c.over:
            v = R.discs_diff(c) if c.side == g.side else -R.discs_diff(c)
        elif c.side == g.side:
            v = _search(c, bs, a, beta, count)[0]
        else:
            v = -_search(c, bs, -beta, -a, count)[0]
        if v > best:
            best, best_sq = v, sq
        if best >= beta:
            break
    return best, best_sq


def window_ab(g, bs, alpha, beta):
    if g.over:
        return R.discs_diff(g), -2, 1
    count = [1]
    r, sq = _search(g, bs, alpha, beta, count)
    if sq == -1:
        move = bs * bs
    elif r <= alpha:
        move = -6
    else:
        move = sq
    return r, move, count[0]


@functools.lru_cache(maxsize=None)
def _window_ab_seed(seed, empties, bs, alpha, beta):
    return window_ab(R.position(seed, empties, bs)[0], bs, alpha, beta)


def window_ab_seed(seed, empties, bs, alpha, beta):
    """window_ab of solve_ref.position(seed, empties, bs), computed once per session."""
    return _window_ab_seed(seed, empties, bs, alpha, beta)


def child_values(g, bs):
    out = {}
    if g.over:
        return out
    for sq in R.squares(R.mover_mask(g, bs)):
        c = g.copy()
        assert O.make_move(c, sq, bs)
        v = R.negamax(c, bs)[0]
        out[sq] = v if c.side == g.side else -v
    return out


@functools.lru_cache(maxsize=None)
def child_values_seed(seed, empties, bs):
    return child_values(R.position(seed, empties, bs)[0], bs)


def check_result(g, bs, alpha, beta, v, r, move, values=None):
    """Assert rvz_solve_window's contract for one row: v the exact score, (r, move) the answer;
    values = child_values(g, bs) checks that the move qualifies (any qualifying square passes)."""
    nsq = bs * bs
    if g.over:
        assert (r, move) == (R.discs_diff(g), -2), (r, move)
        return
    if alpha < v < beta:
        assert r == v, (r, v, alpha, beta)
    elif v <= alpha:
        assert v <= r <= alpha, (r, v, alpha, beta)
    else:
        assert beta <= r <= v, (r, v, alpha, beta)
    if R.mover_mask(g, bs) == 0:
        assert move == nsq, move
    elif r <= alpha:
        assert move == -6, move
    elif values is not None:
        assert move in values, move
        m = values[move]
        assert (m == v) if r < beta else (m >= beta), (move, m, v, r, beta)
