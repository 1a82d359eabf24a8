"""Host reference of the per-move endgame solve (rvz_solve_moves), on top of tests/solve_ref.py,
tests/solve_window_ref.py and the CPU oracle.

moves_ab(g, bs, alpha, beta)  the definition of include/rvz.h applied literally: make_move per
                  legal square, then solve_window_ref.window_ab on the child with the mapped
                  window; a pass root is window_ab of the root itself at the pass index:
                  (scores [S*S+1], count, nodes [S*S+1]) as lists. max_empties and node_limit are
                  optional: rows above max_empties get count -3, and a move whose search needs
                  more than node_limit positions is ABANDONED with nodes = node_limit (what
                  rvz_solve_window reports for such a row).
host_moves_solver records_to_training's `moves_solver` on the host.
"""
import functools

import numpy as np

import solve_ref as R
import solve_window_ref as W

O = R.O
NOT_A_MOVE, ABANDONED = -128, -127


def malformed(g, bs):
    full = (1 << bs * bs) - 1
    return bool(g.black & g.white) or bool((g.black | g.white) & ~full) or g.side not in (1, 2)


def _limited(r, k, node_limit):
    """rvz_solve_window's (score, nodes) of a searched position under node_limit: the search
    completes exactly when its k positions are at most node_limit."""
    if node_limit is not None and k > node_limit:
        return ABANDONED, node_limit
    return r, k


def moves_ab(g, bs, alpha, beta, max_empties=None, node_limit=None):
    nsq = bs * bs
    scores, nodes = [NOT_A_MOVE] * (nsq + 1), [0] * (nsq + 1)
    if malformed(g, bs):
        return scores, -5, nodes
    if g.over:
        return scores, -2, nodes
    if max_empties is not None and R.empties(g, bs) > max_empties:
        return scores, -3, nodes
    M = R.mover_mask(g, bs)
    if not M:
        r, _, k = W.window_ab(g, bs, alpha, beta)
        scores[nsq], nodes[nsq] = _limited(r, k, node_limit)
        return scores, 1, nodes
    for sq in R.squares(M):
        c = g.copy()
        assert O.make_move(c, sq, bs)
        if c.over:
            assert c.side == g.side
            scores[sq], nodes[sq] = R.discs_diff(c), 1
        elif c.side == g.side:
            r, _, k = W.window_ab(c, bs, alpha, beta)
            scores[sq], nodes[sq] = _limited(r, k, node_limit)
        else:
            r, _, k = W.window_ab(c, bs, -beta, -alpha)
            scores[sq], nodes[sq] = _limited(-r, k, node_limit)
    return scores, bin(M).count("1"), nodes


@functools.lru_cache(maxsize=None)
def _moves_ab_seed(seed, empties, bs, alpha, beta):
    s, c, k = moves_ab(R.position(seed, empties, bs)[0], bs, alpha, beta)
    return tuple(s), c, tuple(k)


def moves_ab_seed(seed, empties, bs, alpha, beta):
    """moves_ab of solve_ref.position(seed, empties, bs), computed once per session."""
    return _moves_ab_seed(seed, empties, bs, alpha, beta)


def stack(rows):
    """[(scores, count, nodes)] -> (int32 [n, S*S+1], int32 [n], int64 [n, S*S+1]) numpy arrays."""
    return (np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32),
            np.array([r[2] for r in rows], np.int64))


def clamp(x, alpha, beta):
    return min(max(x, alpha), beta)


def host_best_moves(scores, count, alpha, beta):
    """rvz.best_moves by direct evaluation: (best, mask list, complete) of one row."""
    complete = count >= 1 and ABANDONED not in scores
    if not complete:
        return 0, [False] * len(scores), False
    vals = [clamp(x, alpha, beta) if x > ABANDONED else None for x in scores]
    best = max(v for v in vals if v is not None)
    return best, [v == best for v in vals], True


def host_moves_solver(black, white, status, board_size, max_empties, alpha=-64, beta=64,
                      abandoned=()):
    """records_to_training's `moves_solver` on the host: torch CPU tensors in, (scores, count,
    nodes) out by moves_ab; in the rows whose index is in `abandoned` the lowest legal entry is
    ABANDONED."""
    import torch
    b = black.numpy().view(np.uint64)
    w = white.numpy().view(np.uint64)
    st = status.numpy()
    rows = []
    for i in range(len(b)):
        g = O.Game(int(b[i]), int(w[i]), int(st[i, 0]), int(st[i, 1]), int(st[i, 2]),
                   int(st[i, 3]))
        s, c, k = moves_ab(g, board_size, alpha, beta, max_empties=max_empties)
        if i in abandoned and c >= 1:
            s[next(j for j, x in enumerate(s) if x != NOT_A_MOVE)] = ABANDONED
        rows.append((s, c, k))
    return tuple(torch.from_numpy(a) for a in stack(rows))
