"""Host reference of the exact endgame solver (rvz_solve) and the positions its tests use.

Everything here runs on the CPU oracle (oracle/oracle.py: legal / make_move follow board.py and
game.py literally, quirks included), so it is independent of the HIP kernel under test.

negamax(g, bs)    the unpruned definition of include/rvz.h's rvz_solve: (score, move, nodes)
alphabeta(g, bs)  the same score and move by fail-soft alpha-beta with full-window root children
                  (for roots too deep for brute force in Python)
position(seed, empties, bs)   a random playout from the start position (random.Random(seed), a
                  uniform choice among the legal squares in increasing index) until at most
                  `empties` squares are empty; also reports whether make_move auto-passed
"""
import functools
import random

import numpy as np

from oracle import oracle as O

INF = 1000


def squares(mask: int):
    while mask:
        low = mask & -mask
        yield low.bit_length() - 1
        mask ^= low


def discs_diff(g) -> int:
    b, w = bin(g.black).count("1"), bin(g.white).count("1")
    return b - w if g.side == 1 else w - b


def mover_mask(g, bs: int) -> int:
    P, Q = (g.black, g.white) if g.side == 1 else (g.white, g.black)
    return O.legal(P, Q, bs)


def negamax(g, bs: int = 8):
    """(score, move, nodes) of the definition: move is a square, -1 for the pass, None when g is
    over; nodes counts every position visited, g included."""
    if g.over:
        return discs_diff(g), None, 1
    M = mover_mask(g, bs)
    best, best_sq, nodes = -INF, None, 1
    for sq in (list(squares(M)) if M else [-1]):
        c = g.copy()
        assert O.make_move(c, sq, bs)
        v, _, k = negamax(c, bs)
        nodes += k
        if c.side != g.side:
            v = -v
        if v > best:
            best, best_sq = v, sq
    return best, best_sq, nodes


def _ab(g, bs, alpha, beta):
    if g.over:
        return discs_diff(g)
    M = mover_mask(g, bs)
    best = -INF
    for sq in (list(squares(M)) if M else [-1]):
        c = g.copy()
        O.make_move(c, sq, bs)
        v = _ab(c, bs, alpha, beta) if c.side == g.side else -_ab(c, bs, -beta, -alpha)
        if v > best:
            best = v
            if best > alpha:
                alpha = best
            if alpha >= beta:
                break
    return best


def alphabeta(g, bs: int = 8):
    """(score, move) of the definition; every root child is searched with the full window, so
    its value is exact and the strict comparison keeps the first maximum."""
    if g.over:
        return discs_diff(g), None
    M = mover_mask(g, bs)
    best, best_sq = -INF, None
    for sq in (list(squares(M)) if M else [-1]):
        c = g.copy()
        O.make_move(c, sq, bs)
        v = _ab(c, bs, -INF, INF)
        if c.side != g.side:
            v = -v
        if v > best:
            best, best_sq = v, sq
    return best, best_sq


def expected_move(g, move, bs: int) -> int:
    """The host move in rvz_solve's encoding."""
    if g.over:
        return -2
    return bs * bs if move == -1 else move


def empties(g, bs: int) -> int:
    return bs * bs - bin(g.black | g.white).count("1")


@functools.lru_cache(maxsize=None)
def _position(seed: int, max_empties: int, bs: int):
    rng = random.Random(seed)
    g = O.new_game(bs)
    auto_passed = False
    while not g.over and empties(g, bs) > max_empties:
        mover = g.side
        sq = rng.choice(list(squares(mover_mask(g, bs))))
        assert O.make_move(g, sq, bs)
        if not g.over and g.side == mover:
            auto_passed = True
    return g.astuple(), auto_passed


def position(seed: int, max_empties: int, bs: int = 8):
    """(Game, auto_passed): auto_passed is True when some make_move of the playout kept the side
    (the opponent had no move) without ending the game."""
    t, ap = _position(seed, max_empties, bs)
    g = O.Game(*t)
    return g, ap


def last_auto_pass(seed: int, max_empties: int, bs: int = 8):
    """The position right after the LAST auto-pass of the playout, or None: there the side not
    to move has no legal square while the mover has one."""
    rng = random.Random(seed)
    g = O.new_game(bs)
    found = None
    while not g.over and empties(g, bs) > max_empties:
        mover = g.side
        sq = rng.choice(list(squares(mover_mask(g, bs))))
        assert O.make_move(g, sq, bs)
        if not g.over and g.side == mover:
            found = g.copy()
    return found


def standard_legal(P: int, Q: int, bs: int = 8) -> int:
    """Standard Othello's legal mask (no wrap-around, a move must flip): what an off-the-shelf
    solver would generate."""
    out = 0
    for sq in range(bs * bs):
        if (P | Q) >> sq & 1:
            continue
        r, c = divmod(sq, bs)
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                if dr == 0 and dc == 0:
                    continue
                rr, cc, seen = r + dr, c + dc, 0
                while 0 <= rr < bs and 0 <= cc < bs and Q >> (rr * bs + cc) & 1:
                    rr, cc, seen = rr + dr, cc + dc, seen + 1
                if seen and 0 <= rr < bs and 0 <= cc < bs and P >> (rr * bs + cc) & 1:
                    out |= 1 << sq
    return out


def to_arrays(games):
    """(black int64 [n], white int64 [n], status int32 [n, 4]) numpy arrays (bit patterns)."""
    b = np.array([g.black for g in games], np.uint64).view(np.int64)
    w = np.array([g.white for g in games], np.uint64).view(np.int64)
    st = np.array([[g.side, g.over, g.winner, g.passed] for g in games], np.int32).reshape(-1, 4)
    return b, w, st


@functools.lru_cache(maxsize=None)
def solved(seed: int, max_empties: int, bs: int = 8):
    """(score, move in rvz_solve's encoding, nodes) of position(seed, max_empties, bs) by the
    unpruned negamax; computed once per session and shared."""
    g, _ = position(seed, max_empties, bs)
    s, m, k = negamax(g, bs)
    return s, expected_move(g, m, bs), k


def host_solver(black, white, status, board_size, max_empties, unsolved=()):
    """records_to_training's `solver` on the host: torch CPU tensors in, (score, move, nodes) out
    by the unpruned negamax; rows above max_empties get -3, rows whose index is in `unsolved`
    get -4 (an abandoned row)."""
    import torch
    b = black.numpy().view(np.uint64)
    w = white.numpy().view(np.uint64)
    st = status.numpy()
    n = len(b)
    score, move, nodes = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64)
    for i in range(n):
        g = O.Game(int(b[i]), int(w[i]), int(st[i, 0]), int(st[i, 1]), int(st[i, 2]),
                   int(st[i, 3]))
        if i in unsolved:
            move[i] = -4
        elif not g.over and empties(g, board_size) > max_empties:
            move[i] = -3
        else:
            s, m, k = negamax(g, board_size)
            score[i], move[i], nodes[i] = s, expected_move(g, m, board_size), k
    return torch.from_numpy(score), torch.from_numpy(move), torch.from_numpy(nodes)
