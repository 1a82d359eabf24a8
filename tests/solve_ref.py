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


def to_device(games):
    """to_arrays(games) as tensors on the current GPU."""
    import torch
    return tuple(torch.from_numpy(a).cuda() for a in to_arrays(games))


def pass_roots(bs, seeds):
    """Roots whose mover has no move: the position after an auto-pass with the side flipped."""
    out = []
    for s in seeds:
        g = last_auto_pass(s, 0, bs)
        assert g is not None and not g.over
        g.side = 3 - g.side
        assert mover_mask(g, bs) == 0
        out.append(g)
    return out


class RootCases:
    """The root-case batch of the solver tests (run at max_empties = 6): 8 plain rows at 6 empties
    with the rows that need no search, or only the pass, mixed in.

    plain    the 8 ordinary rows; mixed[i] for i in keep, in order
    mixed    the batch: a special row after each of the first plain rows, the rest appended
    where    {index in mixed: index in special / expect}
    expect   per special row (score, move, ends): what rvz_solve reports. ends is False for a
             pass root whose pass does not end the game (its score is searched, so only exact
             inside a window) and True for every other row (score holds under any window)
    zero     the batch for max_empties = 0: a full board, the finished game, plain[0] and the pass
             roots; zero_full is the full board
    """

    def __init__(self, bs, seeds):
        nsq = bs * bs
        self.plain = plain = [position(s, 6, bs)[0] for s in range(8)]
        self.special, self.expect = special, expect = [], []
        # a finished game: play a generated position out
        self.over = over = position(3, 0, bs)[0]
        assert over.over
        special.append(over)
        expect.append((discs_diff(over), -2, True))
        # the mover has no move: passed = 0 (the other side plays on, unless it has no move
        # either) and passed = 1 (the game ends)
        for g in pass_roots(bs, seeds):
            for passed in (0, 1):
                c = g.copy()
                c.passed = passed
                hs, hm, _ = negamax(c, bs)
                assert hm == -1
                child = c.copy()
                assert O.make_move(child, -1, bs)
                ends = bool(child.over) or mover_mask(child, bs) == 0
                if passed:
                    assert ends and hs == discs_diff(c)
                special.append(c)
                expect.append((hs, nsq, ends))
        # above max_empties
        special.append(position(0, 7, bs)[0])
        expect.append((0, -3, True))
        # malformed rows: overlap, bits at or above S*S (6x6 only has such bits), side not 1 | 2
        g = plain[0].copy()
        g.white |= g.black & -g.black
        special.append(g)
        expect.append((0, -5, True))
        if bs == 6:
            for bit, col in ((36, "black"), (63, "white")):
                g = plain[1].copy()
                setattr(g, col, getattr(g, col) | 1 << bit)
                special.append(g)
                expect.append((0, -5, True))
        for side in (0, 3, -1):
            g = plain[2].copy()
            g.side = side
            special.append(g)
            expect.append((0, -5, True))
        # mixed into ordinary rows, whose answers must not change
        self.mixed, self.where = mixed, where = [], {}
        for i, g in enumerate(plain):
            mixed.append(g)
            if i < len(special):
                where[len(mixed)] = i
                mixed.append(special[i])
        for j in range(len(plain), len(special)):
            where[len(mixed)] = j
            mixed.append(special[j])
        self.keep = [i for i in range(len(mixed)) if i not in where]
        # max_empties = 0: only full or finished boards are solved
        full = (1 << nsq) - 1
        self.zero_full = O.Game(full & 0x5555555555555555, full & 0xAAAAAAAAAAAAAAAA, 1, 0, -1, 0)
        self.zero = [self.zero_full, over, plain[0]] + pass_roots(bs, seeds)

    def check_zero(self, bs, s0, m0):
        """The answers of the `zero` batch at max_empties = 0."""
        hs, hm, _ = negamax(self.zero_full, bs)
        assert hm == -1 and (s0[0], m0[0]) == (hs, bs * bs)
        assert (s0[1], m0[1]) == (discs_diff(self.over), -2)
        assert list(m0[2:]) == [-3] * (len(self.zero) - 2) and not s0[2:].any()


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


# ---------------------------------------------------------------- synthetic rows (solver tests)
SYNTHETIC_MAX_EMPTIES = 7


@functools.lru_cache(maxsize=None)
def _synthetic_rows(bs: int):
    import os

    import synthetic_positions as SP
    if bs == 8:
        path = os.path.join(os.path.dirname(__file__), "golden", "board_vectors_synthetic.npz")
        with np.load(path) as z:
            d = {k: z[k] for k in ("kind", "black", "white", "side", "passed")}
        rows = [tuple(int(d[k][i]) for k in ("kind", "black", "white", "side", "passed"))
                for i in range(len(d["kind"]))]
    else:
        rows = [r[:5] for r in SP.rows(bs, 314, lambda P, Q: O.legal(P, Q, bs))]
    nsq = bs * bs
    full = (1 << nsq) - 1
    seen, out = set(), []

    def add(black, white, side, passed):
        for s in (side, 3 - side):
            t = (black, white, s, 0, -1, passed)
            if t not in seen:
                seen.add(t)
                out.append(t)

    for kind, black, white, side, passed in rows:
        if kind <= SP.E and nsq - SP.popcount(black | white) <= SYNTHETIC_MAX_EMPTIES:
            add(black, white, side, passed)
    # the fixture's densities leave 3 to 7 empties to one-colour boards only: kind (a)'s
    # construction at those densities too, so that the synthetic batch holds real searches
    rng = random.Random(99)
    for e in range(3, SYNTHETIC_MAX_EMPTIES + 1):
        for _ in range(10):
            black = white = 0
            for c in rng.sample(range(nsq), nsq - e):
                if rng.random() < 0.5:
                    black |= 1 << c
                else:
                    white |= 1 << c
            add(black, white, 1, rng.choice((0, 1)))
    for sq in (0, nsq // 2 + 1, nsq - 1):          # one colour, one square empty
        for passed in (0, 1):
            add(full ^ 1 << sq, 0, 1, passed)
            add(0, full ^ 1 << sq, 1, passed)
    return tuple(out)


def synthetic_rows(bs: int = 8):
    """The solver tests' synthetic batch: the rows of kinds (a) to (e) of
    tests/synthetic_positions.py with at most SYNTHETIC_MAX_EMPTIES empty squares (8x8: the
    committed fixture's positions; 6x6: its twin built with the oracle), each also with the other
    side to move, duplicates dropped, plus 10 random boards at each of 3 to 7 empties (the
    fixture's densities skip them) and the one-colour boards with one empty square."""
    return [O.Game(*t) for t in _synthetic_rows(bs)]


@functools.lru_cache(maxsize=None)
def synthetic_solved(bs: int = 8):
    """negamax of every synthetic row, computed once per session: ((score, move, nodes), ...)."""
    return tuple(negamax(g, bs) for g in synthetic_rows(bs))


def synthetic_kinds(bs: int = 8):
    """Host counts over the synthetic batch: pass roots (no legal square, not over), roots where
    the other side has none either, and roots whose best move (negamax's) flips nothing."""
    n_pass = n_stuck = n_noflip = 0
    for g, (_, move, _) in zip(synthetic_rows(bs), synthetic_solved(bs)):
        P, Q = (g.black, g.white) if g.side == 1 else (g.white, g.black)
        if O.legal(P, Q, bs) == 0:
            n_pass += 1
            n_stuck += O.legal(Q, P, bs) == 0
        elif O.flips(move, P, Q, bs) == 0:
            n_noflip += 1
    return {"pass": n_pass, "stuck": n_stuck, "noflip": n_noflip}


def check_synthetic_kinds(bs: int = 8):
    got = synthetic_kinds(bs)
    print(f"synthetic solver rows {bs}x{bs}: {len(synthetic_rows(bs))} rows, {got}")
    assert min(got.values()) >= 10, got
    return got
