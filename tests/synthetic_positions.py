"""Synthetic positions: states no game from the start position reaches (make_move auto-passes
inside the call, so a live position whose mover has no legal square never occurs in a playout),
built bit by bit from a seeded random.Random. Shared by tests/golden/make_golden.py
(make_synthetic_vectors, which records the reference's answers for the 8x8 rows into
tests/golden/board_vectors_synthetic.npz) and by the tests (the 6x6 twin, answered by the oracle).

rows(bs, seed, legal_fn)  [(kind, black, white, side, passed, move)]: the positions and the one
                          move tried on each. legal_fn(P, Q) is the legal mask of the side whose
                          discs are P (the reference's get_valid_moves or the oracle's legal).
coverage(d)               the counts a fixture must reach, from the fixture's arrays alone.

Kinds (the `kind` column):
  0 (a) uniform random occupancy at 0, 2, 8, 32, 56, 62 and 64 discs (scaled to the board), each
        disc coloured at random
  1 (b) one colour absent
  2 (c) a full edge row or column of one colour against a single disc of the other on every other
        border square (corners, bit 0 and the top bit included)
  3 (d) runs of opponent discs in index order (shift +-1, wrapping across row ends; 7 to 15 exceed
        move generation's seed + 5 steps, 4 to 6 stay inside it) and diagonal runs crossing the
        a/h files, each capped by a mover disc and an empty square
  4 (e) every position of (a) to (d) whose mover has no legal square, twice: passed 0 and 1, the
        move -1
  5 (f) the positions of (e) with a square tried instead
Moves of (a) to (d): about 70% a legal square (where there is one), 15% any square, 15% -1.
"""
import random

A, B, C, D, E, F = range(6)
KIND_NAMES = "abcdef"

# what tests/golden/board_vectors_synthetic.npz must hold at least (coverage()'s keys)
REQUIRED = {"passes_ok": 100, "passes_end": 50, "passes_refused": 50, "sparse": 100, "full": 20,
            "non_standard": 200}


def popcount(x: int) -> int:
    return bin(x).count("1")


def _split(cells, rng):
    """Colour every cell at random: (black, white)."""
    b = w = 0
    for c in cells:
        if rng.random() < 0.5:
            b |= 1 << c
        else:
            w |= 1 << c
    return b, w


def _as_colours(mover, opp, side):
    return (mover, opp) if side == 1 else (opp, mover)


def _kind_a(bs, rng):
    nsq = bs * bs
    # the 8x8 densities, and on a smaller board the same distances from empty and from full
    dens = {0: 8, 2: 150, 8: 250, nsq // 2: 300, nsq - 8: 300, nsq - 2: 250, nsq: 40}
    for n, count in dens.items():
        for _ in range(count):
            b, w = _split(rng.sample(range(nsq), n), rng)
            yield b, w, rng.choice((1, 2))


def _kind_b(bs, rng):
    nsq = bs * bs
    for _ in range(150):
        n = rng.choice((1, 2, 3, 8, nsq // 2, nsq - 7, nsq - 4, nsq - 1, nsq))
        discs = sum(1 << c for c in rng.sample(range(nsq), n))
        yield (discs, 0, rng.choice((1, 2))) if rng.random() < 0.5 else (0, discs, rng.choice((1, 2)))


def _kind_c(bs, rng):
    nsq = bs * bs
    lines = [[c for c in range(bs)], [nsq - bs + c for c in range(bs)],
             [r * bs for r in range(bs)], [r * bs + bs - 1 for r in range(bs)]]
    border = [s for s in range(nsq) if s // bs in (0, bs - 1) or s % bs in (0, bs - 1)]
    for line in lines:
        full = sum(1 << c for c in line)
        inner = [s for s in range(nsq) if s not in border]
        for single in [s for s in border if s not in line] + rng.sample(inner, 4):
            for line_is_mover in (True, False):
                side = rng.choice((1, 2))
                mover, opp = (full, 1 << single) if line_is_mover else (1 << single, full)
                yield (*_as_colours(mover, opp, side), side)


def _with_noise(mover, opp, used, nsq, rng):
    """Half of the time, up to 6 more discs on cells the construction does not use."""
    if rng.random() < 0.5:
        free = [s for s in range(nsq) if not used >> s & 1]
        for c in rng.sample(free, min(len(free), rng.randrange(1, 7))):
            if rng.random() < 0.5:
                mover |= 1 << c
            else:
                opp |= 1 << c
    return mover, opp


def _run(start, step, n, nsq):
    """cells start, start + step, ..., start + (n + 1) * step, or None when they leave the board."""
    cells = [start + k * step for k in range(n + 2)]
    return cells if all(0 <= c < nsq for c in cells) else None


def _kind_d(bs, rng):
    nsq = bs * bs
    # index-order runs: mover, n opponents, empty; in both directions
    for n in range(4, 16):
        for step in (1, -1):
            for _ in range(6):
                cells = None
                while cells is None:
                    cells = _run(rng.randrange(nsq), step, n, nsq)
                yield _capped(cells, nsq, rng)
    # diagonal runs whose cells cross the a/h files (the column wraps somewhere along the run)
    for mag in (bs + 1, bs - 1):
        for step in (mag, -mag):
            for n in range(1, bs - 1):
                done = tries = 0
                while done < 5 and tries < 10000:
                    tries += 1
                    cells = _run(rng.randrange(nsq), step, n, nsq)
                    if cells is None:
                        continue
                    cols = [c % bs for c in cells]
                    if all(abs(x - y) == 1 for x, y in zip(cols, cols[1:])):
                        continue                      # an honest diagonal: no wrap
                    done += 1
                    yield _capped(cells, nsq, rng)


def _capped(cells, nsq, rng):
    mover, opp = 1 << cells[0], sum(1 << c for c in cells[1:-1])
    used = sum(1 << c for c in cells)
    mover, opp = _with_noise(mover, opp, used, nsq, rng)
    side = rng.choice((1, 2))
    return (*_as_colours(mover, opp, side), side)


def rows(bs, seed, legal_fn):
    rng = random.Random(seed)
    nsq = bs * bs
    out, stuck = [], []
    for kind, gen in ((A, _kind_a), (B, _kind_b), (C, _kind_c), (D, _kind_d)):
        for black, white, side in gen(bs, rng):
            assert black & white == 0 and (black | white) >> nsq == 0
            P, Q = (black, white) if side == 1 else (white, black)
            legal = legal_fn(P, Q)
            roll = rng.random()
            if roll < 0.70 and legal:
                move = rng.choice([s for s in range(nsq) if legal >> s & 1])
            elif roll < 0.85:
                move = rng.randrange(nsq)
            else:
                move = -1
            out.append((kind, black, white, side, int(rng.random() < 0.25), move))
            if not legal:
                stuck.append((black, white, side))
    for black, white, side in stuck:
        for passed in (0, 1):
            out.append((E, black, white, side, passed, -1))
    for black, white, side in stuck:
        out.append((F, black, white, side, rng.choice((0, 1)), rng.randrange(nsq)))
    return out


def coverage(d, bs=8):
    """The counts of REQUIRED from a fixture's arrays (board_vectors.npz keys) alone."""
    import numpy as np

    from solve_ref import standard_legal
    full = (1 << bs * bs) - 1
    occ = [int(b) | int(w) for b, w in zip(d["black"], d["white"])]
    is_pass = d["move"] == -1
    non_standard = 0
    for b, w, s, lm in zip(d["black"], d["white"], d["side"], d["legal"]):
        P, Q = (int(b), int(w)) if s == 1 else (int(w), int(b))
        non_standard += standard_legal(P, Q, bs) != int(lm)
    return {"passes_ok": int(np.sum(is_pass & (d["ok"] == 1))),
            "passes_end": int(np.sum(is_pass & (d["ok"] == 1) & (d["over_after"] == 1))),
            "passes_refused": int(np.sum(is_pass & (d["ok"] == 0))),
            "sparse": sum(popcount(o) < 4 for o in occ),
            "full": sum(o == full for o in occ),
            "non_standard": non_standard}


def check_coverage(d, bs=8, required=REQUIRED):
    got = coverage(d, bs)
    print("synthetic fixture: %d rows; " % len(d["black"]) +
          ", ".join(f"{k} {got[k]} (>= {v})" for k, v in required.items()))
    for k, v in required.items():
        assert got[k] >= v, (k, got[k], v)
    return got
