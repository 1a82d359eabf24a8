"""A plain Python restatement of rvz_openings' level rule (include/rvz.h) over the CPU oracle's
legal / make_move (oracle/oracle.py: board.py and game.py followed literally, quirks included),
and of the opening-index draw on the Python Philox of tests/replay_ref.py. Independent of the HIP
kernels under test.

levels(bs, plies)        every level 0 .. plies: its rows in order, its candidate count, the
                         finished children dropped and the duplicates removed on the way to it
openings(bs, plies)      rvz.openings' dict as NumPy arrays
opening_index(s, salt, n)   the pool row seed s picks
"""
import functools

import numpy as np

import replay_ref as RR
from oracle import oracle as O

M32 = 0xFFFFFFFF


def squares(mask: int):
    while mask:
        low = mask & -mask
        yield low.bit_length() - 1
        mask ^= low


def children(row, bs: int):
    """The children of (black, white, side) over its legal squares in increasing index, as
    (black, white, side, over) after make_move (auto-pass and game end inside it)."""
    b, w, s = row
    mask = O.legal(b, w, bs) if s == 1 else O.legal(w, b, bs)
    for sq in squares(mask):
        g = O.Game(b, w, s, 0, -1, 0)
        assert O.make_move(g, sq, bs)
        yield int(g.black), int(g.white), int(g.side), bool(g.over)


@functools.lru_cache(maxsize=None)
def levels(bs: int, plies: int):
    """A tuple of plies + 1 dicts {"rows", "candidates", "dropped", "dups"}; level 0 is the start
    position with black to move and counts as one candidate."""
    first = O.new_game(bs)
    out = [{"rows": [(int(first.black), int(first.white), 1)], "candidates": 1, "dropped": 0,
            "dups": 0}]
    for _ in range(plies):
        seen, cand, dropped = {}, 0, 0
        for row in out[-1]["rows"]:
            for b, w, s, over in children(row, bs):
                if over:
                    dropped += 1
                    continue
                cand += 1
                seen.setdefault((b, w, s), None)            # a dict keeps first occurrences in order
        out.append({"rows": list(seen), "candidates": cand, "dropped": dropped,
                    "dups": cand - len(seen)})
    return tuple(out)


def openings(bs: int, plies: int):
    lv = levels(bs, plies)
    rows = lv[-1]["rows"]
    m = len(rows)
    status = np.zeros((m, 4), np.int32)
    status[:, 0] = [r[2] for r in rows]
    status[:, 2] = -1
    stats = np.array([m, lv[-1]["candidates"], sum(x["dropped"] for x in lv),
                      sum(x["dups"] for x in lv), max(x["candidates"] for x in lv), 0, 0, 0],
                     np.int64)
    return {"black": np.array([r[0] for r in rows], np.uint64),
            "white": np.array([r[1] for r in rows], np.uint64), "status": status, "stats": stats}


def opening_index(seed: int, salt: int, n: int) -> int:
    """i = (x.0 * n) >> 32, x = Philox4x32-10(key (seed, salt), counter (0, 0, 0, 1))."""
    x = RR.philox4x32_10((seed & M32, salt & M32), (0, 0, 0, 1))
    return (x[0] * n) >> 32
