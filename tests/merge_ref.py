"""Host reference of rvz_merge_positions (include/rvz.h), written from the definition alone:

    P = black if side == 1 else white, O = the other; rows with equal (P, O) are one position
    output rows: the distinct positions in order of first occurrence
    q(x) = (int64) rint((float64) x * 2^36); mean = float32(float64(sum q) / (float64(c) * 2^36))
    a group of one copies its row; a malformed row joins no group and gets group -1

A dict keyed by (P, O) walked in row order, int64 sums, one float64 division per entry. It shares
no code with the product.

merge(...)                  the six outputs, as a dict of NumPy arrays (trimmed to m)
host_merger(...)            records_to_training's `merger` on CPU tensors
playout_pool(bs)            positions of oracle random playouts from the start, once per session
mixed_rows(bs, n, seed)     n rows drawn from the pool (early plies repeat naturally) with
                            planted colour-swapped twins and rows that occur once, random
                            policies and outcomes
distinct_rows(bs, n, seed)  n rows of pairwise distinct positions
"""
import functools

import numpy as np

from oracle import oracle as O

Q36 = float(2 ** 36)


def malformed(black, white, side, policy, value, bs: int) -> np.ndarray:
    black, white = np.asarray(black, np.uint64), np.asarray(white, np.uint64)
    side = np.asarray(side)
    off = np.uint64(0) if bs == 8 else ~np.uint64((1 << (bs * bs)) - 1)
    with np.errstate(invalid="ignore"):
        pol_ok = ((policy >= 0) & (policy <= 1)).all(axis=1)            # NaN fails both
        val_ok = (value >= -1) & (value <= 1)
    return ((black & white) != 0) | (((black | white) & off) != 0) | \
        ((side != 1) & (side != 2)) | ~pol_ok | ~val_ok


def merge(black, white, side, policy, value, bs: int = 8) -> dict:
    """black / white uint64 [n], side [n], policy float32 [n, S*S+1], value float32 [n]."""
    black, white = np.asarray(black, np.uint64), np.asarray(white, np.uint64)
    side = np.asarray(side)
    policy = np.asarray(policy, np.float32).reshape(len(black), bs * bs + 1)
    value = np.asarray(value, np.float32).reshape(len(black))
    n = len(black)
    bad = malformed(black, white, side, policy, value, bs)
    group = np.full(n, -1, np.int32)
    seen, first = {}, []
    for i in range(n):
        if bad[i]:
            continue
        b, w = int(black[i]), int(white[i])
        key = (b, w) if side[i] == 1 else (w, b)
        j = seen.get(key)
        if j is None:
            j = seen[key] = len(first)
            first.append(i)
        group[i] = j
    m = len(first)
    first = np.array(first, np.int32).reshape(m)
    ok = ~bad
    count = np.bincount(group[ok], minlength=m).astype(np.int32)
    rows = np.concatenate([policy, value[:, None]], axis=1)
    q = np.rint(rows[ok].astype(np.float64) * Q36).astype(np.int64)
    sums = np.zeros((m, rows.shape[1]), np.int64)
    np.add.at(sums, group[ok], q)
    mean = (sums.astype(np.float64) / (count.astype(np.float64) * Q36)[:, None]).astype(np.float32)
    one = count == 1
    mean[one] = rows[first[one]]                                        # moved, never recomputed
    return {"m": m, "first": first, "count": count, "policy": np.ascontiguousarray(mean[:, :-1]),
            "value": np.ascontiguousarray(mean[:, -1]), "group": group}


def host_merger(black, white, status, policy, value, board_size):
    """records_to_training's `merger` on CPU tensors."""
    import torch
    out = merge(black.numpy().view(np.uint64), white.numpy().view(np.uint64),
                status.numpy()[:, 0], policy.numpy(), value.numpy(), board_size)
    return {k: (v if k == "m" else torch.from_numpy(v)) for k, v in out.items()}


# ---------------------------------------------------------------- test rows
@functools.lru_cache(maxsize=None)
def playout_pool(bs: int):
    """(black, white, side) of every position of 40 oracle random playouts from the start, game
    after game: the start position 40 times, the early plies repeating among the games."""
    rng = np.random.default_rng(4000 + bs)
    rows = []
    for _ in range(40):
        g = O.new_game(bs)
        while not g.over:
            rows.append((int(g.black), int(g.white), int(g.side)))
            P, Q = (g.black, g.white) if g.side == 1 else (g.white, g.black)
            mask = O.legal(P, Q, bs)
            assert O.make_move(g, int(rng.choice([s for s in range(bs * bs) if mask >> s & 1])), bs)
    out = (np.array([r[0] for r in rows], np.uint64), np.array([r[1] for r in rows], np.uint64),
           np.array([r[2] for r in rows], np.int32))
    for a in out:
        a.setflags(write=False)
    return out


def targets(n: int, bs: int, rng):
    """Random float32 policies in [0, 1] (rows summing to about 1, some entries exactly 0 or 1)
    and outcomes in {-1, 0, +1}."""
    raw = rng.random((n, bs * bs + 1)) * (rng.random((n, bs * bs + 1)) < 0.4)
    raw[:, 0] += 1e-3
    pol = (raw / raw.sum(axis=1, keepdims=True)).astype(np.float32)
    pol[::7] = 0.0
    pol[::7, 3] = 1.0                                                   # one-hot rows
    val = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), size=n)
    return np.clip(pol, 0.0, 1.0), val


def mixed_rows(bs: int, n: int, seed: int = 0):
    """(black, white, side, policy, value): n rows drawn from the playout pool, the pool's early
    rows ten times as likely as the rest; every fifth row is stored as its colour-swapped twin
    (black and white exchanged, the other side to move): the same position to the merge; every
    fourth row is a random position that occurs once."""
    pb, pw, ps = playout_pool(bs)
    rng = np.random.default_rng(seed * 1000 + n)
    weight = np.where(np.arange(len(pb)) % (bs * bs - 4) < 6, 10.0, 1.0)
    at = rng.choice(len(pb), size=n, p=weight / weight.sum())
    b, w, s = pb[at].copy(), pw[at].copy(), ps[at].copy()
    twin = np.arange(n) % 5 == 2
    b[twin], w[twin], s[twin] = pw[at][twin], pb[at][twin], 3 - ps[at][twin]
    lone = np.arange(n) % 4 == 3                    # and every fourth a position of its own
    if lone.any():
        b[lone], w[lone], s[lone] = distinct_rows(bs, int(lone.sum()), seed + 1)[:3]
    pol, val = targets(n, bs, rng)
    return b, w, s, pol, val


def distinct_rows(bs: int, n: int, seed: int = 0):
    """n rows whose (mover, opponent) pairs are pairwise distinct: random disjoint bitboards."""
    rng = np.random.default_rng(77 + seed)
    full = np.uint64((1 << (bs * bs)) - 1) if bs < 8 else ~np.uint64(0)
    keys = {}
    while len(keys) < n:
        occ = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + \
            rng.integers(0, 2, size=n, dtype=np.uint64)
        col = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2)
        for P, Q in zip((occ & col & full).tolist(), (occ & ~col & full).tolist()):
            keys.setdefault((P, Q), None)
    keys = list(keys)[:n]
    s = rng.integers(1, 3, size=n).astype(np.int32)
    P = np.array([k[0] for k in keys], np.uint64)
    Q = np.array([k[1] for k in keys], np.uint64)
    b, w = np.where(s == 1, P, Q), np.where(s == 1, Q, P)
    pol, val = targets(n, bs, rng)
    return b, w, s, pol, val
