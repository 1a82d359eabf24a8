"""Host reference of the board-symmetry augmentation (rvz_board_symmetry, rvz_training_rows,
records_to_training(symmetries=...)), written from the definition alone:

    k = 4*f + r,   T_k(x) = np.fliplr(np.rot90(x, r)) if f else np.rot90(x, r)

on unpacked [S, S] arrays indexed (row, col); a bitboard is the 0/1 array with square
s = row*S + col at bit s; a policy row transforms its first S*S entries, the pass stays. It shares
no code with the product: arrays are unpacked, transformed by NumPy and packed again, legal masks
come from the CPU oracle (oracle/oracle.py).

image(x, k)                 T_k of an array whose first two axes are (row, col)
unpack / pack               bitboards <-> [S, S, n] 0/1 arrays
image_bits, image_policy    the images of bitboards and policy rows
COMPOSE, INVERSE            the group table, derived by transforming an index array
training_rows(...)          the three outputs of rvz_training_rows
positions(bs), policies(bs), reference(bs)   the shared test set and its fan = 8 answer, computed
                            once per session and handed out read-only
"""
import functools
import os

import numpy as np

from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def image(x, k: int):
    """T_k of x; x's first two axes are (row, col), further axes ride along."""
    assert 0 <= k < 8
    f, r = divmod(k, 4)
    y = np.rot90(x, r)
    return np.fliplr(y) if f else y


def unpack(bits, S: int) -> np.ndarray:
    """uint64 [n] -> uint8 [S, S, n]; bits at or above S*S are dropped."""
    b = np.asarray(bits, dtype=np.uint64).reshape(-1)
    sq = np.arange(S * S, dtype=np.uint64).reshape(S * S, 1)
    return ((b[None, :] >> sq) & np.uint64(1)).astype(np.uint8).reshape(S, S, -1)


def pack(arr) -> np.ndarray:
    """0/1 [S, S, n] -> uint64 [n]."""
    S = arr.shape[0]
    flat = np.ascontiguousarray(arr).reshape(S * S, -1).astype(np.uint64)
    sq = np.arange(S * S, dtype=np.uint64).reshape(S * S, 1)
    return np.bitwise_or.reduce(flat << sq, axis=0)


def image_bits(bits, k: int, S: int) -> np.ndarray:
    return pack(image(unpack(bits, S), k))


def image_policy(rows, k: int, S: int) -> np.ndarray:
    """[n, S*S+1] -> [n, S*S+1]: the squares as an [S, S] array, the pass in place."""
    rows = np.asarray(rows)
    n = rows.shape[0]
    sq = image(rows[:, :S * S].T.reshape(S, S, n), k)
    return np.concatenate([np.ascontiguousarray(sq).reshape(S * S, n).T, rows[:, S * S:]], axis=1)


def _tables():
    idx = np.arange(16).reshape(4, 4)                     # 4x4 tells all eight images apart
    imgs = [image(idx, k).tobytes() for k in range(8)]
    assert len(set(imgs)) == 8
    compose = [[imgs.index(image(image(idx, b), a).tobytes()) for b in range(8)] for a in range(8)]
    inverse = [compose_row.index(0) for compose_row in
               [[compose[c][k] for c in range(8)] for k in range(8)]]
    return compose, inverse


COMPOSE, INVERSE = _tables()     # T_a(T_b(x)) == T_COMPOSE[a][b](x);  T_INVERSE[k](T_k(x)) == x


def mover_opp(black, white, side):
    black, white = np.asarray(black, np.uint64), np.asarray(white, np.uint64)
    mine = np.asarray(side) == 1
    return np.where(mine, black, white), np.where(mine, white, black)


def legal_masks(P, Q, S: int) -> np.ndarray:
    return np.array([O.legal(int(p), int(q), S) for p, q in zip(P, Q)], dtype=np.uint64)


def canonical(black, white, side, S: int) -> np.ndarray:
    """The oracle's get_canonical_state of every row: float32 [n, 3, S, S]."""
    out = np.zeros((len(black), 3, S, S), np.float32)
    for i in range(len(black)):
        out[i] = O.canonical(O.Game(int(black[i]), int(white[i]), int(side[i])), S)
    return out


def quirk_flags(black, white, side, k: int, S: int) -> np.ndarray:
    """1 where the oracle's legal mask of the image position differs from the image of its mask
    of the original."""
    P, Q = mover_opp(black, white, side)
    moved = image_bits(legal_masks(P, Q, S), k, S)
    own = legal_masks(image_bits(P, k, S), image_bits(Q, k, S), S)
    return (own != moved).astype(np.int32)


def training_rows(black, white, side, policy, sym, S: int, all_images: bool = False):
    """rvz_training_rows' outputs (states f32 [m, 3, S, S], policy f32 [m, S*S+1], quirk i32 [m]).
    all_images: m = 8n, row 8*i + k the image under T_k; else m = n, row i under T_sym[i], a sym
    outside [0, 8) giving a zero row with quirk -1."""
    n = len(black)
    policy = np.asarray(policy, np.float32).reshape(n, S * S + 1)
    planes = canonical(black, white, side, S)                       # [n, 3, S, S]
    per_k = []
    for k in range(8):
        st = np.ascontiguousarray(image(planes.transpose(2, 3, 0, 1), k)).transpose(2, 3, 0, 1)
        per_k.append((st, image_policy(policy, k, S), quirk_flags(black, white, side, k, S)))
    if all_images:
        states = np.stack([p[0] for p in per_k], axis=1).reshape(8 * n, 3, S, S)
        pol = np.stack([p[1] for p in per_k], axis=1).reshape(8 * n, S * S + 1)
        quirk = np.stack([p[2] for p in per_k], axis=1).reshape(8 * n)
        return np.ascontiguousarray(states), np.ascontiguousarray(pol), quirk
    sym = np.asarray(sym).reshape(n)
    states = np.zeros((n, 3, S, S), np.float32)
    pol = np.zeros((n, S * S + 1), np.float32)
    quirk = np.full(n, -1, np.int32)
    for k in range(8):
        m = sym == k
        states[m], pol[m], quirk[m] = per_k[k][0][m], per_k[k][1][m], per_k[k][2][m]
    return states, pol, quirk


def augment(black, white, status, policy, sym, board_size, all_images):
    """records_to_training's `augment` on CPU tensors, by the functions above."""
    import torch
    b = black.numpy().view(np.uint64)
    w = white.numpy().view(np.uint64)
    st, pol, q = training_rows(b, w, status.numpy()[:, 0], policy.numpy(),
                               None if sym is None else sym.numpy(), board_size, all_images)
    return torch.from_numpy(st), torch.from_numpy(pol), torch.from_numpy(q)


# ---------------------------------------------------------------- the shared test set
def _random_playouts(S: int, games: int, seed: int):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(games):
        g = O.new_game(S)
        while not g.over:
            rows.append((int(g.black), int(g.white), int(g.side)))
            P, Q = (g.black, g.white) if g.side == 1 else (g.white, g.black)
            m = O.legal(P, Q, S)
            assert O.make_move(g, int(rng.choice([s for s in range(S * S) if m >> s & 1])), S)
    return rows


@functools.lru_cache(maxsize=None)
def positions(S: int):
    """(black, white, side), uint64 / uint64 / int32 [n], in a seeded random order so that every
    prefix mixes the sources. 8x8: 400 rows spread over tests/golden/board_vectors.npz (positions
    of real games) and all of board_vectors_synthetic.npz (long wrapping runs, explicit passes,
    sparse, one-colour, empty and full boards). 6x6: the synthetic twin of
    tests/synthetic_positions.py answered by the oracle, and oracle playouts."""
    if S == 8:
        rows = []
        with np.load(os.path.join(GOLDEN, "board_vectors.npz")) as z:
            pick = np.linspace(0, len(z["black"]) - 1, 400).astype(np.int64)
            rows += list(zip(z["black"][pick], z["white"][pick], z["side"][pick]))
        with np.load(os.path.join(GOLDEN, "board_vectors_synthetic.npz")) as z:
            rows += list(zip(z["black"], z["white"], z["side"]))
    else:
        import synthetic_positions as SP
        rows = [(r[1], r[2], r[3]) for r in SP.rows(S, 314, lambda P, Q: O.legal(P, Q, S))]
        rows += _random_playouts(S, 12, 2718)
    order = np.random.default_rng(1234 + S).permutation(len(rows))
    black = np.array([int(rows[i][0]) for i in order], dtype=np.uint64)
    white = np.array([int(rows[i][1]) for i in order], dtype=np.uint64)
    side = np.array([int(rows[i][2]) for i in order], dtype=np.int32)
    for a in (black, white, side):
        a.setflags(write=False)
    return black, white, side


@functools.lru_cache(maxsize=None)
def policies(S: int) -> np.ndarray:
    """Seeded random float32 rows for positions(S): the mass on the legal squares, or on the pass
    for a position without one; every 16th row has mass on every index, so that a misplaced
    permutation cannot hide behind zeros."""
    black, white, side = positions(S)
    masks = legal_masks(*mover_opp(black, white, side), S)
    rng = np.random.default_rng(99 + S)
    n, nsq = len(black), S * S
    raw = rng.random((n, nsq + 1)) + 0.01
    on = ((masks[:, None] >> np.arange(nsq, dtype=np.uint64)[None, :]) & np.uint64(1)) != 0
    keep = np.concatenate([on, (masks == 0)[:, None]], axis=1)
    keep[::16] = True
    raw = np.where(keep, raw, 0.0)
    pol = (raw / raw.sum(axis=1, keepdims=True)).astype(np.float32)
    pol.setflags(write=False)
    return pol


@functools.lru_cache(maxsize=None)
def reference(S: int):
    """training_rows(all_images=True) of positions(S) with policies(S): (states, policy, quirk),
    read-only. Row 8*i + k answers input row i under T_k, whatever the batch it travels in."""
    black, white, side = positions(S)
    out = training_rows(black, white, side, policies(S), None, S, all_images=True)
    for a in out:
        a.setflags(write=False)
    return out


def reference_rows(S: int, rows, sym):
    """The fan = 1 answer for input rows `rows` of positions(S) under sym (one per row), read from
    reference(S); a sym outside [0, 8) gives a zero row and quirk -1."""
    st, pol, q = reference(S)
    rows, sym = np.asarray(rows), np.asarray(sym)
    ok = (sym >= 0) & (sym < 8)
    at = 8 * rows + np.where(ok, sym, 0)
    states, policy, quirk = st[at].copy(), pol[at].copy(), q[at].copy()
    states[~ok], policy[~ok], quirk[~ok] = 0.0, 0.0, -1
    return states, policy, quirk
