"""Host reference of weighted replay sampling (rvz_replay_cdf and rvz_replay_batch_weighted,
include/rvz.h), written from the contract alone on Python integers and NumPy arrays; it shares no
code with the product. The generator and the rows themselves come from tests/replay_ref.py.

q(w)                        a float32 weight in fixed point, None where the weight is invalid
cdf(weight, start, live)    the table's contract words [0, 4 + live) as uint64
search(C, t)                the smallest i with C[i] > t
draw(table, seed, step, r, random_sym, word)   output row r's (logical row or -1, symmetry, t)
batch(...)                  rvz_replay_batch_weighted's six outputs
weighted_batcher / cdf_builder   the same on CPU tensors: ReplayBuffer's injection points
WORD_MAX, word_for(t, total)     the largest 64-bit word, and the smallest word that gives t
"""
import bisect
import math

import numpy as np

import replay_ref as RR

M32 = 0xFFFFFFFF
WORD_MAX = (1 << 64) - 1
HEAD = 4


def q(w):
    """rint(w * 2^16) (half to even) as a Python int for a finite w in [0, 65536], else None."""
    w = float(np.float32(w))
    if math.isnan(w) or math.isinf(w) or w < 0.0 or w > 65536.0:
        return None
    return int(np.rint(np.float64(w) * 65536.0))


def cdf(weight, start, live):
    """[total, invalid, start, live, C[0] .. C[live - 1]] as uint64; logical row i is slot
    (start + i) % capacity."""
    weight = np.asarray(weight, np.float32).reshape(-1)
    cap = len(weight)
    assert 0 <= live <= cap and 0 <= start < cap
    w = weight[(start + np.arange(live)) % cap].astype(np.float64)
    valid = np.isfinite(w) & (w >= 0.0) & (w <= 65536.0)
    fixed = np.rint(np.where(valid, w, 0.0) * 65536.0).astype(np.uint64)   # exact: below 2^33
    assert live < 1 << 31                                      # so the sums stay below 2^63
    C = np.cumsum(fixed, dtype=np.uint64)
    total = int(C[-1]) if live else 0
    return np.concatenate([np.array([total, live - int(valid.sum()), start, live], np.uint64), C])


def search(C, t):
    """The smallest i with C[i] > t (C non-decreasing, t < C[-1])."""
    i = bisect.bisect_right(C, t)
    assert i < len(C) and C[i] > t and (i == 0 or C[i - 1] <= t)
    return i


def word_for(t, total):
    """The smallest 64-bit word u with (u * total) >> 64 == t."""
    u = -((-t << 64) // total)
    assert 0 <= u <= WORD_MAX and (u * total) >> 64 == t
    assert u == 0 or ((u - 1) * total) >> 64 < t
    return u


def draw(table, seed, step, r, random_sym=True, word=None):
    """(i, k, t) of output row r: u = word or the block's words 2 and 3, t = (u * total) >> 64,
    i the smallest row with C[i] > t; i = -1 and t = None with total == 0."""
    seed, step = seed % (1 << 64), step % (1 << 64)
    x = RR.philox4x32_10((seed & M32, seed >> 32), (r, step & M32, step >> 32, 0))
    k = (x[1] & 7) if random_sym else 0
    total, live = int(table[0]), int(table[3])
    if not total:
        return -1, k, None
    u = ((x[2] << 32) | x[3]) if word is None else int(word) % (1 << 64)
    t = (u * total) >> 64
    return search([int(c) for c in table[HEAD:HEAD + live]], t), k, t


def batch(mover, opponent, policy, value, table, start, live, nb, seed, step, random_sym=True,
          idx=None, sym=None, word=None, board_size=8):
    """(states, policy, value [nb, 1], slot, sym, prob f32 [nb]). A table built for another
    (start, live) gives zero rows; so does a drawn row with total == 0. word: nb Python
    integers, or an integer array (uint64, or int64 bit patterns)."""
    assert word is None or len(word) == nb
    table = np.asarray(table).view(np.uint64).reshape(-1)
    total = int(table[0])
    fresh = int(table[2]) == start and int(table[3]) == live
    C = [int(c) for c in table[HEAD:HEAD + live]] if fresh else []
    if not fresh:
        i = np.full(nb, -1, np.int64)
    elif idx is not None:
        i = np.asarray(idx).astype(np.int64).reshape(nb)
    elif not total:
        i = np.full(nb, -1, np.int64)
    else:
        seed_, step_ = seed % (1 << 64), step % (1 << 64)
        i = np.zeros(nb, np.int64)
        for r in range(nb):
            if word is None:
                x = RR.philox4x32_10((seed_ & M32, seed_ >> 32), (r, step_ & M32, step_ >> 32, 0))
                u = (x[2] << 32) | x[3]
            else:
                u = int(word[r]) % (1 << 64)                   # exact: no float on the way
            i[r] = bisect.bisect_right(C, (u * total) >> 64)
    states, pol, val, slot, k = RR.batch(mover, opponent, policy, value, start, live, nb, seed,
                                         step, random_sym, i, sym, board_size)
    prob = np.zeros(nb, np.float32)
    for r in range(nb):
        if slot[r] >= 0 and total:
            qi = C[i[r]] - (C[i[r] - 1] if i[r] else 0)
            prob[r] = np.float32(np.float64(qi) / np.float64(total))
    return states, pol, val, slot, k, prob


def cdf_builder(weight, start, live, tile_log2, out):
    """ReplayBuffer's `cdf_builder` on CPU tensors: the contract words into `out` (int64)."""
    import torch
    words = cdf(weight.numpy(), start, live)
    out[:len(words)] = torch.from_numpy(words.view(np.int64))
    return out


def weighted_batcher(mover, opponent, policy, value, table, start, live, nb, seed, step,
                     random_sym, idx, sym, word, board_size):
    """ReplayBuffer's `weighted_batcher` on CPU tensors, by batch() above."""
    import torch
    out = batch(mover.numpy(), opponent.numpy(), policy.numpy(), value.numpy(), table.numpy(),
                start, live, nb, seed, step, random_sym, None if idx is None else idx.numpy(),
                None if sym is None else sym.numpy(),
                None if word is None else word.numpy().view(np.uint64), board_size)
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in out)
