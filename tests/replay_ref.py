"""Host reference of the replay buffer's minibatch draw (rvz_replay_batch, include/rvz.h), written
from the definition alone on Python integers and NumPy arrays; it shares no code with the product.

philox4x32_10(key, ctr)     the generator, restated from the paper (as tests/test_gpu_dirichlet.py)
draw(seed, step, r, live, random_sym)   output row r's (logical index, symmetry)
batch(...)                  rvz_replay_batch's five outputs, the rows themselves through
                            tests/symmetry_ref.training_rows
batcher(...)                the same on CPU tensors: ReplayBuffer's `batcher`
ring(bs, capacity, first)   a ring filled from the shared positions of tests/symmetry_ref.py
"""
import numpy as np

import symmetry_ref as S

M32 = 0xFFFFFFFF


def philox4x32_10(key, ctr):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
    SC'11): 10 rounds of two 32x32 -> 64 multiplies, the key bumped by the Weyl constants between
    rounds."""
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    k0, k1 = key
    c0, c1, c2, c3 = ctr
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & M32, (k1 + W1) & M32
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
    return c0, c1, c2, c3


def draw(seed: int, step: int, r: int, live: int, random_sym: bool = True):
    """(i, k) of output row r: i = mulhi(x.0, live), k = x.1 & 7 (0 without random_sym), x the
    block of key (seed lo, seed hi) and counter (r, step lo, step hi, 0); seed and step mod 2^64."""
    seed, step = seed % (1 << 64), step % (1 << 64)
    x = philox4x32_10((seed & M32, seed >> 32), (r, step & M32, step >> 32, 0))
    return (x[0] * live) >> 32, (x[1] & 7) if random_sym else 0


def draws(seed, step, nb, live, random_sym=True):
    """draw() for rows 0 .. nb-1: (idx int32 [nb], sym int32 [nb])."""
    got = [draw(seed, step, r, live, random_sym) for r in range(nb)]
    return (np.array([g[0] for g in got], np.int32).reshape(nb),
            np.array([g[1] for g in got], np.int32).reshape(nb))


def batch(mover, opponent, policy, value, start, live, nb, seed, step, random_sym=True,
          idx=None, sym=None, board_size=8):
    """(states f32 [nb, 3, S, S], policy f32 [nb, S*S+1], value f32 [nb, 1], slot i32 [nb],
    sym i32 [nb]) of the ring (mover / opponent uint64 [capacity], policy, value)."""
    mover = np.asarray(mover).view(np.uint64).reshape(-1)
    opponent = np.asarray(opponent).view(np.uint64).reshape(-1)
    cap, bs = len(mover), board_size
    policy = np.asarray(policy, np.float32).reshape(cap, bs * bs + 1)
    value = np.asarray(value, np.float32).reshape(cap)
    assert 1 <= live <= cap and 0 <= start < cap
    di, dk = draws(seed, step, nb, live, random_sym)
    i = di if idx is None else np.asarray(idx).astype(np.int64).reshape(nb)
    k = dk if sym is None else np.asarray(sym).astype(np.int64).reshape(nb)
    inside = (i >= 0) & (i < live)
    ok = inside & (k >= 0) & (k < 8)
    slot = np.where(inside, (start + np.where(inside, i, 0)) % cap, -1).astype(np.int32)
    states = np.zeros((nb, 3, bs, bs), np.float32)
    pol = np.zeros((nb, bs * bs + 1), np.float32)
    val = np.zeros((nb, 1), np.float32)
    used = np.unique(slot[ok])
    if len(used):          # every image of every slot that is read, once
        st8, pol8, _ = S.training_rows(mover[used], opponent[used], np.ones(len(used), np.int32),
                                       policy[used], None, bs, all_images=True)
        at = 8 * np.searchsorted(used, slot[ok]) + k[ok]
        states[ok], pol[ok], val[ok, 0] = st8[at], pol8[at], value[slot[ok]]
    return states, pol, val, slot, np.where(ok, k, -1).astype(np.int32)


def batcher(mover, opponent, policy, value, start, live, nb, seed, step, random_sym, idx, sym,
            board_size):
    """ReplayBuffer's `batcher` on CPU tensors, by batch() above."""
    import torch
    out = batch(mover.numpy(), opponent.numpy(), policy.numpy(), value.numpy(), start, live, nb,
                seed, step, random_sym, None if idx is None else idx.numpy(),
                None if sym is None else sym.numpy(), board_size)
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in out)


def ring(bs: int, capacity: int, first: int = 0):
    """(mover uint64, opponent uint64, policy f32, value f32) [capacity]: slot s holds row
    first + s of the shared set (symmetry_ref.positions / policies) as seen by its mover, with a
    value in [-1, 1] that tells the slots apart."""
    b, w, s = S.positions(bs)
    rows = (first + np.arange(capacity)) % len(b)
    mover, opponent = S.mover_opp(b[rows], w[rows], s[rows])
    value = ((rows * 37 % 201 - 100) / 100).astype(np.float32)
    return mover, opponent, S.policies(bs)[rows].copy(), value
