"""Host reference of prioritized replay's two calls (rvz_replay_is_weight and rvz_replay_priority,
include/rvz.h), written from the contract alone on NumPy float64 and 60-digit decimal arithmetic;
it shares no code with the product.

pow_cr(x, e)                 the correctly rounded x ** e for x >= 0, as rvz_pow is pinned in
                             tests/test_oracle_search.py: 60-digit exp(e ln x), rounded once
is_weight(prob, slot, beta)  (out_weight f32 [nb], out_min_prob f32)
priority(weight, slot, rows, ...)   (weight', out_priority f32 [nb], out_state i32 [nb],
                             max_priority'), the duplicate rule as the sequential loop
is_weighter / priority_updater      the same on CPU tensors: ReplayBuffer's injection points
mixed_rows(rng, nb, capacity, ...)  seeded test inputs: random loss rows mixed with every invalid
                             kind, with duplicates
"""
import math
from decimal import Decimal, getcontext
from functools import lru_cache

import numpy as np


@lru_cache(maxsize=None)
def pow_cr(x, e):
    x, e = float(x), float(e)
    assert x >= 0.0 and math.isfinite(x) and math.isfinite(e)
    if e == 0.0 or x == 1.0:
        return 1.0
    if x == 0.0:
        return 0.0 if e > 0.0 else math.inf
    getcontext().prec = 60
    return float((Decimal(x).ln() * Decimal(e)).exp())


def is_weight(prob, slot, beta):
    prob = np.asarray(prob, np.float32).reshape(-1)
    slot = np.asarray(slot).astype(np.int64).reshape(-1)
    assert prob.shape == slot.shape and 0.0 <= beta <= 1.0
    valid = (slot >= 0) & np.isfinite(prob) & (prob > 0)
    out = np.zeros(len(prob), np.float32)
    if not valid.any():
        return out, np.float32(0)
    pmin = prob[valid].min()
    for r in np.flatnonzero(valid):
        ratio = np.float64(pmin) / np.float64(prob[r])                  # one rounded division
        out[r] = np.float32(pow_cr(float(ratio), beta))
    return out, np.float32(pmin)


def row_priority(capacity, slot, row, policy_coef, value_coef, subtract_entropy, alpha, floor,
                 cap):
    """p_r as np.float32, or None for an invalid row."""
    Lp, Lv, H = (np.float64(x) for x in row)
    with np.errstate(all="ignore"):
        d = Lp - H
        k = (d if d > 0.0 else np.float64(0.0)) if subtract_entropy else Lp
        e = np.float64(policy_coef) * k + np.float64(value_coef) * Lv   # each op rounded
    if not (0 <= slot < capacity and np.isfinite(Lp) and np.isfinite(Lv) and np.isfinite(H) and
            Lp >= 0.0 and Lv >= 0.0 and np.isfinite(e)):
        return None
    return np.float32(min(float(cap), max(float(floor), pow_cr(float(e), alpha))))


def priority(weight, slot, rows, policy_coef=1.0, value_coef=1.0, subtract_entropy=True,
             alpha=0.6, floor=2.0 ** -8, cap=2.0 ** 8, max_priority=None):
    """Returns (the new weight array (a copy), out_priority, out_state, the new max_priority or
    None)."""
    weight = np.array(weight, np.float32).reshape(-1)
    slot = np.asarray(slot).astype(np.int64).reshape(-1)
    rows = np.asarray(rows, np.float64).reshape(-1, 3)
    nb, capacity = len(slot), len(weight)
    assert len(rows) == nb and 2.0 ** -16 <= floor <= cap <= 65536.0 and 0.0 <= alpha <= 1.0
    pri = np.zeros(nb, np.float32)
    state = np.full(nb, -1, np.int32)
    last = {}
    top = None if max_priority is None else np.float32(max_priority)
    for r in range(nb):                                                 # the sequential loop
        p = row_priority(capacity, int(slot[r]), rows[r], policy_coef, value_coef,
                         subtract_entropy, alpha, floor, cap)
        if p is None:
            continue
        pri[r] = p
        weight[slot[r]] = p
        if int(slot[r]) in last:
            state[last[int(slot[r])]] = 0
        last[int(slot[r])] = r
        state[r] = 1
        if top is not None and p > top:
            top = p
    return weight, pri, state, top


# ------------------------------------------------------------------ ReplayBuffer's injection points
def is_weighter(prob, slot, beta):
    import torch
    from rvz.records import check_is_weight_args
    check_is_weight_args(prob, slot, beta)
    return torch.from_numpy(is_weight(prob.numpy(), slot.numpy(), beta)[0])


def priority_updater(weight, slot, rows, policy_coef, value_coef, subtract_entropy, alpha, floor,
                     cap, max_priority):
    import torch
    from rvz.records import check_priority_args
    check_priority_args(weight, slot, rows, policy_coef, value_coef, subtract_entropy, alpha,
                        floor, cap, max_priority)
    w, pri, state, top = priority(weight.numpy(), slot.numpy(), rows.detach().numpy(),
                                  policy_coef, value_coef, subtract_entropy, alpha, floor, cap,
                                  None if max_priority is None else max_priority.item())
    weight.copy_(torch.from_numpy(w))
    if max_priority is not None:
        max_priority.fill_(float(top))
    return torch.from_numpy(pri), torch.from_numpy(state)


# ------------------------------------------------------------------ seeded inputs
INVALID_ROWS = ((float("nan"), 0.5, 0.1), (1.0, float("inf"), 0.1), (1.0, 0.5, float("nan")),
                (-0.25, 0.5, 0.1), (1.0, -1e-9, 0.1), (float("-inf"), 0.0, 0.0))


def mixed_rows(rng, nb, capacity, slots=None, weird=True):
    """(slot int32 [nb], rows float64 [nb, 3]): Lp in [0, 6), Lv in [0, 4), H in [0, Lp * 1.1]
    (so some KL clamp at 0), a few exact zeros and huge values, and with `weird` about one row in
    eight made invalid: slot -1, slot >= capacity, or one of INVALID_ROWS. slots: the slots to
    use (default: uniform over the ring)."""
    slot = (rng.integers(0, capacity, nb) if slots is None else np.asarray(slots)).astype(np.int32)
    Lp = rng.uniform(0, 6, nb)
    rows = np.stack([Lp, rng.uniform(0, 4, nb) ** 2 / 4, Lp * rng.uniform(0, 1.1, nb)], 1)
    for r in range(0, nb, 11):
        rows[r] = ((0.0, 0.0, 0.0), (1e300, 1e300, 0.0), (3e-7, 0.0, 2e-7), (700.0, 4.0, 0.0))[
            (r // 11) % 4]
    if weird:
        for r in np.flatnonzero(rng.integers(0, 8, nb) == 0):
            kind = int(rng.integers(0, 3))
            if kind == 0:
                slot[r] = -1
            elif kind == 1:
                slot[r] = capacity + int(rng.integers(0, 3))
            else:
                rows[r] = INVALID_ROWS[int(rng.integers(0, len(INVALID_ROWS)))]
    return slot, rows


def mixed_probs(rng, nb, slot):
    """prob float32 [nb]: random probabilities, a few zero / NaN / inf / negative / subnormal."""
    prob = (rng.uniform(1e-6, 1.0, nb) ** 3).astype(np.float32)
    for r in np.flatnonzero(rng.integers(0, 8, nb) == 0):
        prob[r] = (0.0, np.nan, np.inf, -0.5, 1e-42)[int(rng.integers(0, 5))]
    return prob
