"""The replay buffer without a GPU: ReplayBuffer on CPU tensors with the NumPy batcher
(tests/replay_ref.py) - append without and with wrap, eviction by capacity and by window, the
ledger, logical order - records_to_training(compact=True) with the oracle's `canonical`, the
reference draw's range, and rvz_replay_batch's argument checks (they run before any HIP call)."""
import numpy as np
import pytest
import torch

import merge_ref as M
import replay_ref as RR
import symmetry_ref as S
from test_pipeline_cpu import synthetic_records
from test_solve_cpu import _oracle_canonical, _train

EINVAL = -22


def _rows(bs, lo, hi):
    """Rows lo .. hi-1 of the shared set as append()'s four CPU tensors; row j carries value
    j / 1000, so a sampled value names the row it came from."""
    mover, opponent, policy, _ = RR.ring(bs, hi - lo, lo)
    value = (np.arange(lo, hi) / 1000).astype(np.float32)
    return (torch.from_numpy(mover.view(np.int64)), torch.from_numpy(opponent.view(np.int64)),
            torch.from_numpy(policy), torch.from_numpy(value))


def _buffer(capacity, bs=8, window=0):
    import rvz
    return rvz.ReplayBuffer(capacity, bs, "cpu", window_iterations=window, batcher=RR.batcher)


def _held(buf):
    """The source rows the buffer holds, oldest first, read through sample()."""
    n = len(buf)
    out = buf.sample(n, 0, 0, idx=torch.arange(n), sym=torch.zeros(n, dtype=torch.int32))
    return [int(round(float(v) * 1000)) for v in out[2].reshape(-1)], out


# ---------------------------------------------------------------- the ring
@pytest.mark.parametrize("bs", [8, 6])
def test_append_evicts_by_capacity(bs):
    """Capacity 7, appends of 3, 3, 3: the third wraps and overwrites the two oldest rows."""
    buf = _buffer(7, bs)
    assert len(buf) == 0 and buf.start == 0 and buf.rows_by_iteration() == []
    buf.append(*_rows(bs, 0, 3), 0)
    assert len(buf) == 3 and buf.start == 0 and buf.rows_by_iteration() == [(0, 3)]
    assert _held(buf)[0] == [0, 1, 2]
    buf.append(*_rows(bs, 3, 6), 1)
    assert len(buf) == 6 and buf.start == 0 and buf.rows_by_iteration() == [(0, 3), (1, 3)]
    assert _held(buf)[0] == [0, 1, 2, 3, 4, 5]
    buf.append(*_rows(bs, 6, 9), 2)                           # slots 6, 0, 1
    assert len(buf) == 7 and buf.start == 2
    assert buf.rows_by_iteration() == [(0, 1), (1, 3), (2, 3)]
    held, out = _held(buf)
    assert held == [2, 3, 4, 5, 6, 7, 8]                      # logical order, oldest first
    assert out[3].tolist() == [2, 3, 4, 5, 6, 0, 1]           # the slots they sit in
    # the rows are the reference rows of those positions, untransformed
    b, w, s = S.positions(bs)
    assert np.array_equal(out[0].numpy(), S.canonical(b[held], w[held], s[held], bs))
    assert np.array_equal(out[1].numpy(), S.policies(bs)[held])
    buf.append(*_rows(bs, 9, 16), 2)                          # a whole ring of iteration 2
    assert len(buf) == 7 and buf.start == 2 and buf.rows_by_iteration() == [(2, 7)]
    assert _held(buf)[0] == [9, 10, 11, 12, 13, 14, 15]
    buf.append(*_rows(bs, 16, 16), 3)                         # nothing
    assert len(buf) == 7 and buf.rows_by_iteration() == [(2, 7)]


def test_append_evicts_by_window():
    buf = _buffer(16, window=2)
    buf.append(*_rows(8, 0, 4), 0)
    buf.append(*_rows(8, 4, 9), 1)
    assert len(buf) == 9 and buf.start == 0 and buf.rows_by_iteration() == [(0, 4), (1, 5)]
    buf.append(*_rows(8, 9, 12), 2)                           # iteration 0 leaves the window
    assert len(buf) == 8 and buf.start == 4 and buf.rows_by_iteration() == [(1, 5), (2, 3)]
    assert _held(buf)[0] == list(range(4, 12))
    buf.append(*_rows(8, 12, 18), 3)                          # wraps: slots 12 .. 15, 0, 1
    assert len(buf) == 9 and buf.start == 9 and buf.rows_by_iteration() == [(2, 3), (3, 6)]
    held, out = _held(buf)
    assert held == list(range(9, 18))
    assert out[3].tolist() == [9, 10, 11, 12, 13, 14, 15, 0, 1]
    buf.append(*_rows(8, 18, 19), 7)                          # a gap: everything older leaves
    assert len(buf) == 1 and buf.start == 2 and buf.rows_by_iteration() == [(7, 1)]
    assert _held(buf)[0] == [18]
    # capacity and window together: the window drops what the overwrite left
    both = _buffer(7, window=2)
    for it, (lo, hi) in enumerate(((0, 3), (3, 6), (6, 9))):
        both.append(*_rows(8, lo, hi), it)
    assert both.rows_by_iteration() == [(1, 3), (2, 3)] and both.start == 3 and len(both) == 6
    assert _held(both)[0] == [3, 4, 5, 6, 7, 8]


def test_buffer_errors():
    import rvz
    buf = _buffer(7)
    with pytest.raises(ValueError):
        buf.sample(4, 0, 0)                                   # empty
    with pytest.raises(ValueError):
        buf.append(*_rows(8, 0, 8), 0)                        # more rows than the ring
    assert len(buf) == 0 and buf.rows_by_iteration() == []
    buf.append(*_rows(8, 0, 3), 5)
    with pytest.raises(ValueError):
        buf.append(*_rows(8, 3, 4), 4)                        # iterations go forward
    m, o, p, v = _rows(8, 3, 5)
    for bad in ((m[:1], o, p, v), (m, o, p[:, :64], v), (m.to(torch.int32), o, p, v),
                (m, o, p.double(), v), (m, o, p, v.reshape(1, 2))):
        with pytest.raises(ValueError):
            buf.append(*bad, 5)
    buf.append(m, o, p, v.reshape(2, 1), 5)                   # value [n, 1] is fine
    assert len(buf) == 5 and buf.rows_by_iteration() == [(5, 5)]
    for kw in (dict(capacity=0), dict(capacity=7, board_size=7), dict(capacity=2 ** 31),
               dict(capacity=7, window_iterations=-1), dict(capacity=7.0)):
        with pytest.raises(ValueError):
            rvz.ReplayBuffer(device="cpu", **kw)


def test_sample_is_the_reference_draw():
    """Without idx / sym the buffer's batch is the reference's for (start, live, seed, step)."""
    buf = _buffer(7)
    for it, (lo, hi) in enumerate(((0, 3), (3, 6), (6, 9))):
        buf.append(*_rows(8, lo, hi), it)
    held = _held(buf)[0]
    states, policy, value, slot, sym = buf.sample(64, 11, 3)
    idx, k = RR.draws(11, 3, 64, 7)
    assert sym.tolist() == k.tolist() and len(set(k.tolist())) == 8
    assert slot.tolist() == [(2 + i) % 7 for i in idx]
    assert [int(round(float(v) * 1000)) for v in value.reshape(-1)] == [held[i] for i in idx]
    assert value.shape == (64, 1) and states.shape == (64, 3, 8, 8) and policy.shape == (64, 65)
    off = buf.sample(64, 11, 3, symmetries=False)
    assert off[3].tolist() == slot.tolist() and not off[4].any()
    assert not torch.equal(buf.sample(64, 11, 4)[3], slot)


# ---------------------------------------------------------------- the reference draw
def test_reference_draw():
    """4,096 rows with live = 5 hit only [0, 5), every one of them, under all eight symmetries."""
    idx, sym = RR.draws(3, 9, 4096, 5)
    assert idx.min() == 0 and idx.max() == 4 and set(idx.tolist()) == set(range(5))
    assert set(sym.tolist()) == set(range(8))
    assert not RR.draws(3, 9, 4096, 5, random_sym=False)[1].any()
    assert not RR.draws(3, 9, 64, 1)[0].any()
    # a function of (seed, step, r): a prefix of a longer batch, and seeds / steps taken mod 2^64
    assert np.array_equal(RR.draws(3, 9, 64, 5)[0], idx[:64])
    assert RR.draw(2 ** 64 + 3, 9, 17, 5) == RR.draw(3, 2 ** 64 + 9, 17, 5) == (idx[17], sym[17])
    assert not np.array_equal(RR.draws(3, 10, 4096, 5)[0], idx)
    assert not np.array_equal(RR.draws(4, 9, 4096, 5)[0], idx)
    assert not np.array_equal(RR.draws(3 + 2 ** 32, 9, 4096, 5)[0], idx)      # the key's high word
    assert not np.array_equal(RR.draws(3, 9 + 2 ** 32, 4096, 5)[0], idx)      # the counter's
    # the block itself: the known-answer vector of the published algorithm
    assert RR.philox4x32_10((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e,
                                                       0x03707344)) == \
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


def test_reference_bad_rows():
    mover, opponent, policy, value = RR.ring(8, 7)
    st, pol, val, slot, sym = RR.batch(mover, opponent, policy, value, 5, 4, 5, 0, 0,
                                       idx=[0, -1, 4, 3, 1], sym=[1, 2, 3, 8, 7])
    assert slot.tolist() == [5, -1, -1, 1, 6] and sym.tolist() == [1, -1, -1, -1, 7]
    for r in (1, 2, 3):
        assert not st[r].any() and not pol[r].any() and val[r, 0] == 0
    assert st[0].any() and val[4, 0] == value[6]


# ---------------------------------------------------------------- records_to_training
def test_compact_rows_are_the_default_rows():
    rec, _ = synthetic_records(G=6, seed=3)
    calls = []

    def canonical(*a):
        calls.append(a)
        return _oracle_canonical(*a)

    from rvz.trainer import records_to_training
    args = [rec[k] for k in ("rec_black", "rec_white", "rec_side", "rec_idx", "rec_p",
                             "final_status")]
    base = _train(rec, 8)
    off = records_to_training(*args, 8, canonical=canonical, compact=False)
    assert len(calls) == 1 and list(off) == list(base) == ["states", "policy_targets",
                                                           "value_targets"]
    for k in base:
        assert off[k].dtype == base[k].dtype and off[k].shape == base[k].shape
        assert off[k].numpy().tobytes() == base[k].numpy().tobytes(), k
    out = records_to_training(*args, 8, canonical=canonical, compact=True)
    assert len(calls) == 1                                    # canonical is not called
    assert list(out) == ["mover", "opponent", "policy_targets", "value_targets"]
    n = base["states"].shape[0]
    assert out["mover"].dtype == out["opponent"].dtype == torch.int64
    assert out["mover"].shape == out["opponent"].shape == (n,)
    side1 = torch.stack([torch.ones(n, dtype=torch.int32)] * 4, dim=1)
    assert torch.equal(_oracle_canonical(out["mover"], out["opponent"], side1, 8), base["states"])
    for k in ("policy_targets", "value_targets"):
        assert out[k].dtype == base[k].dtype
        assert out[k].numpy().tobytes() == base[k].numpy().tobytes(), k
    sides = rec["rec_side"].t().reshape(-1)[(rec["rec_idx"] >= 0).t().reshape(-1)]
    assert set(sides.tolist()) == {1, 2}                      # both colours move in this set
    for bad in ("all", "random"):
        with pytest.raises(ValueError):
            _train(rec, 8, compact=True, symmetries=bad, augment=S.augment)


def test_compact_rows_after_exact_targets_and_merging():
    import solve_moves_ref as V
    import solve_ref as R
    from test_solve_moves_cpu import synthetic_records as exact_records
    _, rec = exact_records(8, 5)
    kw = dict(exact_policy=5, moves_solver=V.host_moves_solver, exact_endgame=5,
              solver=R.host_solver)
    full, out = _train(rec, 8, **kw), _train(rec, 8, compact=True, **kw)
    assert set(out) == (set(full) - {"states"}) | {"mover", "opponent"}
    for k in set(full) - {"states"}:
        assert torch.equal(out[k], full[k]), k
    assert not torch.equal(full["policy_targets"], _train(rec, 8)["policy_targets"])
    # merging: the bitboards of each group's first record
    rec, _ = synthetic_records(G=6, seed=3)
    plain = _train(rec, 8, compact=True)
    full = _train(rec, 8, merge_positions=True, merger=M.host_merger)
    out = _train(rec, 8, merge_positions=True, merger=M.host_merger, compact=True)
    assert list(out) == ["mover", "opponent", "policy_targets", "value_targets",
                         "position_counts", "merge_rows", "merge_input_rows"]
    for k in set(full) - {"states"}:
        assert torch.equal(out[k], full[k]), k
    keys = list(zip(plain["mover"].tolist(), plain["opponent"].tolist()))
    first = [keys.index(k) for k in dict.fromkeys(keys)]
    m = int(out["merge_rows"])
    assert m == len(first) < len(keys)
    assert torch.equal(out["mover"], plain["mover"][first])
    assert torch.equal(out["opponent"], plain["opponent"][first])
    side1 = torch.stack([torch.ones(m, dtype=torch.int32)] * 4, dim=1)
    assert torch.equal(_oracle_canonical(out["mover"], out["opponent"], side1, 8), full["states"])


def test_compact_rows_feed_the_buffer():
    """records_to_training(compact=True) -> append -> sample under the identity gives back the
    default call's rows."""
    rec, _ = synthetic_records(G=2, seed=1)
    base, out = _train(rec, 8), _train(rec, 8, compact=True)
    n = out["mover"].numel()
    buf = _buffer(n + 3)
    buf.append(out["mover"], out["opponent"], out["policy_targets"], out["value_targets"], 0)
    states, policy, value, slot, sym = buf.sample(n, 0, 0, idx=torch.arange(n),
                                                  sym=torch.zeros(n, dtype=torch.int64))
    assert torch.equal(states, base["states"]) and torch.equal(policy, base["policy_targets"])
    assert torch.equal(value, base["value_targets"]) and slot.tolist() == list(range(n))


# ---------------------------------------------------------------- the C-ABI's argument checks
def test_entry_point_refuses_bad_arguments_without_a_gpu():
    """RVZ_EINVAL before any HIP call (the pointers are never dereferenced)."""
    import rvz
    lib = rvz.load()
    p = 0x10000
    #       bs cap mover opp pol val start live nb idx   sym  rs seed step st pol val slot sym
    good = [8, 7, p, p, p, p, 5, 3, 4, None, None, 1, 0, 0, p, p, p, p, p, None]
    for bs in (8, 6):
        zero = [bs, 7] + [None] * 4 + [5, 3, 0, None, None, 1, 2 ** 64 - 1, 2 ** 64 - 1] + \
            [None] * 6
        assert lib.rvz_replay_batch(*zero) == 0               # nb = 0: nothing to do
    for k, v in ((0, 7), (0, 4), (1, 0), (1, -1), (7, 0), (7, 8), (7, -1), (6, -1), (6, 7),
                 (8, -1), (8, 2 ** 31 // 65 + 1), (14, p + 4), (14, p + 8)):
        args = list(good)
        args[k] = v
        assert lib.rvz_replay_batch(*args) == EINVAL, (k, v)
    args = list(good)
    args[0], args[8] = 6, 2 ** 31 // 37 + 1
    assert lib.rvz_replay_batch(*args) == EINVAL
    for k in (2, 3, 4, 5, 14, 15, 16, 17, 18):                # idx (9) and sym (10) may be null
        args = list(good)
        args[k] = None
        assert lib.rvz_replay_batch(*args) == EINVAL, k
    # bad arguments are refused at nb = 0 too
    for k, v in ((0, 7), (1, 0), (7, 0), (7, 8), (6, 7)):
        args = list(good)
        args[8], args[k] = 0, v
        assert lib.rvz_replay_batch(*args) == EINVAL, (k, v)
