"""Prioritized replay without a GPU: the reference (tests/replay_priority_ref.py) on its own
properties, ReplayBuffer(prioritized=True) on CPU tensors with the reference's callables, the
argument rules of the C-ABI, the wrappers, the buffer, the trainer and SelfPlayTrainer (all checked
before any HIP call), and DDPTrainer.train_replay on the CPU with the NumPy loss and a tiny net."""
import math

import numpy as np
import pytest
import torch

import loss_ref as LR
import replay_priority_ref as P
import replay_weighted_ref as W
from test_replay_cpu import _rows

EINVAL = -22
NAN, INF = float("nan"), float("inf")


def _buffer(capacity, bs=8, **kw):
    import rvz
    kw.setdefault("cdf_builder", W.cdf_builder)
    return rvz.ReplayBuffer(capacity, bs, "cpu", prioritized=True,
                            weighted_batcher=W.weighted_batcher,
                            priority_updater=P.priority_updater, is_weighter=P.is_weighter, **kw)


def _f64(*rows):
    return torch.tensor(rows, dtype=torch.float64).reshape(-1, 3)


def _i32(*x):
    return torch.tensor(x, dtype=torch.int32)


# ---------------------------------------------------------------- the reference itself
def test_pow_is_the_pinned_power():
    assert P.pow_cr(0.3, 0.0) == 1.0 and P.pow_cr(1.0, 0.7) == 1.0 and P.pow_cr(0.0, 0.6) == 0.0
    assert P.pow_cr(4.0, 0.5) == 2.0 and P.pow_cr(2.0, 1.0) == 2.0
    rng = np.random.default_rng(0)
    x, e = rng.uniform(0, 8, 400), rng.uniform(0, 1, 400)
    got = np.array([P.pow_cr(a, b) for a, b in zip(x, e)])
    lib = np.array([math.pow(a, b) for a, b in zip(x, e)])
    assert np.all(np.abs(got - lib) <= np.spacing(lib))         # glibc is within an ulp of it


def test_priority_last_row_wins_and_other_slots_keep_their_bytes():
    weight = np.array([NAN, 7.0, -3.0, 0.5, 1e-30, 9.0], np.float32)
    #          r:  0  1  2  3   4  5  6
    slot = [4, 1, 4, 1, -1, 6, 4]
    rows = [(1.0, 0.0, 0.0), (4.0, 0.0, 0.0), (9.0, 0.0, 0.0), (NAN, 0.0, 0.0), (1.0, 1.0, 0.0),
            (1.0, 1.0, 0.0), (16.0, 0.0, 0.0)]
    w, pri, state, top = P.priority(weight, slot, rows, subtract_entropy=False, alpha=0.5,
                                    max_priority=2.5)
    assert state.tolist() == [0, 1, 0, -1, -1, -1, 1]           # row 3 is invalid: row 1 stands
    assert pri.tolist() == [1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 4.0]
    assert w[4] == 4.0 and w[1] == 2.0
    keep = [0, 2, 3, 5]
    assert np.array_equal(w[keep].view(np.int32), weight[keep].view(np.int32))   # NaN bits too
    assert top == 4.0                                           # over every valid row
    assert P.priority(weight, slot, rows, subtract_entropy=False, alpha=0.5,
                      max_priority=5.0)[3] == 5.0               # monotone
    # superseded rows count for the maximum: row 0's 8 loses its slot to row 1 and still counts
    _, _, st, top = P.priority(np.ones(2, np.float32), [0, 0], [(64.0, 0, 0), (1.0, 0, 0)],
                               subtract_entropy=False, alpha=0.5, max_priority=1.0)
    assert st.tolist() == [0, 1] and top == 8.0


def test_priority_alpha_floor_cap_and_kl():
    rng = np.random.default_rng(3)
    slot, rows = P.mixed_rows(rng, 96, 200, weird=False)
    ones = P.priority(np.zeros(200, np.float32), slot, rows, alpha=0.0)
    assert set(ones[1].tolist()) == {1.0} and set(ones[2].tolist()) <= {0, 1}
    _, pri, _, _ = P.priority(np.zeros(200, np.float32), slot, rows, alpha=1.0, floor=0.25, cap=2.0)
    assert pri.min() == 0.25 and pri.max() == 2.0 and ((pri > 0.25) & (pri < 2.0)).any()
    # KL: Lp - H, clamped at 0 where rounding (or a caller) made it negative
    def one(row, **kw):
        return float(P.priority(np.zeros(1, np.float32), [0], [row], alpha=1.0, floor=2.0 ** -16,
                                cap=65536.0, **kw)[1][0])
    assert one((3.0, 0.5, 1.0)) == 2.5 and one((3.0, 0.5, 1.0), subtract_entropy=False) == 3.5
    assert one((1.0, 0.5, 1.0 + 1e-12)) == 0.5 and one((1.0, 0.0, 2.0)) == 2.0 ** -16
    assert one((3.0, 0.5, 1.0), policy_coef=2.0, value_coef=4.0) == 6.0
    assert one((0.0, 0.0, 0.0)) == 2.0 ** -16                   # e = 0: the floor
    # the floor keeps a written row drawable: its fixed-point weight is above 0
    assert W.q(np.float32(2.0 ** -16)) == 1


def test_priority_invalid_rows():
    w0 = np.full(4, 0.75, np.float32)
    for slot, row in ((-1, (1, 1, 0)), (4, (1, 1, 0)), (7, (1, 1, 0)), (0, (NAN, 1, 0)),
                      (0, (1, NAN, 0)), (0, (1, 1, NAN)), (0, (INF, 1, 0)), (0, (1, INF, 0)),
                      (0, (1, 1, -INF)), (0, (-1e-300, 1, 0)), (0, (1, -1e-300, 0))):
        w, pri, state, top = P.priority(w0, [slot], [row], max_priority=1.0)
        assert state.tolist() == [-1] and pri.tolist() == [0.0] and top == 1.0, (slot, row)
        assert np.array_equal(w, w0)
    # e overflows although every entry is finite
    assert P.priority(w0, [0], [(1e300, 0, 0)], policy_coef=1e10)[2].tolist() == [-1]
    assert P.priority(w0, [0], [(1e300, 0, 0)], policy_coef=1e8)[2].tolist() == [1]
    # a negative H is a valid row (only Lp and Lv are signed losses)
    assert P.priority(w0, [3], [(1.0, 0.0, -1.0)], alpha=1.0)[1].tolist() == [2.0]


def test_is_weight_properties():
    rng = np.random.default_rng(5)
    slot = rng.integers(0, 50, 300).astype(np.int32)
    slot[::17] = -1
    prob = P.mixed_probs(rng, 300, slot)
    valid = (slot >= 0) & np.isfinite(prob) & (prob > 0)
    assert valid.sum() > 200 and (~valid).sum() > 30
    for beta in (0.4, 1.0):
        w, pmin = P.is_weight(prob, slot, beta)
        assert w.dtype == np.float32 and pmin == prob[valid].min()
        assert np.all(w[valid] > 0) and np.all(w[valid] <= 1) and not w[~valid].any()
        assert set(w[valid & (prob == pmin)].tolist()) == {1.0}  # the rarest row weighs 1
        order = np.argsort(prob[valid], kind="stable")
        assert np.all(np.diff(w[valid][order]) <= 0)             # rarer rows weigh more
    w, _ = P.is_weight(prob, slot, 0.0)
    assert set(w[valid].tolist()) == {1.0} and not w[~valid].any()
    # beta = 1 is the plain ratio, rounded once to float32
    w, pmin = P.is_weight(np.array([0.5, 0.125, 0.25], np.float32), [0, 1, 2], 1.0)
    assert w.tolist() == [0.25, 1.0, 0.5] and pmin == 0.125
    # a batch with no valid row
    w, pmin = P.is_weight(np.array([0.0, NAN, 0.5, INF], np.float32), [0, 0, -1, 3], 0.4)
    assert not w.any() and pmin == 0.0
    w, pmin = P.is_weight(np.zeros(0, np.float32), np.zeros(0, np.int32), 0.4)
    assert len(w) == 0 and pmin == 0.0


def test_seeded_inputs_show_every_state():
    """What the GPU tests rely on: their seeded inputs carry winners, superseded rows and invalid
    rows alike, at every shape."""
    for nb, cap in ((64, 8), (65, 300), (4097, 8), (4097, 1 << 20)):
        slot, rows = P.mixed_rows(np.random.default_rng(nb), nb, cap)
        if cap == 1 << 20:
            slot = np.where(slot < 0, slot, np.where(slot >= cap, slot, np.arange(nb))).astype(
                np.int32)
            slot[nb - 1] = slot[1] = 5                          # rows 1 and nb - 1 name one slot
            rows[1] = rows[nb - 1] = (1.0, 1.0, 0.5)
        state = P.priority(np.ones(cap, np.float32), slot, rows)[2]
        assert set(state.tolist()) == {-1, 0, 1}, (nb, cap)


# ---------------------------------------------------------------- ReplayBuffer(prioritized=True)
def _held_weights(buf):
    at = (buf.start + torch.arange(len(buf))) % buf.capacity
    return buf.weight[at].tolist()


def test_new_rows_enter_at_the_running_maximum():
    buf = _buffer(8, priority_alpha=1.0, subtract_entropy=False)
    assert buf.weighted and buf.prioritized and buf.max_priority() == 1.0
    buf.append(*_rows(8, 0, 3), 0)
    assert _held_weights(buf) == [1.0, 1.0, 1.0]
    pri, state = buf.update_priorities(_i32(1, 1, -1), _f64((9.0, 0, 0), (2.0, 1.0, 0), (5, 5, 0)))
    assert pri.tolist() == [9.0, 3.0, 0.0] and state.tolist() == [0, 1, -1]
    assert buf.max_priority() == 9.0 and _held_weights(buf) == [1.0, 3.0, 1.0]
    buf.append(*_rows(8, 3, 5), 0)                              # at the maximum: 9, not 1
    buf.append(*_rows(8, 5, 6), 0, weight=torch.tensor([0.5]))  # an explicit weight still wins
    assert _held_weights(buf) == [1.0, 3.0, 1.0, 9.0, 9.0, 0.5]
    buf.update_priorities(_i32(0), _f64((0.25, 0, 0)))
    assert buf.max_priority() == 9.0                            # monotone
    buf.append(*_rows(8, 6, 9), 0)                              # wraps over row 0
    assert buf.start == 1 and buf.weight.tolist() == [9.0, 3.0, 1.0, 9.0, 9.0, 0.5, 9.0, 9.0]


def test_update_marks_the_table_stale_and_the_next_draw_sees_it():
    calls = []

    def builder(*a):
        calls.append(a[1:3])
        return W.cdf_builder(*a)
    buf = _buffer(8, cdf_builder=builder)
    buf.append(*_rows(8, 0, 6), 0)
    out = buf.sample(64, 1, 0, with_prob=True)
    assert len(calls) == 1 and set(out[5].tolist()) == {float(np.float32(1 / 6))}
    rows = torch.from_numpy(np.random.default_rng(0).uniform(0, 3, (64, 3)))
    before = buf.weight.numpy().copy()
    pri, state = buf.update_priorities(out[3], rows, 1.0, 0.5)
    want = P.priority(before, out[3].numpy(), rows.numpy(), 1.0, 0.5)
    assert np.array_equal(buf.weight.numpy(), want[0]) and np.array_equal(pri.numpy(), want[1])
    assert np.array_equal(state.numpy(), want[2]) and set(state.tolist()) == {0, 1}
    assert len(calls) == 1 and buf._dirty                       # lazily
    idx = torch.arange(6, dtype=torch.int32)
    got = buf.sample(6, 1, 1, idx=idx, with_prob=True)
    assert len(calls) == 2
    q = [W.q(x) for x in buf.weight[:6].tolist()]
    assert got[5].tolist() == [float(np.float32(np.float64(x) / np.float64(sum(q)))) for x in q]
    assert buf.total_weight() == sum(q) / 65536
    w = buf.is_weights(got[5], got[3], 0.5)
    assert np.array_equal(w.numpy(), P.is_weight(got[5].numpy(), got[3].numpy(), 0.5)[0])
    assert float(w.max()) == 1.0 and int(w.argmax()) == int(got[5].argmin())


def test_recency_decay_leaves_the_maximum_alone():
    buf = _buffer(8, recency_decay=0.5, priority_alpha=1.0, subtract_entropy=False)
    buf.append(*_rows(8, 0, 2), 0)
    buf.update_priorities(_i32(0), _f64((4.0, 0, 0)))
    buf.append(*_rows(8, 2, 3), 1)
    assert _held_weights(buf) == [2.0, 0.5, 4.0] and buf.max_priority() == 4.0


def test_buffer_argument_rules():
    import rvz
    for kw in (dict(priority_alpha=-0.1), dict(priority_alpha=1.5), dict(priority_alpha=NAN),
               dict(priority_alpha="0.6"), dict(priority_alpha=True),
               dict(priority_floor=2.0 ** -17), dict(priority_floor=0.0),
               dict(priority_cap=65537.0), dict(priority_floor=2.0, priority_cap=1.0),
               dict(priority_floor=NAN), dict(priority_cap=INF), dict(subtract_entropy="yes")):
        with pytest.raises(ValueError):
            _buffer(8, **kw)
    _buffer(8, priority_floor=2.0 ** -16, priority_cap=65536.0, priority_alpha=0)
    for kw in (dict(priority_alpha=0.5), dict(priority_floor=0.5), dict(priority_cap=4.0),
               dict(subtract_entropy=False), dict(priority_updater=P.priority_updater),
               dict(is_weighter=P.is_weighter)):
        for weighted in (False, True):
            with pytest.raises(ValueError):                     # they need prioritized=True
                rvz.ReplayBuffer(8, 8, "cpu", weighted=weighted, **kw)
    plain = rvz.ReplayBuffer(8, 8, "cpu", weighted=True, weighted_batcher=W.weighted_batcher,
                             cdf_builder=W.cdf_builder)
    assert not plain.prioritized and not hasattr(plain, "_max_priority")
    plain.append(*_rows(8, 0, 2), 0)
    assert _held_weights(plain) == [1.0, 1.0]
    for call in (lambda: plain.update_priorities(_i32(0), _f64((1, 1, 0))),
                 lambda: plain.is_weights(torch.ones(1), _i32(0), 0.4), plain.max_priority):
        with pytest.raises(ValueError):
            call()
    buf = _buffer(8)
    buf.append(*_rows(8, 0, 2), 0)
    for call in (lambda: buf.update_priorities(_i32(0, 1), _f64((1, 1, 0))),
                 lambda: buf.update_priorities(_i32(0), _f64((1, 1, 0)).float()),
                 lambda: buf.update_priorities(torch.zeros(1), _f64((1, 1, 0))),
                 lambda: buf.update_priorities(_i32(0), _f64((1, 1, 0)), policy_coef=-1.0),
                 lambda: buf.update_priorities(_i32(0), _f64((1, 1, 0)), value_coef=INF),
                 lambda: buf.is_weights(torch.ones(2), _i32(0), 0.4),
                 lambda: buf.is_weights(torch.ones(1).double(), _i32(0), 0.4),
                 lambda: buf.is_weights(torch.ones(1), _i32(0), 1.5),
                 lambda: buf.is_weights(torch.ones(1), _i32(0), NAN)):
        with pytest.raises(rvz.RvzError):
            call()
    assert _held_weights(buf) == [1.0, 1.0]


def test_wrappers_refuse_bad_arguments_before_the_library():
    import rvz
    w, s, r = torch.ones(4), _i32(0, 1), _f64((1, 1, 0), (1, 1, 0))
    for call in (lambda: rvz.replay_priority(w.double(), s, r),
                 lambda: rvz.replay_priority(w.reshape(2, 2), s, r),
                 lambda: rvz.replay_priority(torch.ones(8)[::2], s, r),
                 lambda: rvz.replay_priority(torch.ones(0), s, r),
                 lambda: rvz.replay_priority(w, s, r.float()),
                 lambda: rvz.replay_priority(w, s, r.reshape(3, 2)),
                 lambda: rvz.replay_priority(w, s[:1], r),
                 lambda: rvz.replay_priority(w, s.float(), r),
                 lambda: rvz.replay_priority(w, s, r, policy_coef=NAN),
                 lambda: rvz.replay_priority(w, s, r, value_coef=-0.5),
                 lambda: rvz.replay_priority(w, s, r, subtract_entropy=None),
                 lambda: rvz.replay_priority(w, s, r, alpha=1.01),
                 lambda: rvz.replay_priority(w, s, r, floor=2.0 ** -17),
                 lambda: rvz.replay_priority(w, s, r, cap=2.0 ** 17),
                 lambda: rvz.replay_priority(w, s, r, floor=3.0, cap=2.0),
                 lambda: rvz.replay_priority(w, s, r, max_priority=torch.ones(2)),
                 lambda: rvz.replay_priority(w, s, r, max_priority=torch.ones(1).double()),
                 lambda: rvz.replay_priority(w, s, r, max_priority=1.0),
                 lambda: rvz.replay_is_weight(w, s, 0.4),
                 lambda: rvz.replay_is_weight(w[:2].double(), s, 0.4),
                 lambda: rvz.replay_is_weight(w[:2], s.float(), 0.4),
                 lambda: rvz.replay_is_weight(w[:2], s, -0.1),
                 lambda: rvz.replay_is_weight(w[:2], s, True),
                 lambda: rvz.replay_is_weight(w[:2], s, "0.4")):
        with pytest.raises(rvz.RvzError):
            call()
    if not torch.cuda.is_available():                           # well-formed, but no device
        with pytest.raises(rvz.RvzError):
            rvz.replay_priority(w, s, r)
        with pytest.raises(rvz.RvzError):
            rvz.replay_is_weight(w[:2], s, 0.4)
    # an empty batch launches nothing and needs no device
    pri, state = rvz.replay_priority(w, _i32(), torch.zeros(0, 3, dtype=torch.float64))
    assert pri.shape == (0,) and state.shape == (0,) and w.tolist() == [1, 1, 1, 1]
    out, pmin = rvz.replay_is_weight(torch.zeros(0), _i32(), 0.4, with_min=True)
    assert out.shape == (0,) and pmin.tolist() == [0.0]


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """RVZ_EINVAL before any HIP call (the pointers are never dereferenced)."""
    import rvz
    lib = rvz.load()
    p = 0x10000
    assert lib.rvz_replay_is_weight_scratch_size(0) == 16
    assert lib.rvz_replay_is_weight_scratch_size(2 ** 31 - 1) == 16
    assert lib.rvz_replay_is_weight_scratch_size(-1) < 0
    #       nb prob slot beta scratch out  min  stream
    good = [5, p, p, 0.4, p, p, None, None]
    for k, v in ((0, -1), (3, -0.01), (3, 1.01), (3, NAN), (3, INF), (1, None), (2, None),
                 (4, None), (5, None), (4, p + 8), (4, p + 4)):
        args = list(good)
        args[k] = v
        assert lib.rvz_replay_is_weight(*args) == EINVAL, (k, v)
    assert lib.rvz_replay_is_weight(0, None, None, 0.4, None, None, None, None) == 0
    for beta in (0.0, 1.0):
        assert lib.rvz_replay_is_weight(0, None, None, beta, None, None, None, None) == 0
    assert lib.rvz_replay_is_weight(0, None, None, 2.0, None, None, None, None) == EINVAL
    assert lib.rvz_replay_is_weight(-1, p, p, 0.4, p, p, None, None) == EINVAL

    sizes = [lib.rvz_replay_priority_scratch_size(n) for n in (0, 1, 32, 33, 64, 65, 4096, 4097,
                                                               2 ** 21, 2 ** 30)]
    assert sizes == sorted(sizes) and all(s % 16 == 0 and s > 0 for s in sizes)
    assert sizes[0] == 16 + 8 * 64 and sizes[4] == 16 + 4 * 64 + 8 * 128
    assert sizes[5] == 16 + 272 + 8 * 256                       # 65 rows: the table doubles
    assert lib.rvz_replay_priority_scratch_size(-1) < 0
    assert lib.rvz_replay_priority_scratch_size(2 ** 30 + 1) < 0
    #       0    1  2  3  4  5    6    7  8    9        10     11 12    13    14    15
    good = [100, p, 5, p, p, 1.0, 1.0, 1, 0.6, 2 ** -8, 2 ** 8, p, None, None, None, None]
    for k, v in ((0, 0), (0, -1), (2, -1), (2, 2 ** 30 + 1), (5, -1.0), (5, NAN), (5, INF),
                 (6, -1e-300), (6, NAN), (6, INF), (8, -0.1), (8, 1.1), (8, NAN),
                 (9, 2.0 ** -17), (9, 0.0), (9, NAN), (9, 2.0 ** 9), (10, 2.0 ** 17), (10, NAN),
                 (10, 2.0 ** -9), (1, None), (3, None), (4, None), (11, None), (11, p + 8),
                 (11, p + 4)):
        args = list(good)
        args[k] = v
        assert lib.rvz_replay_priority(*args) == EINVAL, (k, v)
    zero = [100, None, 0, None, None, 0.0, 0.0, 0, 0.0, 2.0 ** -16, 65536.0, None, None, None,
            None, None]
    assert lib.rvz_replay_priority(*zero) == 0                  # nb = 0: nothing to do
    for k, v in ((0, 0), (5, -1.0), (8, 2.0), (9, 2.0 ** -17), (10, 2.0 ** 17)):
        args = list(zero)                                       # refused at nb = 0 too
        args[k] = v
        assert lib.rvz_replay_priority(*args) == EINVAL, (k, v)


# ---------------------------------------------------------------- the trainer
def _model():
    import rvz
    torch.manual_seed(0)
    return rvz.AlphaZeroNetwork(8, 1, 16)


def _loss_fn():
    from rvz.loss import differentiable
    return differentiable(LR.as_kernel)


def _filled(buf, n=24):
    g = torch.Generator().manual_seed(1)
    mover, opponent, _, value = _rows(8, 0, n)
    policy = torch.rand(n, 65, generator=g) * (torch.rand(n, 65, generator=g) < 0.3)
    policy[:, 64] += 0.01
    policy = policy / policy.sum(1, keepdim=True)
    buf.append(mover, opponent, policy, (value * 40 - 0.5).clamp(-1, 1), 0)
    return buf


def test_loss_rows_option():
    from rvz.loss import differentiable
    seen = []

    def kernel(*a, **k):
        seen.append(k)
        return LR.as_kernel(*a, **k)
    fn = differentiable(kernel)
    g = torch.Generator().manual_seed(2)
    z, y = torch.randn(5, 65, generator=g), torch.tanh(torch.randn(5, generator=g))
    pi = torch.softmax(torch.randn(5, 65, generator=g), 1)
    t = torch.zeros(5)
    plain = fn(z, y, pi, t)
    rows = fn(z, y, pi, t, rows=True)
    assert seen == [dict(rows=False, grads=True), dict(rows=True, grads=True)]
    assert "rows" not in plain[3] and sorted(plain[3]) == ["agreement", "malformed",
                                                           "target_entropy", "weight_sum"]
    assert rows[3]["rows"].shape == (5, 3) and rows[3]["rows"].dtype == torch.float64
    assert torch.equal(plain[0], rows[0]) and torch.equal(plain[1], rows[1])
    assert float(rows[3]["rows"][:, 0].mean()) == pytest.approx(float(rows[1]), rel=1e-12)


def test_train_replay_prioritized_on_cpu():
    from rvz.trainer import DDPTrainer
    buf = _filled(_buffer(32))
    before = buf.weight.clone()
    log = []
    upd = buf.priority_updater

    def updater(weight, slot, rows, *a):
        out = upd(weight, slot, rows, *a)
        log.append((slot.clone(), rows.clone(), a, out[0].clone(), out[1].clone()))
        return out
    buf.priority_updater = updater
    tr = DDPTrainer(_model(), policy_target="full", batch_size=16, policy_loss_weight=1.0,
                    value_loss_weight=0.5, loss_fn=_loss_fn())
    out = tr.train_replay(buf, 2, seed=3, priority_beta=0.7)
    assert out["steps"] == 2 and len(log) == 2
    for key in ("train/is_weight_mean", "train/priority_mean", "train/policy_kl", "train/loss"):
        assert math.isfinite(out[key]), key
    assert 0 < out["train/is_weight_mean"] <= 1
    assert buf.priority_floor <= out["train/priority_mean"] <= buf.priority_cap
    # the ring's weights changed at exactly the winning sampled slots, to the values the
    # sequential rule gives for the loss rows of each step, with the trainer's loss weights
    want = before.numpy().copy()
    touched = set()
    for slot, rows, a, pri, state in log:
        assert a[:2] == (1.0, 0.5) and a[2:6] == (True, 0.6, 2.0 ** -8, 2.0 ** 8)
        want, p, st, _ = P.priority(want, slot.numpy(), rows.numpy(), 1.0, 0.5)
        assert np.array_equal(p, pri.numpy()) and np.array_equal(st, state.numpy())
        assert (state >= 0).all() and (state == 1).any()
        touched |= set(slot[state == 1].tolist())
    assert np.array_equal(buf.weight.numpy(), want)
    changed = set(np.flatnonzero(buf.weight.numpy() != before.numpy()).tolist())
    assert changed and changed <= touched and touched <= set(range(24))
    assert np.array_equal(buf.weight.numpy()[24:], before.numpy()[24:])
    mean = np.mean([float(pri[state >= 0].double().mean()) for _, _, _, pri, state in log])
    assert out["train/priority_mean"] == pytest.approx(mean, rel=1e-12)
    assert buf.max_priority() == max(1.0, max(float(x[3].max()) for x in log))
    assert buf._dirty
    # step 1 drew through the priorities step 0 wrote
    first = P.priority(before.numpy(), log[0][0].numpy(), log[0][1].numpy(), 1.0, 0.5)[0]
    ref = W.batch(buf.mover.numpy(), buf.opponent.numpy(), buf.policy.numpy(), buf.value.numpy(),
                  W.cdf(first, 0, 24), 0, 24, 16, 3, 1)
    assert np.array_equal(ref[3], log[1][0].numpy())
    # it needs the full policy loss
    with pytest.raises(ValueError):
        DDPTrainer(_model()).train_replay(buf, 1)
    with pytest.raises(ValueError):
        DDPTrainer(_model()).train_step(torch.zeros(1, 3, 8, 8), torch.zeros(1, 65),
                                        torch.zeros(1, 1), rows=True)


def test_unprioritized_train_replay_is_unchanged():
    """A weighted buffer that is not prioritized takes the path of before: the calls it
    receives, the loss_fn's arguments and the trained bytes."""
    import rvz
    from rvz.trainer import DDPTrainer

    def run(spy):
        buf = rvz.ReplayBuffer(32, 8, "cpu", weighted=True, weighted_batcher=W.weighted_batcher,
                               cdf_builder=W.cdf_builder)
        _filled(buf)
        calls = []
        sample = buf.sample

        def sampled(*a, **k):
            calls.append((a, k))
            return sample(*a, **k)
        fn = _loss_fn()

        def loss_fn(*a, **k):
            calls.append(("loss", len(a), a[4], k))
            return fn(*a, **k)
        if spy:
            buf.sample = sampled
        model = _model()
        tr = DDPTrainer(model, policy_target="full", batch_size=16,
                        loss_fn=loss_fn if spy else fn)
        out = tr.train_replay(buf, 2, seed=3)
        return model, out, calls, buf

    a, out_a, calls, buf = run(True)
    assert calls == [((16, 3, 0, True), {}), ("loss", 8, None, {}),
                     ((16, 3, 1, True), {}), ("loss", 8, None, {})]
    assert sorted(out_a) == ["steps", "train/loss", "train/lr", "train/policy_agreement",
                             "train/policy_kl", "train/policy_loss", "train/value_loss"]
    assert buf.weight[:24].tolist() == [1.0] * 24 and not buf._dirty
    # the same bytes as the loop written out by hand on the old interface
    b = _model()
    tr = DDPTrainer(b, policy_target="full", batch_size=16, loss_fn=_loss_fn())
    buf2 = run(False)[3]
    for s in range(2):
        tr.train_step(*buf2.sample(16, 3, s, True)[:3])
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    c, out_c, _, _ = run(False)
    assert out_c == out_a and all(torch.equal(sa[k], c.state_dict()[k]) for k in sa)


def test_selfplay_trainer_priority_arguments():
    from rvz.pipeline import SelfPlayTrainer
    m = torch.nn.Linear(1, 1)
    ok = dict(replay_sampling="priority", replay_iterations=2, policy_target="full")
    for bad, says in ((dict(ok, replay_iterations=0), "replay_iterations"),
                      (dict(ok, policy_target="argmax"), "policy_target"),
                      (dict(ok, replay_priority_alpha=1.5), "replay_priority_alpha"),
                      (dict(ok, replay_priority_alpha=True), "replay_priority_alpha"),
                      (dict(ok, replay_priority_beta=-0.1), "replay_priority_beta"),
                      (dict(ok, replay_priority_beta=(0.4, 1.0)), "replay_priority_beta"),
                      (dict(ok, replay_priority_beta=(0.4, 1.5, 10)), "replay_priority_beta"),
                      (dict(ok, replay_priority_beta=(0.4, 1.0, 0)), "replay_priority_beta"),
                      (dict(ok, replay_priority_beta=(0.4, 1.0, 2.5)), "replay_priority_beta"),
                      (dict(ok, replay_priority_beta="0.4"), "replay_priority_beta"),
                      (dict(replay_iterations=2, replay_priority_alpha=0.5), "replay_sampling"),
                      (dict(replay_iterations=2, replay_priority_beta=1.0), "replay_sampling"),
                      (dict(replay_sampling="prioritised", replay_iterations=2),
                       "replay_sampling")):
        with pytest.raises(ValueError) as err:
            SelfPlayTrainer(m, games=4, **bad)
        assert says in str(err.value), (bad, str(err.value))
    import types
    spt = types.SimpleNamespace(replay_priority_beta=(0.4, 1.0, 4), iteration=1)
    beta = SelfPlayTrainer.priority_beta
    assert [beta(spt, i) for i in (0, 1, 2, 4, 9)] == [0.4, 0.55, 0.7, 1.0, 1.0]
    assert beta(spt) == 0.55
    spt.replay_priority_beta = 0.25
    assert beta(spt) == 0.25 and beta(spt, 100) == 0.25
    # the iteration's rows enter a prioritized buffer at its running maximum
    buf = _buffer(32)
    buf.update_priorities(_i32(0), _f64((30.0, 0.0, 0.0)))
    top = buf.max_priority()
    assert top > 1.0
    mover, opponent, policy, value = _rows(8, 0, 3)
    spt = types.SimpleNamespace(buffer=buf, replay_sampling="priority", iteration=0)
    SelfPlayTrainer._append(spt, {"mover": mover, "opponent": opponent, "policy_targets": policy,
                                  "value_targets": value.reshape(-1, 1)})
    assert _held_weights(buf) == [top] * 3
