"""Weighted replay sampling without a GPU: the reference (tests/replay_weighted_ref.py) at the
edges of its search and in its frequencies, ReplayBuffer(weighted=True) on CPU tensors with the
reference's callables (weights that wrap, leave with their rows and age by recency_decay; the
table rebuilt after an append only), SelfPlayTrainer's new arguments, and the argument checks of
rvz_replay_cdf / rvz_replay_batch_weighted (they run before any HIP call)."""
import math
import types

import numpy as np
import pytest
import torch

import merge_ref as M
import replay_ref as RR
import replay_weighted_ref as W
from test_pipeline_cpu import synthetic_records
from test_replay_cpu import _rows
from test_solve_cpu import _train

EINVAL = -22
FREQ_WEIGHTS = (1, 0, 2, 0.5, 0, 4, 0.25, 0.25)


def _buffer(capacity, bs=8, window=0, decay=1.0, builder=W.cdf_builder):
    import rvz
    return rvz.ReplayBuffer(capacity, bs, "cpu", window_iterations=window, weighted=True,
                            recency_decay=decay, weighted_batcher=W.weighted_batcher,
                            cdf_builder=builder)


def _w(*x):
    return torch.tensor(x, dtype=torch.float32)


def _held_weights(buf):
    """The weights of the rows held, oldest first."""
    at = (buf.start + torch.arange(len(buf))) % buf.capacity
    return buf.weight[at].tolist()


# ---------------------------------------------------------------- the reference itself
def test_fixed_point():
    assert W.q(0.0) == 0 and W.q(-0.0) == 0 and W.q(1.0) == 65536 and W.q(65536.0) == 1 << 32
    assert W.q(2.0 ** -17) == 0 and W.q(3 * 2.0 ** -17) == 2      # halves go to even
    assert W.q(2.0 ** -16) == 1 and W.q(0.25) == 16384
    for bad in (float("nan"), float("inf"), -float("inf"), -1.0, -1e-30, 65537.0,
                np.nextafter(np.float32(65536), np.float32(1e9))):
        assert W.q(bad) is None, bad
    t = W.cdf(np.array([9, 1, float("nan"), 0.5, -1, 65537, float("inf"), 2], np.float32), 6, 5)
    # logical rows: slots 6, 7, 0, 1, 2 = inf, 2, 9, 1, nan
    assert t.dtype == np.uint64 and t.tolist() == [12 << 16, 2, 6, 5, 0, 2 << 16, 11 << 16,
                                                   12 << 16, 12 << 16]
    assert W.cdf(np.ones(3, np.float32), 2, 0).tolist() == [0, 0, 2, 0]


def test_search_edges_through_word():
    """t = 0, t = total - 1, and t = C[i] - 1 / t = C[i] for a row followed by a run of
    zero-weight rows; zero weights at both ends of the ring are never chosen."""
    #                     slot: 0  1  2  3  4  5  6  7      start 6: rows 6, 7, 0, 1, 2, 3, 4, 5
    weight = np.array([3, 0, 0, 0, 5, 0, 0, 2], np.float32)
    start, live = 6, 8
    t = W.cdf(weight, start, live)
    C = [int(c) for c in t[4:]]
    total = int(t[0])
    assert C == [0, 2 << 16, 5 << 16, 5 << 16, 5 << 16, 5 << 16, 10 << 16, 10 << 16]
    assert total == 10 << 16
    assert W.search(C, 0) == 1 and W.search(C, total - 1) == 6    # never rows 0 and 7
    assert W.search(C, C[2] - 1) == 2 and W.search(C, C[2]) == 6  # past the run of zeros
    assert W.search(C, C[1] - 1) == 1 and W.search(C, C[1]) == 2
    for want_t, row in ((0, 1), (total - 1, 6), (C[2] - 1, 2), (C[2], 6), (C[1], 2)):
        for u in (W.word_for(want_t, total), W.word_for(want_t + 1, total) - 1
                  if want_t + 1 < total else W.WORD_MAX):
            i, _, got_t = W.draw(t, 0, 0, 0, word=u)
            assert (i, got_t) == (row, want_t), (want_t, u)
    assert W.draw(t, 0, 0, 0, word=0)[0] == 1 and W.draw(t, 0, 0, 0, word=W.WORD_MAX)[0] == 6
    # the whole batch: slots, probabilities, and never a zero-weight row
    ring = RR.ring(8, 8)
    out = W.batch(*ring, t, start, live, 4096, 7, 1)
    assert set(out[3].tolist()) == {7, 0, 4}
    for slot, p in ((7, 0.2), (0, 0.3), (4, 0.5)):
        assert set(out[5][out[3] == slot].tolist()) == {float(np.float32(p))}
    # a total of 0 and a stale table: zero rows
    zero = W.cdf(np.zeros(8, np.float32), start, live)
    for table, kw in ((zero, {}), (t, {"start_": 5}), (t, {"live_": 7})):
        out = W.batch(*ring, table, kw.get("start_", start), kw.get("live_", live), 9, 7, 1)
        assert not out[0].any() and not out[1].any() and not out[2].any() and not out[5].any()
        assert set(out[3].tolist()) == {-1} and set(out[4].tolist()) == {-1}
    given = W.batch(*ring, zero, start, live, 3, 7, 1, idx=[0, 1, 9])
    assert given[3].tolist() == [6, 7, -1] and not given[5].any() and given[0][:2].any()


def test_reference_frequencies():
    """live = 8, nb = 65,536: every row's count is within 5 sqrt(nb p (1 - p)) of nb p, and the
    zero-weight rows are never drawn."""
    nb = 65536
    t = W.cdf(np.array(FREQ_WEIGHTS, np.float32), 0, 8)
    C = [int(c) for c in t[4:]]
    rows = [W.draw(t, 2024, 5, r)[0] for r in range(nb)]
    count = np.bincount(rows, minlength=8)
    total = sum(FREQ_WEIGHTS)
    for i, w in enumerate(FREQ_WEIGHTS):
        p = w / total
        assert abs(count[i] - nb * p) <= 5 * math.sqrt(nb * p * (1 - p)), (i, count[i], nb * p)
        assert w or count[i] == 0
    assert C[-1] == int(total * 65536)
    # the symmetry is replay_batch's for the same (seed, step, r); the row is not
    ks = [W.draw(t, 2024, 5, r)[1] for r in range(64)]
    assert ks == RR.draws(2024, 5, 64, 8)[1].tolist()
    ones = W.cdf(np.ones(8, np.float32), 0, 8)
    assert [W.draw(ones, 2024, 5, r)[0] for r in range(64)] != RR.draws(2024, 5, 64, 8)[0].tolist()


# ---------------------------------------------------------------- ReplayBuffer(weighted=True)
def test_weights_wrap_and_leave_with_their_rows():
    buf = _buffer(7)
    assert buf.weight.shape == (7,) and buf.weight.dtype == torch.float32
    buf.append(*_rows(8, 0, 3), 0, weight=_w(1, 2, 3))
    buf.append(*_rows(8, 3, 6), 1)                            # no weights: 1.0 each
    assert _held_weights(buf) == [1, 2, 3, 1, 1, 1]
    buf.append(*_rows(8, 6, 9), 2, weight=_w(7, 8, 9))        # slots 6, 0, 1: evicts rows 0, 1
    assert len(buf) == 7 and buf.start == 2
    assert buf.weight.tolist() == [8, 9, 3, 1, 1, 1, 7]
    assert _held_weights(buf) == [3, 1, 1, 1, 7, 8, 9]
    assert buf.total_weight() == 30.0 and buf.invalid_weights() == 0
    out = buf.sample(512, 3, 0, with_prob=True)
    assert len(out) == 6 and len(buf.sample(4, 3, 0)) == 5
    want = W.batch(buf.mover.numpy(), buf.opponent.numpy(), buf.policy.numpy(),
                   buf.value.numpy(), W.cdf(buf.weight.numpy(), 2, 7), 2, 7, 512, 3, 0)
    for g, x in zip(out, want):
        assert np.array_equal(g.numpy(), x)
    value_of = {int(round(float(v) * 1000)): float(p) for v, p in zip(out[2].reshape(-1), out[5])}
    assert value_of == {r: float(np.float32(w / 30)) for r, w in
                        zip(range(2, 9), (3, 1, 1, 1, 7, 8, 9))}
    # given rows and words
    idx = torch.arange(7)
    got = buf.sample(7, 0, 0, idx=idx, sym=torch.zeros(7, dtype=torch.int32), with_prob=True)
    assert got[3].tolist() == [2, 3, 4, 5, 6, 0, 1]
    assert got[5].tolist() == [float(np.float32(w / 30)) for w in (3, 1, 1, 1, 7, 8, 9)]
    word = torch.from_numpy(np.array([0, W.WORD_MAX], np.uint64).view(np.int64))
    assert buf.sample(2, 0, 0, word=word)[3].tolist() == [2, 1]
    # by the window
    win = _buffer(16, window=2)
    win.append(*_rows(8, 0, 4), 0, weight=_w(5, 5, 5, 5))
    win.append(*_rows(8, 4, 9), 1, weight=_w(1, 2, 3, 4, 5))
    win.append(*_rows(8, 9, 12), 2, weight=_w(6, 7, 8))       # iteration 0 leaves
    assert win.start == 4 and _held_weights(win) == [1, 2, 3, 4, 5, 6, 7, 8]
    assert win.total_weight() == 36.0
    # invalid weights are counted and never drawn
    bad = _buffer(7)
    bad.append(*_rows(8, 0, 5), 0, weight=_w(float("nan"), -1, 2, 65537, float("inf")))
    assert bad.invalid_weights() == 4 and bad.total_weight() == 2.0
    assert set(bad.sample(64, 1, 1)[3].tolist()) == {2}


def test_recency_decay_once_per_newer_iteration():
    buf = _buffer(16, decay=0.7)
    f = np.float32(0.7)
    buf.append(*_rows(8, 0, 2), 3, weight=_w(1, 3))
    assert _held_weights(buf) == [1, 3]
    buf.append(*_rows(8, 2, 3), 3, weight=_w(5))              # the same iteration: no decay
    assert _held_weights(buf) == [1, 3, 5]
    buf.append(*_rows(8, 3, 4), 4)
    want = [np.float32(1) * f, np.float32(3) * f, np.float32(5) * f, np.float32(1)]
    assert _held_weights(buf) == [float(x) for x in want]
    buf.append(*_rows(8, 4, 4), 9)                            # no rows: nothing ages
    assert _held_weights(buf) == [float(x) for x in want]
    buf.append(*_rows(8, 4, 5), 6, weight=_w(2))              # two iterations on: float32(0.7^2)
    f2 = np.float32(0.7 ** 2)
    want = [x * f2 for x in want] + [np.float32(2)]
    assert _held_weights(buf) == [float(x) for x in want]
    assert buf.total_weight() == sum(W.q(x) for x in want) / 65536
    # 1.0 is the default and leaves the weights alone
    plain = _buffer(16)
    plain.append(*_rows(8, 0, 2), 0, weight=_w(1, 3))
    plain.append(*_rows(8, 2, 3), 5)
    assert _held_weights(plain) == [1, 3, 1]


def test_table_is_rebuilt_after_an_append_only():
    calls = []

    def builder(*a):
        calls.append(a[1:4])
        return W.cdf_builder(*a)

    buf = _buffer(7, window=2, builder=builder)
    buf.append(*_rows(8, 0, 3), 0)
    buf.append(*_rows(8, 3, 5), 0)
    assert calls == []                                        # lazily
    a = buf.sample(8, 1, 0)
    b = buf.sample(8, 1, 1)
    assert calls == [(0, 5, 0)] and not torch.equal(a[3], b[3])
    table = buf._cdf
    assert buf.total_weight() == 5.0 and buf.invalid_weights() == 0 and len(calls) == 1
    buf.append(*_rows(8, 5, 7), 1)
    assert len(calls) == 1
    buf.sample(8, 1, 2)
    assert calls[1:] == [(0, 7, 0)] and buf._cdf is table     # the buffer allocated once
    buf.append(*_rows(8, 7, 7), 2)                            # no rows, but iteration 0 leaves
    buf.sample(8, 1, 3)
    assert calls[2:] == [(5, 2, 0)] and len(buf) == 2
    buf.sample(8, 1, 4)
    assert len(calls) == 3


def test_unweighted_buffers_are_unchanged():
    import rvz
    buf = rvz.ReplayBuffer(7, 8, "cpu", batcher=RR.batcher)
    assert not buf.weighted and not hasattr(buf, "weight") and not hasattr(buf, "_cdf")
    buf.append(*_rows(8, 0, 5), 0)
    got = buf.sample(16, 3, 1)
    want = RR.batch(buf.mover.numpy(), buf.opponent.numpy(), buf.policy.numpy(),
                    buf.value.numpy(), 0, 5, 16, 3, 1)
    assert len(got) == 5 and all(np.array_equal(g.numpy(), x) for g, x in zip(got, want))
    for call in (lambda: buf.append(*_rows(8, 5, 6), 0, weight=_w(1)),
                 lambda: buf.sample(4, 0, 0, with_prob=True),
                 lambda: buf.sample(4, 0, 0, word=torch.zeros(4, dtype=torch.int64)),
                 buf.total_weight, buf.invalid_weights,
                 lambda: rvz.ReplayBuffer(7, 8, "cpu", recency_decay=0.5),
                 lambda: rvz.ReplayBuffer(7, 8, "cpu", weighted_batcher=W.weighted_batcher),
                 lambda: rvz.ReplayBuffer(7, 8, "cpu", cdf_builder=W.cdf_builder)):
        with pytest.raises(ValueError):
            call()
    assert len(buf) == 5
    for decay in (0.0, -0.5, 1.5, float("nan"), "0.5", True):
        with pytest.raises(ValueError):
            rvz.ReplayBuffer(7, 8, "cpu", weighted=True, recency_decay=decay)
    w = _buffer(7)
    for weight in (_w(1, 2), _w(1).double(), torch.ones(1, 1)):
        with pytest.raises(ValueError):
            w.append(*_rows(8, 0, 1), 0, weight=weight)
    with pytest.raises(ValueError):
        w.sample(4, 0, 0)                                     # empty
    assert w.total_weight() == 0.0 and w.invalid_weights() == 0


# ---------------------------------------------------------------- SelfPlayTrainer
def test_selfplay_trainer_refuses_the_missing_combinations():
    from rvz.pipeline import SelfPlayTrainer
    m = torch.nn.Linear(1, 1)
    for bad, says in ((dict(replay_sampling="counts", merge_positions=True), "replay_iterations"),
                      (dict(replay_sampling="counts", replay_iterations=2), "merge_positions"),
                      (dict(replay_sampling="priorities", replay_iterations=2), "replay_sampling"),
                      (dict(replay_recency_decay=0.9), "replay_iterations"),
                      (dict(replay_recency_decay=0.0, replay_iterations=2), "(0, 1]"),
                      (dict(replay_recency_decay=1.5, replay_iterations=2), "(0, 1]")):
        with pytest.raises(ValueError) as err:
            SelfPlayTrainer(m, games=4, **bad)
        assert says in str(err.value), (bad, str(err.value))
    # the existing refusal stands, with its message
    with pytest.raises(ValueError) as err:
        SelfPlayTrainer(m, games=4, policy_target="full", count_weights=True,
                        merge_positions=True, replay_iterations=2, replay_sampling="counts")
    assert "count_weights=True needs replay_iterations=0" in str(err.value)


def test_merged_rows_append_their_counts_as_weights():
    """SelfPlayTrainer's append of an iteration's data: with replay_sampling="counts" the merged
    compact rows' position_counts are the weights; with "uniform" every weight is 1."""
    from rvz.pipeline import SelfPlayTrainer
    rec, _ = synthetic_records(G=6, seed=3)
    data = _train(rec, 8, merge_positions=True, merger=M.host_merger, compact=True)
    counts = data["position_counts"]
    n = counts.numel()
    assert counts.dtype == torch.int32 and int(counts.max()) == 6 and int(counts.min()) == 1
    for sampling, want in (("counts", counts.tolist()), ("uniform", [1] * n)):
        spt = types.SimpleNamespace(buffer=_buffer(n + 5, decay=0.5), replay_sampling=sampling,
                                    iteration=4)
        SelfPlayTrainer._append(spt, data)
        assert len(spt.buffer) == n and spt.buffer.rows_by_iteration() == [(4, n)]
        assert _held_weights(spt.buffer) == want
        assert spt.buffer.total_weight() == float(sum(want))
        # row 0 is the start position: drawn as often as the six games that began there
        out = spt.buffer.sample(1, 0, 0, idx=torch.zeros(1, dtype=torch.int32), with_prob=True)
        assert float(out[5]) == float(np.float32(want[0] / sum(want))) and want[0] in (1, 6)
    spt.replay_sampling = "counts"
    spt.iteration = 5
    SelfPlayTrainer._append(spt, data)                        # evicts, ages and appends
    assert len(spt.buffer) == n + 5
    assert _held_weights(spt.buffer) == [0.5] * 5 + counts.tolist()


# ---------------------------------------------------------------- the C-ABI's argument checks
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """RVZ_EINVAL before any HIP call (the pointers are never dereferenced)."""
    import rvz
    lib = rvz.load()
    p = 0x10000
    # rvz_replay_cdf_size
    assert lib.rvz_replay_cdf_size(1, 0) >= 8 * 5
    for tl in (0, 6, 9, 12):
        sizes = [lib.rvz_replay_cdf_size(c, tl) for c in (1, 2, 63, 64, 65, 4095, 4096, 4097,
                                                          2 ** 21, 2 ** 31 - 1)]
        assert sizes == sorted(sizes) and all(s % 16 == 0 for s in sizes), tl
        assert all(s >= 8 * (4 + c) for s, c in zip(sizes, (1, 2, 63, 64, 65, 4095, 4096, 4097,
                                                           2 ** 21, 2 ** 31 - 1)))
    assert lib.rvz_replay_cdf_size(2 ** 31 - 1, 6) < 8 * 1.04 * 2 ** 31
    for cap, tl in ((0, 0), (-1, 0), (7, 5), (7, 13), (7, -1), (7, 1)):
        assert lib.rvz_replay_cdf_size(cap, tl) < 0, (cap, tl)
    # rvz_replay_cdf:  cap weight start live tile cdf stream
    good = [7, p, 5, 3, 0, p, None]
    for k, v in ((0, 0), (0, -1), (2, -1), (2, 7), (3, -1), (3, 8), (4, 5), (4, 13), (4, -6),
                 (1, None), (5, None), (5, p + 8), (5, p + 4)):
        args = list(good)
        args[k] = v
        assert lib.rvz_replay_cdf(*args) == EINVAL, (k, v)
    assert lib.rvz_replay_cdf(7, None, 5, 0, 0, None, None) == 0      # live = 0: nothing to do
    for k, v in ((0, 0), (2, 7), (4, 13)):                            # refused at live = 0 too
        args = [7, None, 5, 0, 0, None, None]
        args[k] = v
        assert lib.rvz_replay_cdf(*args) == EINVAL, (k, v)
    # rvz_replay_batch_weighted
    #       0  1  2 .. 5     6  7  8  9  10    11    12   13 14 15 16 .. 20       21 (prob) 22
    good = [8, 7, p, p, p, p, p, 5, 3, 4, None, None, None, 1, 0, 0, p, p, p, p, p, None, None]
    for bs in (8, 6):
        zero = [bs, 7] + [None] * 5 + [5, 3, 0, None, None, None, 1, 2 ** 64 - 1, 2 ** 64 - 1] + \
            [None] * 7
        assert lib.rvz_replay_batch_weighted(*zero) == 0              # nb = 0: nothing to do
    for k, v in ((0, 7), (0, 4), (1, 0), (1, -1), (8, 0), (8, 8), (8, -1), (7, -1), (7, 7),
                 (9, -1), (9, 2 ** 31 // 65 + 1), (16, p + 4), (16, p + 8), (6, p + 8),
                 (6, p + 4)):
        args = list(good)
        args[k] = v
        assert lib.rvz_replay_batch_weighted(*args) == EINVAL, (k, v)
    args = list(good)
    args[0], args[9] = 6, 2 ** 31 // 37 + 1
    assert lib.rvz_replay_batch_weighted(*args) == EINVAL
    for k in (2, 3, 4, 5, 6, 16, 17, 18, 19, 20):             # idx, sym, word and prob may be null
        args = list(good)
        args[k] = None
        assert lib.rvz_replay_batch_weighted(*args) == EINVAL, k
    for k, v in ((0, 7), (1, 0), (8, 0), (8, 8), (7, 7)):     # refused at nb = 0 too
        args = list(good)
        args[9], args[k] = 0, v
        assert lib.rvz_replay_batch_weighted(*args) == EINVAL, (k, v)
    # the Python surface refuses malformed arguments before the library sees them
    w = torch.ones(7)
    for call in (lambda: rvz.replay_cdf(w.double(), 0, 7), lambda: rvz.replay_cdf(w, 7, 7),
                 lambda: rvz.replay_cdf(w, 0, 8), lambda: rvz.replay_cdf(w, 0, 7, tile_log2=5),
                 lambda: rvz.replay_cdf(w, 0, 7, out=torch.zeros(4, dtype=torch.int64)),
                 lambda: rvz.replay_cdf(w.reshape(7, 1), 0, 7), lambda: rvz.replay_cdf(w, 0, 7.0)):
        with pytest.raises(rvz.RvzError):
            call()
