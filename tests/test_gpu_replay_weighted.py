"""Weighted replay sampling on the GPU: rvz_replay_cdf's table against the Python-integer reference
(tests/replay_weighted_ref.py) byte for byte over its contract words, at every size where the
tiled scan takes another path; rvz_replay_batch_weighted against the reference and against
rvz_training_rows on the reported (slot, sym), bit for bit; the search's edges through `word`,
given and bad idx / sym (and rvz_replay_batch's own bytes for them), stale and all-zero tables,
purity, graph capture of table + draw,
ReplayBuffer(weighted=True) on the device against the reference-driven buffer, and one
SelfPlayTrainer(replay_sampling="counts") iteration. Outputs are pre-filled with NaN / a sentinel
before every raw call, so a comparison also shows that every element was written."""
import numpy as np
import pytest
import torch

import replay_ref as RR
import replay_weighted_ref as W
from test_gpu_replay import (PARENT_KEYS, SENTINEL, _appends, _bits, _by_training_rows, _fresh,
                             _i32, _ring)
from test_gpu_replay import _raw as _raw_uniform

pytestmark = pytest.mark.gpu

NAMES = ("states", "policy", "value", "slot", "sym", "prob")
TILE = 2048                                                   # the default tile
PALETTE = np.array([0, 0, 0.25, 1, 3, 0.5, 65536, 1e-5, 1234.567, 2.0 ** -17, 3 * 2.0 ** -17],
                   np.float32)
INVALID = np.array([float("nan"), -1, 65537, float("inf")], np.float32)


def _weights(n, seed, invalid=False):
    rng = np.random.default_rng(seed)
    w = PALETTE[rng.integers(0, len(PALETTE), size=n)]
    w[rng.integers(0, n)] = 7                                 # never all zero
    if invalid:
        at = rng.choice(n, size=min(n, 2 * len(INVALID)), replace=False)
        w[at] = np.resize(INVALID, len(at))
    return w


def _table(w, start, live, tile_log2=0):
    import rvz
    out = torch.full((rvz.load().rvz_replay_cdf_size(len(w), tile_log2) // 8,), -1,
                     dtype=torch.int64, device="cuda")
    got = rvz.replay_cdf(torch.from_numpy(w).cuda(), start, live, tile_log2, out=out)
    assert got is out
    return out


def _same_table(w, start, live, tile_log2=0):
    want = W.cdf(w, start, live)
    got = _table(w, start, live, tile_log2)[:4 + live].cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want), (len(w), start, live, tile_log2,
                                       np.flatnonzero(got != want)[:4])
    return want


# ---------------------------------------------------------------- the table
@pytest.mark.parametrize("live", [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_table_at_the_default_tile(live):
    _same_table(_weights(live, live), 0, live)
    cap = live + 3                                            # rows that wrap the ring's end
    _same_table(_weights(cap, live + 1), cap - 1, live)


@pytest.mark.parametrize("live", [4095, 4096, 4097])
def test_table_at_the_smallest_tile(live):
    """tile_log2 = 6: 64 * 64 + 1 rows reach the scan's third level."""
    _same_table(_weights(live, live), 0, live, 6)
    _same_table(_weights(live + 70, live + 1), 69, live, 6)   # wraps


def test_table_start_wrap_and_invalid_weights():
    w = _weights(300, 1)
    for start, live in ((123, 100), (123, 177), (123, 178), (123, 300), (299, 300), (0, 300)):
        _same_table(w, start, live)
    bad = _weights(300, 2, invalid=True)
    want = _same_table(bad, 250, 300)
    assert int(want[1]) == 8
    part = _same_table(bad, 0, 37)
    assert int(part[1]) == int(sum(W.q(x) is None for x in bad[:37]))
    only = _same_table(INVALID, 1, 4)                         # nothing valid: total 0
    assert only.tolist()[:2] == [0, 4]
    big = np.full(70, 65536, np.float32)                      # q = 2^32 each
    assert int(_same_table(big, 0, 70)[0]) == 70 << 32


def test_table_does_not_depend_on_the_tile():
    w = _weights(5003, 3, invalid=True)
    want = _same_table(w, 4000, 5000, 0)
    for tl in (6, 9, 12):
        assert np.array_equal(_same_table(w, 4000, 5000, tl), want)


# ---------------------------------------------------------------- the draw
def _raw(bs, dev, table, start, live, nb, seed=0, step=0, random_sym=1, idx=None, sym=None,
         word=None, out=None, prob=True, stream=None):
    """rvz_replay_batch_weighted through the C-ABI on pre-filled outputs."""
    import rvz
    from rvz._lib import ptr
    if out is None:
        out = _fresh(bs, nb) + (torch.full((nb,), float("nan"), device="cuda"),)
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    rc = rvz.load().rvz_replay_batch_weighted(
        bs, dev[0].numel(), *[ptr(t) for t in dev], ptr(table), start, live, nb, ptr(idx),
        ptr(sym), ptr(word), random_sym, seed, step, *[ptr(t) for t in out[:5]],
        ptr(out[5]) if prob else None, stream)
    assert rc == 0, rc
    return out


def _same(got, want, what=""):
    for g, x, name in zip(got, want, NAMES):
        x = torch.from_numpy(np.ascontiguousarray(x)).cuda().reshape(g.shape)
        assert g.dtype == x.dtype, (name, what)
        assert torch.equal(_bits(g), _bits(x)), (name, what)


def _words(ws):
    return torch.from_numpy(np.array(ws, np.uint64).view(np.int64)).cuda()


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 4096, 8195])
@pytest.mark.parametrize("bs", [8, 6])
def test_drawn_rows(bs, nb):
    """nb = 8,195 is three rows past one pass of the 2,048 blocks x 4 waves. live = 211 takes
    two rounds of the search."""
    cap, start, live = 300, 123, 211
    host, dev = _ring(bs, cap, 7, odd_values=True)
    w = _weights(cap, bs + nb, invalid=True)
    table = _table(w, start, live)
    seed, step = 2 ** 64 - 1 - nb, 2 ** 32 + bs
    got = _raw(bs, dev, table, start, live, nb, seed, step)
    want = W.batch(*host, W.cdf(w, start, live), start, live, nb, seed, step, True, None, None,
                   None, bs)
    _same(got, want, (bs, nb))
    slot = got[3].long()
    drawable = torch.tensor([bool(W.q(x)) for x in w]).cuda()     # valid and not zero
    assert int(slot.min()) >= 0 and bool(drawable[slot].all())
    states, policy, value = _by_training_rows(bs, dev, slot, got[4])
    assert torch.equal(_bits(got[0]), _bits(states)) and torch.equal(_bits(got[1]), _bits(policy))
    assert torch.equal(_bits(got[2]), _bits(value))
    # without out_prob and without symmetries
    plain = _raw(bs, dev, table, start, live, nb, seed, step, random_sym=0, prob=False)
    assert torch.equal(plain[3], got[3]) and not bool(plain[4].any())
    assert bool(torch.isnan(plain[5]).all())                  # untouched


@pytest.mark.parametrize("bs", [8, 6])
def test_deep_search_and_the_wrapper(bs):
    """live = 300,000: three rounds of the 64-ary search, then the last 64; through
    rvz.replay_batch_weighted."""
    import rvz
    cap, start, live, nb = 300007, 299000, 300000, 257
    host, dev = _ring(bs, cap, 11)
    w = _weights(cap, bs, invalid=True)
    table = _table(w, start, live)
    ref_table = W.cdf(w, start, live)
    assert np.array_equal(table[:4 + live].cpu().numpy().view(np.uint64), ref_table)
    got = rvz.replay_batch_weighted(*dev, table, start, live, nb, 5, 9, board_size=bs)
    assert got[2].shape == (nb, 1) and len(got) == 6
    _same(got, W.batch(*host, ref_table, start, live, nb, 5, 9, True, None, None, None, bs))
    total = int(ref_table[0])
    C = [int(c) for c in ref_table[4:]]
    edges = [0, total - 1, C[0], C[live // 2] - 1, C[live // 2], C[live - 2] - 1, C[63], C[64],
             C[4095], C[4096] - 1]
    ws = [W.word_for(t, total) for t in edges] + [W.WORD_MAX]
    got = rvz.replay_batch_weighted(*dev, table, start, live, len(ws), 5, 9, word=_words(ws),
                                    board_size=bs)
    _same(got, W.batch(*host, ref_table, start, live, len(ws), 5, 9, True, None, None, ws, bs))


@pytest.mark.parametrize("bs", [8, 6])
def test_search_edges_through_word(bs):
    """The CPU test's ring: t = 0, total - 1, C[i] - 1 and C[i] before a run of zero-weight rows,
    zero weights at both ends."""
    weight = np.array([3, 0, 0, 0, 5, 0, 0, 2], np.float32)
    start, live = 6, 8
    host, dev = _ring(bs, 8, 40)
    ref_table = W.cdf(weight, start, live)
    table = _table(weight, start, live)
    total, C = int(ref_table[0]), [int(c) for c in ref_table[4:]]
    ts = [0, total - 1, C[2] - 1, C[2], C[1] - 1, C[1]]
    ws = [W.word_for(t, total) for t in ts] + \
        [W.word_for(t + 1, total) - 1 for t in ts if t + 1 < total] + [0, W.WORD_MAX]
    got = _raw(bs, dev, table, start, live, len(ws), 3, 4, word=_words(ws))
    _same(got, W.batch(*host, ref_table, start, live, len(ws), 3, 4, True, None, None, ws, bs))
    assert got[3].tolist()[:6] == [7, 4, 0, 4, 7, 0]
    drawn = _raw(bs, dev, table, start, live, 4096, 3, 4)
    assert set(drawn[3].tolist()) == {7, 0, 4}


@pytest.mark.parametrize("bs", [8, 6])
def test_given_and_bad_rows(bs):
    cap, start, live, nb = 7, 5, 4, 9
    host, dev = _ring(bs, cap, 40, odd_values=True)
    w = np.array([1, 0, 65537, 9, 9, 2, 0.5], np.float32)      # logical rows: 2, 0.5, 1, 0
    table, ref_table = _table(w, start, live), W.cdf(w, start, live)
    idx = np.array([0, -1, 1, live, 2, 3, 3, -2 ** 31, 2 ** 31 - 1], np.int32)
    sym = np.array([1, 2, 3, 4, 8, 5, -1, 6, 9], np.int32)
    got = _raw(bs, dev, table, start, live, nb, idx=_i32(idx), sym=_i32(sym))
    _same(got, W.batch(*host, ref_table, start, live, nb, 0, 0, True, idx, sym, None, bs))
    assert got[3].tolist() == [5, -1, 6, -1, 0, 1, 1, -1, -1]
    assert got[4].tolist() == [1, -1, 3, -1, -1, 5, -1, -1, -1]
    p = [float(np.float32(x / 3.5)) for x in (2, 0.5, 1, 0)]
    assert got[5].tolist() == [p[0], 0, p[1], 0, p[2], p[3], p[3], 0, 0]
    one = _raw(bs, dev, table, start, live, nb, 3, 4, idx=_i32(idx))
    _same(one, W.batch(*host, ref_table, start, live, nb, 3, 4, True, idx, None, None, bs))
    two = _raw(bs, dev, table, start, live, nb, 3, 4, sym=_i32(sym))
    _same(two, W.batch(*host, ref_table, start, live, nb, 3, 4, True, None, sym, None, bs))
    assert int((two[4] == -1).sum()) == 3 and int((two[3] == -1).sum()) == 0


@pytest.mark.parametrize("nb", [1, 5])
@pytest.mark.parametrize("live", [7, 4])
@pytest.mark.parametrize("bs", [8, 6])
def test_given_rows_are_the_uniform_entry_points_rows(bs, live, nb):
    """One kernel behind both entry points: with idx and sym given (one idx outside [0, live),
    one sym outside [0, 8)) and a table for the same (start, live), the five common outputs are
    rvz_replay_batch's bit for bit; with a table built for another start every row is the zero
    row. Capacity 7 from slot 5: the rows wrap; nb = 5 is one block of four waves and one more."""
    cap, start = 7, 5
    _, dev = _ring(bs, cap, 11, odd_values=True)
    w = np.array([3, 0.5, 0, 1, 65536, 2.0 ** -17, 7], np.float32)
    idx = _i32(np.array([live - 1, 0, live, 2, 3], np.int32)[:nb])
    sym = _i32(np.array([7, 8, 2, 5, 0], np.int32)[:nb])
    if nb == 1:                                               # the row that wraps the furthest
        idx, sym = _i32([live - 1]), _i32([3])
    want = _raw_uniform(bs, dev, start, live, nb, 9, 2, idx=idx, sym=sym)
    got = _raw(bs, dev, _table(w, start, live), start, live, nb, 9, 2, idx=idx, sym=sym)
    for g, x, name in zip(got, want, NAMES):
        assert g.dtype == x.dtype and torch.equal(_bits(g), _bits(x)), name
    assert not bool(torch.isnan(got[5]).any())
    if nb == 5:
        assert got[3].tolist()[1:3] == [5, -1] and got[4].tolist()[1:3] == [-1, -1]
        assert bool(got[0][0].any()) and not bool(got[0][1:3].any())
    stale = _raw(bs, dev, _table(w, start - 1, live), start, live, nb, 9, 2, idx=idx, sym=sym)
    for t in stale[:3] + stale[5:]:
        assert torch.equal(_bits(t), torch.zeros_like(_bits(t)))
    assert set(stale[3].tolist()) == {-1} and set(stale[4].tolist()) == {-1}


# ---------------------------------------------------------------- errors and robustness
@pytest.mark.parametrize("bs", [8, 6])
def test_stale_and_empty_tables_give_zero_rows(bs):
    cap, start, live, nb = 300, 123, 211, 70
    host, dev = _ring(bs, cap, 7)
    w = _weights(cap, 5)
    table = _table(w, start, live)
    idx = _i32(np.arange(nb) % live)
    cases = [(table, start + 1, live, None), (table, start, live - 1, None),
             (table, start, live + 1, idx), (_table(np.zeros(cap, np.float32), start, live),
                                             start, live, None)]
    for tab, s, n, given in cases:
        got = _raw(bs, dev, tab, s, n, nb, 1, 2, idx=given)
        for t in got[:3] + got[5:]:
            assert not bool(t.any())
        assert set(got[3].tolist()) == {-1} and set(got[4].tolist()) == {-1}
    # an all-zero table still serves given rows, at probability 0
    zero = cases[3][0]
    got = _raw(bs, dev, zero, start, live, nb, 1, 2, idx=idx)
    ref_zero = W.cdf(np.zeros(cap, np.float32), start, live)
    _same(got, W.batch(*host, ref_zero, start, live, nb, 1, 2, True, np.arange(nb) % live, None,
                       None, bs))
    assert int(got[3].min()) >= 0 and not bool(got[5].any())


@pytest.mark.parametrize("bs", [8, 6])
def test_purity(bs):
    cap, start, live = 300, 123, 211
    _, dev = _ring(bs, cap, 7)
    table = _table(_weights(cap, 9), start, live)
    a = _raw(bs, dev, table, start, live, 200, 5, 9)
    b = _raw(bs, dev, table, start, live, 200, 5, 9)
    short = _raw(bs, dev, table, start, live, 64, 5, 9)
    for x, y, z, name in zip(a, b, short, NAMES):
        assert torch.equal(_bits(x), _bits(y)), name          # the same call twice
        assert torch.equal(_bits(x[:64]), _bits(z)), name     # a row does not depend on nb
    assert not torch.equal(_raw(bs, dev, table, start, live, 200, 5, 10)[3], a[3])
    assert not torch.equal(_raw(bs, dev, table, start, live, 200, 6, 9)[3], a[3])
    # neighbours changed: row 5 keeps its word, idx and sym, every other row gets others
    rng = np.random.default_rng(bs)
    outs = []
    for _ in range(2):
        word = rng.integers(0, 2 ** 63, size=64, dtype=np.uint64)
        sym = rng.integers(0, 8, size=64).astype(np.int32)
        word[5], sym[5] = 0x123456789ABCDEF0, 6
        outs.append(_raw(bs, dev, table, start, live, 64, 5, 9, word=_words(word),
                         sym=_i32(sym)))
    for x, y, name in zip(*outs, NAMES):
        assert torch.equal(_bits(x[5]), _bits(y[5])), name
    assert not torch.equal(outs[0][3], outs[1][3])


def test_graph_capture_of_table_and_draw():
    """rvz_replay_cdf + rvz_replay_batch_weighted captured once, replayed on other weights."""
    import rvz
    bs, cap, start, live, nb = 8, 5003, 4000, 5000, 257
    host, dev = _ring(bs, cap, 7)
    w_a, w_b = _weights(cap, 1, invalid=True), _weights(cap, 2)
    weight = torch.from_numpy(w_a).cuda()
    table = torch.zeros(rvz.load().rvz_replay_cdf_size(cap, 6) // 8, dtype=torch.int64,
                        device="cuda")
    rvz.replay_cdf(weight, start, live, 6, out=table)         # warm
    eager = [t.clone() for t in _raw(bs, dev, table, start, live, nb, 5, 9)]
    torch.cuda.synchronize()
    out = tuple(torch.empty_like(t) for t in eager)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rvz.replay_cdf(weight, start, live, 6, out=table)
        _raw(bs, dev, table, start, live, nb, 5, 9, out=out,
             stream=torch.cuda.current_stream().cuda_stream)
    for w in (w_b, w_a):
        weight.copy_(torch.from_numpy(w))
        table.fill_(-1)
        for t in out[:3] + out[5:]:
            t.fill_(float("nan"))
        for t in out[3:5]:
            t.fill_(SENTINEL)
        graph.replay()
        ref_table = W.cdf(w, start, live)
        assert np.array_equal(table[:4 + live].cpu().numpy().view(np.uint64), ref_table)
        _same(out, W.batch(*host, ref_table, start, live, nb, 5, 9, True, None, None, None, bs))
    for g, x, name in zip(out, eager, NAMES):
        assert torch.equal(_bits(g), _bits(x)), name


# ---------------------------------------------------------------- the Python layers
@pytest.mark.parametrize("bs", [8, 6])
def test_weighted_replay_buffer_on_the_device(bs):
    import rvz
    gpu = rvz.ReplayBuffer(300, bs, "cuda", weighted=True, recency_decay=0.75)
    cpu = rvz.ReplayBuffer(300, bs, "cpu", weighted=True, recency_decay=0.75,
                           weighted_batcher=W.weighted_batcher, cdf_builder=W.cdf_builder)
    assert gpu.weight.is_cuda and gpu.weighted_batcher is rvz.replay_batch_weighted
    assert gpu.cdf_builder is rvz.replay_cdf and gpu._cdf.is_cuda
    for it, rows in _appends(bs):
        w = torch.from_numpy(_weights(rows[0].numel(), it, invalid=it == 1))
        gpu.append(*[t.cuda() for t in rows], 2 * it, weight=w.cuda())
        cpu.append(*rows, 2 * it, weight=w)
        assert len(gpu) == len(cpu) and gpu.start == cpu.start
        assert torch.equal(gpu.weight.cpu().nan_to_num(nan=-5.0), cpu.weight.nan_to_num(nan=-5.0))
        for step in (0, 1):
            _same(gpu.sample(100, 3, step, with_prob=True),
                  [t.numpy() for t in cpu.sample(100, 3, step, with_prob=True)], (it, step))
        assert gpu.total_weight() == cpu.total_weight()
        assert gpu.invalid_weights() == cpu.invalid_weights()
    assert len(gpu) == 300 and gpu.start == 50 and gpu.invalid_weights() > 0
    assert len(gpu.sample(64, 4, 0)) == 5
    _same(gpu.sample(64, 4, 0, symmetries=False),
          [t.numpy() for t in cpu.sample(64, 4, 0, symmetries=False)])
    idx = torch.arange(300)
    word = torch.from_numpy(np.random.default_rng(0).integers(
        0, 2 ** 64, size=300, dtype=np.uint64).view(np.int64))
    _same(gpu.sample(300, 0, 0, idx=idx.cuda(), sym=(idx % 8).cuda(), with_prob=True),
          [t.numpy() for t in cpu.sample(300, 0, 0, idx=idx, sym=idx % 8, with_prob=True)])
    _same(gpu.sample(300, 0, 0, word=word.cuda(), with_prob=True),
          [t.numpy() for t in cpu.sample(300, 0, 0, word=word, with_prob=True)])


def test_selfplay_trainer_samples_by_counts():
    """6x6, a one-block 64-filter net, 8 games, a two-batch search: two iterations with a window
    of two, merged rows weighted by their counts."""
    import rvz
    from rvz.pipeline import SelfPlayTrainer
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(6, 1, 64).cuda()
    init = {k: v.clone() for k, v in net.state_dict().items()}
    spt = SelfPlayTrainer(net, games=8, num_simulations=32, batch_size=16, seed=0, train_batch=16,
                          train_steps=2, replay_iterations=2, merge_positions=True,
                          replay_sampling="counts", replay_recency_decay=0.5,
                          policy_target="full")
    assert spt.buffer.weighted and spt.buffer.recency_decay == 0.5
    rs = [spt.run_iteration() for _ in range(2)]
    for r in rs:
        assert set(r) >= PARENT_KEYS | {"replay_rows", "replay_iterations_held"}
        assert r["steps"] == 2 and np.isfinite(r["train/loss"])
        assert r["merge_rows"] == r["samples"] < r["merge_input_rows"]
    n0, n1 = rs[0]["samples"], rs[1]["samples"]
    assert len(spt.buffer) == n0 + n1 and spt.buffer.invalid_weights() == 0
    # every record of iteration 1 counts 1, every record of iteration 0 half of that
    assert spt.buffer.total_weight() == rs[0]["merge_input_rows"] / 2 + rs[1]["merge_input_rows"]
    assert float(spt.buffer.weight[0]) == 4.0 and float(spt.buffer.weight[n0]) == 8.0
    total = spt.buffer.total_weight()
    out = spt.buffer.sample(2, 1, 0, idx=torch.tensor([0, n0], device="cuda"), with_prob=True)
    assert out[5].tolist() == [float(np.float32(4 / total)), float(np.float32(8 / total))]
    assert int(spt.buffer.sample(256, 1, 0)[3].min()) >= 0
    moved = max((net.state_dict()[k].float() - init[k].float()).abs().max().item()
                for k in init if init[k].is_floating_point())
    assert moved > 0
    # the same set of keys as a uniform run: run_iteration's result does not change
    assert set(rs[0]) == set(rs[1])
