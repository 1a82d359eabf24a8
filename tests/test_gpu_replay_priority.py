"""Prioritized replay on the device: rvz_replay_priority and rvz_replay_is_weight against the host
reference (tests/replay_priority_ref.py) bit for bit (weight, out_priority, out_state,
max_priority, out_weight, out_min_prob), at the shapes where the kernels can go wrong; purity,
repeatability, graph capture of the whole step; ReplayBuffer(prioritized=True),
DDPTrainer.train_replay and SelfPlayTrainer(replay_sampling="priority") on the device."""
import numpy as np
import pytest
import torch

import replay_priority_ref as P
import replay_weighted_ref as W
from test_gpu_replay import PARENT_KEYS, _appends, _bits, _ring

pytestmark = pytest.mark.gpu

SENTINEL = -77
# nb = 1, a wave, a wave and a row, 16 workgroups and a row (256 rows a workgroup: 257 is the first
# two-workgroup batch and 65 rows double the 64-entry table)
NBS = (1, 64, 65, 257, 4097)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ring_weight(cap, seed):
    w = np.random.default_rng(seed).uniform(0, 9, cap).astype(np.float32)
    w[:3] = np.array([0x7FC12345, 0x80000000, 0x00012345], np.uint32).view(np.float32)[:min(3, cap)]
    return w


def _priority(weight, slot, rows, kw, max_priority=1.5, outs=True, stream=None):
    """rvz_replay_priority through the C-ABI on pre-filled outputs and a dirty scratch."""
    import rvz
    lib = rvz.load()
    nb = len(slot)
    w, s, r = _cuda(weight), _cuda(np.asarray(slot, np.int32)), _cuda(np.asarray(rows, np.float64))
    scratch = torch.full((lib.rvz_replay_priority_scratch_size(nb),), 0xA5, dtype=torch.uint8,
                         device="cuda")
    top = None if max_priority is None else torch.tensor([max_priority], dtype=torch.float32,
                                                          device="cuda")
    pri = torch.full((nb,), float("nan"), device="cuda") if outs else None
    state = torch.full((nb,), SENTINEL, dtype=torch.int32, device="cuda") if outs else None
    a = lambda t: None if t is None else t.data_ptr()           # noqa: E731
    rc = lib.rvz_replay_priority(
        len(weight), a(w), nb, a(s), a(r), kw.get("policy_coef", 1.0), kw.get("value_coef", 1.0),
        int(kw.get("subtract_entropy", True)), kw.get("alpha", 0.6), kw.get("floor", 2.0 ** -8),
        kw.get("cap", 2.0 ** 8), a(scratch), a(top), a(pri), a(state),
        torch.cuda.current_stream().cuda_stream if stream is None else stream)
    assert rc == 0, rc
    return w, pri, state, top


def _same_priority(weight, slot, rows, kw=None, max_priority=1.5, states=True):
    kw = kw or {}
    got = _priority(weight, slot, rows, kw, max_priority)
    want = P.priority(weight, slot, rows, max_priority=max_priority, **kw)
    for g, x, name in zip(got, want, ("weight", "priority", "state", "max_priority")):
        x = _cuda(np.atleast_1d(x))
        assert g.dtype == x.dtype and torch.equal(_bits(g), _bits(x)), (name, len(slot), kw)
    if states:                                                  # not vacuous: every kind occurs
        assert set(want[2].tolist()) == {-1, 0, 1}, (len(slot), kw)
    return want


def _is_weight(prob, slot, beta, with_min=True):
    import rvz
    lib = rvz.load()
    nb = len(prob)
    p, s = _cuda(np.asarray(prob, np.float32)), _cuda(np.asarray(slot, np.int32))
    scratch = torch.full((lib.rvz_replay_is_weight_scratch_size(nb),), 0xA5, dtype=torch.uint8,
                         device="cuda")
    out = torch.full((nb,), float("nan"), device="cuda")
    pmin = torch.full((1,), float("nan"), device="cuda") if with_min else None
    rc = lib.rvz_replay_is_weight(nb, p.data_ptr(), s.data_ptr(), beta, scratch.data_ptr(),
                                  out.data_ptr(), None if pmin is None else pmin.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return out, pmin


def _same_is_weight(prob, slot, beta):
    out, pmin = _is_weight(prob, slot, beta)
    want = P.is_weight(prob, slot, beta)
    assert torch.equal(_bits(out), _bits(_cuda(want[0]))), (len(prob), beta)
    assert torch.equal(_bits(pmin), _bits(_cuda(np.atleast_1d(want[1])))), (len(prob), beta)
    return want


# ---------------------------------------------------------------- rvz_replay_priority
@pytest.mark.parametrize("nb", NBS)
def test_priority_mixed_rows(nb):
    """Random rows mixed with every invalid kind; slots from a ring of nb / 2 + 3, so about half
    the rows are superseded. nb = 1 cannot show three states: its row is valid, then invalid."""
    cap = nb // 2 + 3
    slot, rows = P.mixed_rows(np.random.default_rng(nb), nb, cap)
    if nb == 1:
        slot[0] = 2
        assert _same_priority(_ring_weight(cap, nb), slot, rows, states=False)[2].tolist() == [1]
        for bad_slot, bad_row in ((-1, rows[0]), (cap, rows[0]), (2, P.INVALID_ROWS[0])):
            want = _same_priority(_ring_weight(cap, nb), [bad_slot], [bad_row], states=False)
            assert want[2].tolist() == [-1]
        return
    _same_priority(_ring_weight(cap, nb), slot, rows)


@pytest.mark.parametrize("subtract_entropy", [True, False])
@pytest.mark.parametrize("alpha", [0.0, 0.5, 0.6, 1.0])
def test_priority_alpha_and_entropy(alpha, subtract_entropy):
    slot, rows = P.mixed_rows(np.random.default_rng(7), 65, 40)
    kw = dict(alpha=alpha, subtract_entropy=subtract_entropy, policy_coef=1.25, value_coef=0.5,
              floor=2.0 ** -16, cap=65536.0)
    want = _same_priority(_ring_weight(40, 1), slot, rows, kw)
    if alpha == 0.0:
        assert set(want[1][want[2] >= 0].tolist()) == {1.0}


def test_priority_nearly_all_duplicates_and_one_slot():
    slot, rows = P.mixed_rows(np.random.default_rng(11), 4097, 8)
    _same_priority(_ring_weight(8, 2), slot, rows, dict(floor=0.125, cap=4.0))
    # every row in one slot: the last valid row's priority, every other valid row superseded
    slot, rows = P.mixed_rows(np.random.default_rng(12), 4097, 8, slots=np.full(4097, 5))
    rows[4096] = P.INVALID_ROWS[3]                              # the last row is invalid
    want = _same_priority(_ring_weight(8, 3), slot, rows)
    winner = np.flatnonzero(want[2] == 1)
    assert len(winner) == 1 and winner[0] == np.flatnonzero(want[2] >= 0).max() < 4096
    # e overflows to inf although every entry is finite: an invalid row
    slot, rows = P.mixed_rows(np.random.default_rng(13), 257, 100)
    _same_priority(_ring_weight(100, 4), slot, rows, dict(policy_coef=1e10, value_coef=1e308))


def test_priority_distinct_slots_in_a_large_ring():
    """Capacity 2^20, all valid slots distinct but one pair at rows 1 and nb - 1 (and, apart
    from it, a pair at rows 0 and nb - 1 in a second call)."""
    nb, cap = 4097, 1 << 20
    rng = np.random.default_rng(4097)
    slot, rows = P.mixed_rows(rng, nb, cap)
    spread = rng.permutation(cap)[:nb].astype(np.int32)
    slot = np.where((slot >= 0) & (slot < cap), spread, slot).astype(np.int32)
    weight = _ring_weight(cap, 5)
    for first in (1, 0):
        s, r = slot.copy(), rows.copy()
        s[first] = s[nb - 1] = cap - 1
        r[first], r[nb - 1] = (2.0, 1.0, 0.5), (0.5, 0.25, 0.125)
        want = _same_priority(weight, s, r)
        assert want[2][first] == 0 and want[2][nb - 1] == 1
        assert (want[2] == 0).sum() == 1                        # the one duplicate pair
        assert (want[0].view(np.int32) != weight.view(np.int32)).sum() == (want[2] == 1).sum()


def test_priority_nullable_outputs_and_repeatability():
    slot, rows = P.mixed_rows(np.random.default_rng(21), 300, 64)
    weight = _ring_weight(64, 6)
    a = _priority(weight, slot, rows, {})
    b = _priority(weight, slot, rows, {})
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))                  # the same bytes on every call
    w, pri, state, top = _priority(weight, slot, rows, {}, max_priority=None, outs=False)
    assert pri is None and state is None and top is None
    assert torch.equal(_bits(w), _bits(a[0]))
    # the running maximum only rises
    assert float(_priority(weight, slot, rows, {}, max_priority=300.0)[3]) == 300.0


def test_priority_purity():
    """The same rows embedded in a larger batch (in front, behind, interleaved with rows of other
    slots) give the same per-slot result: the winners are unchanged."""
    rng = np.random.default_rng(31)
    slot, rows = P.mixed_rows(rng, 65, 30)
    weight = _ring_weight(100, 7)
    alone = _priority(weight, slot, rows, {})
    other_slot, other_rows = P.mixed_rows(rng, 500, 60)
    other_slot = np.where(other_slot >= 0, other_slot + 40, other_slot).astype(np.int32)   # 40 ..
    for at in (0, 500, None):
        if at is None:                                          # interleaved, order kept
            pos = np.sort(rng.choice(565, 65, replace=False))
        else:
            pos = np.arange(at, at + 65)
        big_slot, big_rows = np.empty(565, np.int32), np.empty((565, 3))
        mask = np.zeros(565, bool)
        mask[pos] = True
        big_slot[mask], big_rows[mask] = slot, rows
        big_slot[~mask], big_rows[~mask] = other_slot, other_rows
        got = _priority(weight, big_slot, big_rows, {})
        assert torch.equal(_bits(got[0][:40]), _bits(alone[0][:40])), at
        m = _cuda(mask)
        assert torch.equal(_bits(got[1][m]), _bits(alone[1])), at
        assert torch.equal(got[2][m], alone[2]), at
        _same_priority(weight, big_slot, big_rows)


# ---------------------------------------------------------------- rvz_replay_is_weight
@pytest.mark.parametrize("beta", [0.0, 0.4, 1.0])
@pytest.mark.parametrize("nb", NBS + (1025,))
def test_is_weight(nb, beta):
    """1,025 rows: the one workgroup of the minimum takes a second stride."""
    rng = np.random.default_rng(nb)
    slot = rng.integers(0, 1000, nb).astype(np.int32)
    slot[rng.integers(0, 8, nb) == 0] = -1
    prob = P.mixed_probs(rng, nb, slot)
    if nb == 1:
        slot[0], prob[0] = 3, 0.25
    want = _same_is_weight(prob, slot, beta)
    valid = want[0] > 0
    assert valid.any() and float(want[0].max()) == 1.0
    if nb > 1:
        assert (~valid).any()
    if beta == 0.0:
        assert set(want[0][valid].tolist()) == {1.0}


def test_is_weight_edges():
    nan, inf = float("nan"), float("inf")
    # no valid row: every weight and the minimum are 0
    want = _same_is_weight([0.0, nan, 0.5, inf, -1.0], [0, 0, -1, 3, 2], 0.4)
    assert not want[0].any() and want[1] == 0
    # the minimum where it sits: first, last, behind a workgroup's stride, on an invalid slot
    for nb, at in ((300, 0), (300, 299), (2049, 2048), (2049, 1024)):
        prob = np.random.default_rng(nb + at).uniform(0.01, 1, nb).astype(np.float32)
        slot = np.arange(nb, dtype=np.int32)
        prob[at] = 1e-3
        prob[(at + 7) % nb], slot[(at + 7) % nb] = 1e-5, -1     # smaller, but not a drawn row
        want = _same_is_weight(prob, slot, 0.7)
        assert want[1] == np.float32(1e-3) and want[0][at] == 1.0
    # subnormal and huge ratios
    _same_is_weight(np.array([1e-42, 1.0, 3e-39, 0.5], np.float32), [1, 2, 3, 4], 1.0)
    out, pmin = _is_weight([0.5, 0.25], [0, 1], 0.5, with_min=False)    # out_min_prob is nullable
    assert pmin is None and out.tolist() == [float(np.float32(P.pow_cr(0.5, 0.5))), 1.0]
    a, b = _is_weight([0.5, 0.3, 0.9], [0, 1, 2], 0.4), _is_weight([0.5, 0.3, 0.9], [0, 1, 2], 0.4)
    assert torch.equal(_bits(a[0]), _bits(b[0]))


def test_is_weight_purity():
    """A row's weight depends on its probability and the batch's minimum alone."""
    rng = np.random.default_rng(41)
    prob = rng.uniform(0.01, 1, 65).astype(np.float32)
    slot = np.arange(65, dtype=np.int32)
    alone = _is_weight(prob, slot, 0.4)[0]
    more = rng.uniform(float(prob.min()), 1, 1000).astype(np.float32)   # none below the minimum
    big = _is_weight(np.concatenate([more[:300], prob, more[300:]]),
                     np.concatenate([np.zeros(300, np.int32), slot, np.zeros(700, np.int32)]),
                     0.4)[0]
    assert torch.equal(_bits(big[300:365]), _bits(alone))


# ---------------------------------------------------------------- with the draw, the loss, a graph
def _logits(bs, nb, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(nb, bs * bs + 1, generator=g).cuda(),
            torch.tanh(torch.randn(nb, generator=g)).cuda())


@pytest.mark.parametrize("bs", [8, 6])
def test_slots_of_a_real_draw(bs):
    import rvz
    cap, start, live, nb = 300, 250, 280, 257
    host, dev = _ring(bs, cap, 3)
    w0 = np.random.default_rng(bs).uniform(0.01, 4, cap).astype(np.float32)
    weight = _cuda(w0)
    table = rvz.replay_cdf(weight, start, live)
    out = rvz.replay_batch_weighted(*dev, table, start, live, nb, 5, 9, board_size=bs)
    slot, prob = out[3].cpu().numpy(), out[5].cpu().numpy()
    ref = W.batch(*host, W.cdf(w0, start, live), start, live, nb, 5, 9, True, None, None, None, bs)
    assert np.array_equal(slot, ref[3]) and len(set(slot.tolist())) < nb     # duplicates
    isw, pmin = rvz.replay_is_weight(out[5], out[3], 0.4, with_min=True)
    want = P.is_weight(prob, slot, 0.4)
    assert torch.equal(_bits(isw), _bits(_cuda(want[0]))) and float(pmin) == float(want[1])
    z, y = _logits(bs, nb, 1)
    loss = rvz.policy_value_loss(z, y, out[1], out[2], isw, board_size=bs, rows=True, grads=False)
    top = torch.ones(1, device="cuda")
    pri, state = rvz.replay_priority(weight, out[3], loss["rows"], 1.0, 0.5, max_priority=top)
    want = P.priority(w0, slot, loss["rows"].cpu().numpy(), 1.0, 0.5, max_priority=1.0)
    for g, x in zip((weight, pri, state, top), want):
        assert torch.equal(_bits(g), _bits(_cuda(np.atleast_1d(x))))
    assert set(want[2].tolist()) == {0, 1}


def test_graph_capture_of_the_whole_step():
    """sample, is_weight, loss on fixed logits, priority, cdf: captured on one stream, replayed,
    equal to the eager bytes; a second replay continues from the first's weights."""
    import rvz
    bs, cap, start, live, nb = 8, 300, 250, 280, 257
    _, dev = _ring(bs, cap, 3)
    w0 = _cuda(np.random.default_rng(1).uniform(0.01, 4, cap).astype(np.float32))
    z, y = _logits(bs, nb, 2)

    def step(weight, table, top):
        out = rvz.replay_batch_weighted(*dev, table, start, live, nb, 5, 9, board_size=bs)
        isw = rvz.replay_is_weight(out[5], out[3], 0.4)
        loss = rvz.policy_value_loss(z, y, out[1], out[2], isw, board_size=bs, rows=True,
                                     grads=False)
        pri, state = rvz.replay_priority(weight, out[3], loss["rows"], max_priority=top)
        rvz.replay_cdf(weight, start, live, out=table)
        return out[3], isw, pri, state

    def fresh():
        weight = w0.clone()
        return weight, rvz.replay_cdf(weight, start, live), torch.ones(1, device="cuda")

    eager = []
    weight, table, top = fresh()
    for _ in range(2):
        outs = step(weight, table, top)
        eager.append([t.clone() for t in outs + (weight, table[:4 + live], top)])
    torch.cuda.synchronize()
    weight, table, top = fresh()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(weight, table, top)
    for want in eager:
        graph.replay()
        torch.cuda.synchronize()
        for g, x in zip(outs + (weight, table[:4 + live], top), want):
            assert torch.equal(_bits(g), _bits(x))
    assert not torch.equal(eager[0][0], eager[1][0])            # the second draw saw new weights


# ---------------------------------------------------------------- the Python layers
@pytest.mark.parametrize("bs", [8, 6])
def test_prioritized_replay_buffer_on_the_device(bs):
    import rvz
    kw = dict(prioritized=True, recency_decay=0.75, priority_alpha=0.5, priority_floor=2.0 ** -6)
    gpu = rvz.ReplayBuffer(300, bs, "cuda", **kw)
    cpu = rvz.ReplayBuffer(300, bs, "cpu", weighted_batcher=W.weighted_batcher,
                           cdf_builder=W.cdf_builder, priority_updater=P.priority_updater,
                           is_weighter=P.is_weighter, **kw)
    assert gpu.priority_updater is rvz.replay_priority and gpu.is_weighter is rvz.replay_is_weight
    assert gpu._max_priority.is_cuda and gpu.max_priority() == 1.0
    for it, rows in _appends(bs):
        gpu.append(*[t.cuda() for t in rows], it)
        cpu.append(*rows, it)
        assert torch.equal(_bits(gpu.weight.cpu()), _bits(cpu.weight))
        for step in (0, 1):
            g = gpu.sample(100, 3, step, with_prob=True)
            c = cpu.sample(100, 3, step, with_prob=True)
            assert torch.equal(g[3].cpu(), c[3]) and torch.equal(_bits(g[5].cpu()), _bits(c[5]))
            wg, wc = gpu.is_weights(g[5], g[3], 0.4), cpu.is_weights(c[5], c[3], 0.4)
            assert torch.equal(_bits(wg.cpu()), _bits(wc))
            z, y = _logits(bs, 100, 10 * it + step)
            loss = rvz.policy_value_loss(z, y, g[1], g[2], wg, board_size=bs, rows=True,
                                         grads=False)
            rows64 = loss["rows"]
            if step:
                rows64 = rows64.clone()
                rows64[5] = float("nan")
            pg, sg = gpu.update_priorities(g[3], rows64, 1.0, 2.0)
            pc, sc = cpu.update_priorities(c[3], rows64.cpu(), 1.0, 2.0)
            assert torch.equal(_bits(pg.cpu()), _bits(pc)) and torch.equal(sg.cpu(), sc)
            assert torch.equal(_bits(gpu.weight.cpu()), _bits(cpu.weight))
            assert gpu._dirty and gpu.max_priority() == cpu.max_priority()
            assert set(sg.tolist()) >= {0, 1}
        assert gpu.total_weight() == cpu.total_weight() and gpu.invalid_weights() == 0
    assert gpu.max_priority() > 1.0 and len(gpu) == 300
    held = gpu.weight.cpu()
    assert float(held.min()) >= 2.0 ** -6 * 0.75 ** 2 and float(held.max()) <= 2.0 ** 8


def _synthetic(bs, n, seed):
    host = _ring(bs, n, seed)[0]
    return (torch.from_numpy(host[0].view(np.int64)).cuda(),
            torch.from_numpy(host[1].view(np.int64)).cuda(), torch.from_numpy(host[2]).cuda(),
            torch.from_numpy(host[3]).cuda().clamp(-1, 1))


def test_train_replay_prioritized_on_the_device():
    """Three steps on a 1x64 6x6 net: structure only (the convolutions' backward kernels are not
    reproducible from run to run)."""
    import rvz
    from rvz.trainer import DDPTrainer
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(6, 1, 64).cuda()
    buf = rvz.ReplayBuffer(256, 6, "cuda", prioritized=True)
    buf.append(*_synthetic(6, 200, 1), 0)
    before = buf.weight.clone()
    seen = []
    update = buf.update_priorities

    def spy(slot, rows, *a):
        out = update(slot, rows, *a)
        seen.append((slot.clone(), out[0].clone(), out[1].clone(), a))
        return out
    buf.update_priorities = spy
    tr = DDPTrainer(net, policy_target="full", batch_size=32, value_loss_weight=0.5)
    out = tr.train_replay(buf, 3, seed=2, priority_beta=0.6)
    assert out["steps"] == 3 and len(seen) == 3 and all(x[3] == (1.0, 0.5) for x in seen)
    for key in ("train/loss", "train/policy_kl", "train/is_weight_mean", "train/priority_mean"):
        assert np.isfinite(out[key]), key
    assert 0 < out["train/is_weight_mean"] <= 1
    assert 2.0 ** -8 <= out["train/priority_mean"] <= 2.0 ** 8
    won = torch.cat([slot[state == 1] for slot, _, state, _ in seen]).unique().long()
    changed = torch.nonzero(_bits(buf.weight) != _bits(before)).reshape(-1)
    assert len(won) and set(changed.tolist()) <= set(won.tolist()) <= set(range(200))
    assert len(changed) >= len(won) - 3                         # a priority of exactly 1 is rare
    new = buf.weight[won]
    assert bool(torch.isfinite(new).all()) and float(new.min()) >= 2.0 ** -8
    assert float(new.max()) <= 2.0 ** 8
    last_slot, last_pri, last_state, _ = seen[-1]
    w = last_state == 1
    assert torch.equal(buf.weight[last_slot[w].long()], last_pri[w])
    assert buf.max_priority() == max(1.0, max(float(x[1].max()) for x in seen))
    assert buf.invalid_weights() == 0 and buf.total_weight() > 0
    with pytest.raises(ValueError):
        DDPTrainer(net, batch_size=32).train_replay(buf, 1)


def test_selfplay_trainer_samples_by_priority():
    """6x6, a one-block 64-filter net, 8 games, a two-batch search: two iterations with a window
    of two, sampled by priority (the size of test_selfplay_trainer_samples_by_counts)."""
    import rvz
    from rvz.pipeline import SelfPlayTrainer
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(6, 1, 64).cuda()
    spt = SelfPlayTrainer(net, games=8, num_simulations=32, batch_size=16, seed=0, train_batch=16,
                          train_steps=2, replay_iterations=2, merge_positions=True,
                          replay_sampling="priority", replay_priority_alpha=0.5,
                          replay_priority_beta=(0.4, 1.0, 2), policy_target="full")
    assert spt.buffer.prioritized and spt.buffer.priority_alpha == 0.5
    assert [spt.priority_beta(i) for i in range(3)] == [0.4, 0.7, 1.0]
    rs = [spt.run_iteration() for _ in range(2)]
    for r in rs:
        assert set(r) >= PARENT_KEYS | {"replay_rows", "replay_iterations_held",
                                        "replay_priority_max", "train/is_weight_mean",
                                        "train/priority_mean", "train/policy_kl"}
        assert r["steps"] == 2 and np.isfinite(r["train/loss"])
        assert 0 < r["train/is_weight_mean"] <= 1
        assert 2.0 ** -8 <= r["train/priority_mean"] <= r["replay_priority_max"] <= 2.0 ** 8
    assert 1.0 <= rs[0]["replay_priority_max"] <= rs[1]["replay_priority_max"]
    n0, n1 = rs[0]["samples"], rs[1]["samples"]
    held = spt.buffer.weight[:n0 + n1]
    assert len(spt.buffer) == n0 + n1 and spt.buffer.invalid_weights() == 0
    assert float(held.min()) >= 2.0 ** -8 and float(held.max()) <= 2.0 ** 8
    # iteration 1's rows entered at iteration 0's maximum; at most 2 x 16 of them were rewritten
    entered = (held[n0:] == np.float32(rs[0]["replay_priority_max"])).sum().item()
    assert n1 - 32 <= entered <= n1
    assert 1 <= (spt.buffer.weight[:n0 + n1] != 1.0).sum().item()
