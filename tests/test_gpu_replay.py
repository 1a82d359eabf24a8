"""The replay buffer on the GPU: rvz_replay_batch against rvz_training_rows on the gathered records
and against the NumPy reference (tests/replay_ref.py: Philox restated on Python integers, the rows
through tests/symmetry_ref.py), bit for bit; the draw for extreme seeds and steps, purity, bad
rows, argument errors, graph capture, ReplayBuffer on the device against the CPU-tensor buffer,
DDPTrainer.train_replay and SelfPlayTrainer(replay_iterations=...) end to end. Outputs are
pre-filled with NaN / a sentinel before every raw call, so a comparison also shows that every
element was written. Floats are compared as bit patterns."""
import numpy as np
import pytest
import torch

import replay_ref as RR
import symmetry_ref as S

pytestmark = pytest.mark.gpu

EINVAL = -22
SENTINEL = -77
NAMES = ("states", "policy", "value", "slot", "sym")
EXTREMES = (0, 1, 2 ** 32, 2 ** 64 - 1)


def _ring(bs, capacity, first=0, odd_values=False):
    """(host arrays, device tensors) of a ring filled from the shared set. odd_values: slots 0 to
    3 hold -0.0, a denormal, a NaN with a payload and the largest float, which only a bit-for-bit
    move keeps."""
    host = list(RR.ring(bs, capacity, first))
    if odd_values:
        host[3][:4] = np.array([0x80000000, 0x00012345, 0x7FC12345, 0x7F7FFFFF],
                               np.uint32).view(np.float32)
    dev = (torch.from_numpy(host[0].view(np.int64)).cuda(),
           torch.from_numpy(host[1].view(np.int64)).cuda(),
           torch.from_numpy(host[2]).cuda(), torch.from_numpy(host[3]).cuda())
    return host, dev


def _fresh(bs, nb):
    return (torch.full((nb, 3, bs, bs), float("nan"), device="cuda"),
            torch.full((nb, bs * bs + 1), float("nan"), device="cuda"),
            torch.full((nb,), float("nan"), device="cuda"),
            torch.full((nb,), SENTINEL, dtype=torch.int32, device="cuda"),
            torch.full((nb,), SENTINEL, dtype=torch.int32, device="cuda"))


def _i32(a):
    return None if a is None else torch.from_numpy(np.asarray(a, np.int32)).cuda()


def _raw(bs, dev, start, live, nb, seed=0, step=0, random_sym=1, idx=None, sym=None, stream=None,
         out=None):
    """rvz_replay_batch through the C-ABI on pre-filled outputs; idx / sym device int32 or None."""
    import rvz
    from rvz._lib import ptr
    out = _fresh(bs, nb) if out is None else out
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    rc = rvz.load().rvz_replay_batch(bs, dev[0].numel(), *[ptr(t) for t in dev], start, live, nb,
                                     ptr(idx), ptr(sym), random_sym, seed, step,
                                     *[ptr(t) for t in out], stream)
    assert rc == 0, rc
    return out


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, want, what=""):
    """got: device tensors; want: the reference's arrays (value [nb, 1] or [nb])."""
    for g, x, name in zip(got, want, NAMES):
        x = torch.from_numpy(np.ascontiguousarray(x)).cuda().reshape(g.shape)
        assert g.dtype == x.dtype, (name, what)
        assert torch.equal(_bits(g), _bits(x)), (name, what)


def _by_training_rows(bs, dev, slot, sym):
    """What rvz.training_rows writes for the records gathered from slots `slot` (device int64)."""
    import rvz
    status = torch.zeros(slot.numel(), 4, dtype=torch.int32, device="cuda")
    status[:, 0], status[:, 2] = 1, -1
    states, policy = rvz.training_rows(dev[0][slot], dev[1][slot], status,
                                       dev[2][slot].contiguous(), sym, bs)
    return states, policy, dev[3][slot]


# ---------------------------------------------------------------- given idx and sym
@pytest.mark.parametrize("nb", [1, 3, 5])
@pytest.mark.parametrize("bs", [8, 6])
def test_given_rows_from_a_wrapping_ring(bs, nb):
    """Capacity 7 with start = 5: logical rows 2 .. 6 sit in slots 0 .. 4. Partial blocks of four
    waves."""
    cap, start = 7, 5
    host, dev = _ring(bs, cap, 40, odd_values=True)
    for live in (7, 4):
        rng = np.random.default_rng(10 * nb + live)
        idx = rng.integers(0, live, size=nb).astype(np.int32)
        idx[0] = live - 1                                     # the newest row
        sym = rng.integers(0, 8, size=nb).astype(np.int32)
        got = _raw(bs, dev, start, live, nb, idx=_i32(idx), sym=_i32(sym))
        _same(got, RR.batch(*host, start, live, nb, 0, 0, True, idx, sym, bs), (live, "ref"))
        slot = (start + idx) % cap
        assert got[3].tolist() == slot.tolist() and got[4].tolist() == sym.tolist()
        by_rows = _by_training_rows(bs, dev, torch.from_numpy(slot).cuda().long(), _i32(sym))
        for g, x, name in zip(got, by_rows, NAMES):
            assert torch.equal(_bits(g), _bits(x)), (name, live)


@pytest.mark.parametrize("bs", [8, 6])
def test_given_rows_beyond_one_grid(bs):
    """nb = 8,195: three rows past one pass of the 2,048 blocks x 4 waves (the grid-stride loop),
    through rvz.replay_batch."""
    import rvz
    cap, start, live, nb = 300, 123, 300, 8195
    host, dev = _ring(bs, cap, 7, odd_values=True)
    rng = np.random.default_rng(bs)
    idx = rng.integers(0, live, size=nb).astype(np.int32)
    idx[-3:] = [0, live - 1, 176]                             # slot 299, wrapping
    sym = rng.integers(0, 8, size=nb).astype(np.int32)
    got = rvz.replay_batch(*dev, start, live, nb, 0, 0, idx=_i32(idx), sym=_i32(sym),
                           board_size=bs)
    assert got[2].shape == (nb, 1)
    _same(got, RR.batch(*host, start, live, nb, 0, 0, True, idx, sym, bs))
    slot = torch.from_numpy((start + idx) % cap).cuda().long()
    states, policy, value = _by_training_rows(bs, dev, slot, _i32(sym))
    assert torch.equal(_bits(got[0]), _bits(states)) and torch.equal(_bits(got[1]), _bits(policy))
    assert torch.equal(_bits(got[2].reshape(-1)), _bits(value))
    assert int(got[3][-1]) == 299 and set(got[3].tolist()) == set(range(cap))


# ---------------------------------------------------------------- drawn
@pytest.mark.parametrize("bs", [8, 6])
def test_drawn_rows(bs):
    """The kernel's own draw: seeds and steps in {0, 1, 2^32, 2^64 - 1} (both words of the key
    and of the counter), live in {1, 2, capacity}, with and without random symmetries. Slot and
    symmetry equal the reference's, the rows are the reference's rows of those slots."""
    cap, start, nb = 7, 5, 64
    host, dev = _ring(bs, cap, 40, odd_values=True)
    st8, pol8, _ = S.training_rows(host[0], host[1], np.ones(cap, np.int32), host[2], None, bs,
                                   all_images=True)           # every image of every slot, once
    seen = set()
    for seed in EXTREMES:
        for step in EXTREMES:
            for live in (1, 2, cap):
                for random_sym in (0, 1):
                    idx, sym = RR.draws(seed, step, nb, live, bool(random_sym))
                    slot = ((start + idx) % cap).astype(np.int32)
                    at = 8 * slot + sym
                    got = _raw(bs, dev, start, live, nb, seed, step, random_sym)
                    _same(got, (st8[at], pol8[at], host[3][slot], slot, sym),
                          (seed, step, live, random_sym))
                    assert idx.max() < live and (random_sym or not sym.any())
                    seen.add(got[3].cpu().numpy().tobytes() + got[4].cpu().numpy().tobytes())
    # every (seed, step) pair drew another vector: 16 pairs at live = capacity with symmetries,
    # 16 without, 16 + 16 at live = 2, and the two constant vectors of live = 1
    assert len(seen) >= 16 * 4 + 1
    # through the Python wrapper and the whole reference
    import rvz
    got = rvz.replay_batch(*dev, start, cap, nb, 2 ** 64 - 1, 2 ** 32, board_size=bs)
    _same(got, RR.batch(*host, start, cap, nb, 2 ** 64 - 1, 2 ** 32, True, None, None, bs))
    assert set(got[3].tolist()) == set(range(cap)) and set(got[4].tolist()) == set(range(8))


@pytest.mark.parametrize("bs", [8, 6])
def test_purity(bs):
    cap, start, live = 300, 123, 211
    _, dev = _ring(bs, cap, 7)
    a = _raw(bs, dev, start, live, 200, 5, 9)
    b = _raw(bs, dev, start, live, 200, 5, 9)
    for x, y, name in zip(a, b, NAMES):
        assert torch.equal(_bits(x), _bits(y)), name          # the same call twice
    short = _raw(bs, dev, start, live, 64, 5, 9)
    for x, y, name in zip(a, short, NAMES):
        assert torch.equal(_bits(x[:64]), _bits(y)), name     # a row does not depend on nb
    other = _raw(bs, dev, start, live, 200, 5, 10)
    assert not torch.equal(other[3], a[3]) and not torch.equal(other[4], a[4])
    assert not torch.equal(_raw(bs, dev, start, live, 200, 6, 9)[3], a[3])
    assert int(a[3].min()) >= 0 and int(a[3].max()) < cap
    held = (torch.arange(cap, device="cuda") - start) % cap < live
    assert bool(held[a[3].long()].all())                      # only slots that hold a live row


# ---------------------------------------------------------------- rows that are refused
@pytest.mark.parametrize("bs", [8, 6])
def test_bad_rows(bs):
    """An idx of -1 or live, a sym of 8 or -1: zero rows, their neighbours untouched."""
    cap, start, live, nb = 7, 5, 4, 9
    host, dev = _ring(bs, cap, 40)
    idx = np.array([0, -1, 1, live, 2, 3, 3, -2 ** 31, 2 ** 31 - 1], np.int32)
    sym = np.array([1, 2, 3, 4, 8, 5, -1, 6, 9], np.int32)
    got = _raw(bs, dev, start, live, nb, idx=_i32(idx), sym=_i32(sym))
    _same(got, RR.batch(*host, start, live, nb, 0, 0, True, idx, sym, bs))
    assert got[3].tolist() == [5, -1, 6, -1, 0, 1, 1, -1, -1]
    assert got[4].tolist() == [1, -1, 3, -1, -1, 5, -1, -1, -1]
    bad = torch.tensor([1, 3, 4, 6, 7, 8], device="cuda")
    assert not bool(got[0][bad].any()) and not bool(got[1][bad].any())
    assert not bool(got[2][bad].any())
    fine = torch.tensor([0, 2, 5], device="cuda")
    assert bool(got[0][fine].flatten(1).any(dim=1).all())
    # a given idx with a drawn symmetry, and a drawn row with a given symmetry
    one = _raw(bs, dev, start, live, nb, 3, 4, idx=_i32(idx))
    _same(one, RR.batch(*host, start, live, nb, 3, 4, True, idx, None, bs))
    two = _raw(bs, dev, start, live, nb, 3, 4, sym=_i32(sym))
    _same(two, RR.batch(*host, start, live, nb, 3, 4, True, None, sym, bs))
    assert int((two[4] == -1).sum()) == 3 and int((two[3] == -1).sum()) == 0


def test_einval_through_the_c_abi():
    import rvz
    from rvz._lib import ptr
    lib = rvz.load()
    _, dev = _ring(8, 7)
    out = _fresh(8, 4)
    stream = torch.cuda.current_stream().cuda_stream
    #       0  1  2 .. 5                  6  7  8  9     10    11 12 13 14 .. 18
    good = [8, 7, *[ptr(t) for t in dev], 5, 3, 4, None, None, 1, 0, 0, *[ptr(t) for t in out],
            stream]
    assert lib.rvz_replay_batch(*good) == 0
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(t).any()) for t in out[:3])
    assert int(out[3].min()) >= 0 and int(out[4].min()) >= 0
    for k, v in ((0, 7), (0, 4), (1, 0), (1, -1), (7, 0), (7, 8), (7, -1), (6, -1), (6, 7),
                 (8, -1), (8, 2 ** 31 // 65 + 1), (14, ptr(out[0]) + 4), (14, ptr(out[0]) + 8)):
        args = list(good)
        args[k] = v
        assert lib.rvz_replay_batch(*args) == EINVAL, (k, v)
    args = list(good)
    args[0], args[8] = 6, 2 ** 31 // 37 + 1
    assert lib.rvz_replay_batch(*args) == EINVAL
    for k in (2, 3, 4, 5, 14, 15, 16, 17, 18):
        args = list(good)
        args[k] = None
        assert lib.rvz_replay_batch(*args) == EINVAL, k
    for bs in (8, 6):                                         # nb = 0: no launch, null pointers
        assert lib.rvz_replay_batch(bs, 7, None, None, None, None, 5, 3, 0, None, None, 1, 0, 0,
                                    None, None, None, None, None, stream) == 0
    empty = rvz.replay_batch(*dev, 5, 3, 0, 0, 0)
    assert [tuple(t.shape) for t in empty] == [(0, 3, 8, 8), (0, 65), (0, 1), (0,), (0,)]
    # the Python surface refuses malformed arguments before the library sees them
    m, o, p, v = dev
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    for call in (lambda: rvz.replay_batch(m, o[:3], p, v, 5, 3, 4, 0, 0),
                 lambda: rvz.replay_batch(m.to(torch.int32), o, p, v, 5, 3, 4, 0, 0),
                 lambda: rvz.replay_batch(m, o, p[:, :64], v, 5, 3, 4, 0, 0),
                 lambda: rvz.replay_batch(m, o, p.double(), v, 5, 3, 4, 0, 0),
                 lambda: rvz.replay_batch(m, o, p, v[:3], 5, 3, 4, 0, 0),
                 lambda: rvz.replay_batch(m, o, p, v, 7, 3, 4, 0, 0),
                 lambda: rvz.replay_batch(m, o, p, v, 5, 0, 4, 0, 0),
                 lambda: rvz.replay_batch(m, o, p, v, 5, 8, 4, 0, 0),
                 lambda: rvz.replay_batch(m, o, p, v, 5, 3, -1, 0, 0),
                 lambda: rvz.replay_batch(m, o, p, v, 5, 3, 4, 0.5, 0),
                 lambda: rvz.replay_batch(m, o, p, v, 5, 3, 4, 0, 0, idx=idx[:2]),
                 lambda: rvz.replay_batch(m, o, p, v, 5, 3, 4, 0, 0, sym=idx.float()),
                 lambda: rvz.replay_batch(m, o, p, v, 5, 3, 4, 0, 0, board_size=7)):
        with pytest.raises(rvz.RvzError):
            call()


def test_graph_capture():
    """One captured call replayed: the eager bytes, and the ring's new contents after a change."""
    bs, cap, start, live, nb = 8, 300, 123, 211, 257
    host_a, dev = _ring(bs, cap, 7)
    host_b, other = _ring(bs, cap, 500)
    eager = [t.clone() for t in _raw(bs, dev, start, live, nb, 5, 9)]            # warm
    torch.cuda.synchronize()
    out = tuple(torch.empty_like(t) for t in eager)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _raw(bs, dev, start, live, nb, 5, 9, stream=torch.cuda.current_stream().cuda_stream,
             out=out)
    keep = [t.clone() for t in dev]
    for src, host in ((other, host_b), (keep, host_a)):
        for t, x in zip(dev, src):
            t.copy_(x)
        for t in out[:3]:
            t.fill_(float("nan"))
        for t in out[3:]:
            t.fill_(SENTINEL)
        graph.replay()
        _same(out, RR.batch(*host, start, live, nb, 5, 9, True, None, None, bs))
    for g, x, name in zip(out, eager, NAMES):
        assert torch.equal(_bits(g), _bits(x)), name


# ---------------------------------------------------------------- the Python layers
def _appends(bs):
    """Three iterations of 120, 100 and 130 rows for a ring of 300: the third wraps."""
    out = []
    for it, (lo, hi) in enumerate(((0, 120), (120, 220), (220, 350))):
        host = RR.ring(bs, hi - lo, lo)
        out.append((it, (torch.from_numpy(host[0].view(np.int64)),
                         torch.from_numpy(host[1].view(np.int64)), torch.from_numpy(host[2]),
                         torch.from_numpy(host[3]))))
    return out


@pytest.mark.parametrize("bs", [8, 6])
def test_replay_buffer_on_the_device(bs):
    import rvz
    gpu = rvz.ReplayBuffer(300, bs, "cuda")
    cpu = rvz.ReplayBuffer(300, bs, "cpu", batcher=RR.batcher)
    assert gpu.mover.is_cuda and gpu.batcher is rvz.replay_batch
    with pytest.raises(ValueError):
        gpu.sample(4, 0, 0)
    for it, rows in _appends(bs):
        gpu.append(*[t.cuda() for t in rows], it)
        cpu.append(*rows, it)
        assert len(gpu) == len(cpu) and gpu.start == cpu.start
        assert gpu.rows_by_iteration() == cpu.rows_by_iteration()
        for step in (0, 1):
            _same(gpu.sample(100, 3, step), [t.numpy() for t in cpu.sample(100, 3, step)],
                  (it, step))
    assert len(gpu) == 300 and gpu.start == 50
    assert gpu.rows_by_iteration() == [(0, 70), (1, 100), (2, 130)]
    for a, b in zip((gpu.mover, gpu.opponent, gpu.policy, gpu.value),
                    (cpu.mover, cpu.opponent, cpu.policy, cpu.value)):
        assert torch.equal(a.cpu(), b)
    _same(gpu.sample(64, 4, 0, symmetries=False),
          [t.numpy() for t in cpu.sample(64, 4, 0, symmetries=False)])
    idx = torch.arange(300)
    sym = idx % 8
    _same(gpu.sample(300, 0, 0, idx=idx.cuda(), sym=sym.cuda()),
          [t.numpy() for t in cpu.sample(300, 0, 0, idx=idx, sym=sym)])


def test_train_replay_trains_on_the_buffers_batches():
    import rvz
    from rvz.trainer import DDPTrainer
    bs = 6
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(bs, 1, 64).cuda()
    buf = rvz.ReplayBuffer(300, bs, "cuda")
    for it, rows in _appends(bs):
        buf.append(*[t.cuda() for t in rows], it)
    tr = DDPTrainer(net, batch_size=16)
    seen = []
    step = tr.train_step

    def recording(states, policy, value):
        seen.append((states.clone(), policy.clone(), value.clone()))
        return step(states, policy, value)

    tr.train_step = recording
    out = tr.train_replay(buf, 3, seed=21)
    assert out["steps"] == 3 == len(seen)
    assert set(out) == {"train/loss", "train/policy_loss", "train/value_loss", "train/lr", "steps"}
    for k in ("train/loss", "train/policy_loss", "train/value_loss"):
        assert np.isfinite(out[k]), k
    for s, got in enumerate(seen):
        want = buf.sample(16, 21, s)
        assert got[0].shape == (16, 3, bs, bs) and got[2].shape == (16, 1)
        for g, x in zip(got, want):
            assert torch.equal(_bits(g), _bits(x)), s
    assert not torch.equal(seen[0][0], seen[1][0])
    seen.clear()
    tr.train_replay(buf, 1, seed=21, symmetries=False)
    assert torch.equal(seen[0][0], buf.sample(16, 21, 0, symmetries=False)[0])


PARENT_KEYS = {"train/loss", "train/policy_loss", "train/value_loss", "train/lr", "steps",
               "selfplay_s", "train_s", "board_steps", "samples", "exact_rows", "exact_unsolved",
               "exact_policy_rows", "exact_policy_unsolved", "adjudicated", "adjudicate_unsolved",
               "already_over", "symmetry_rows", "symmetry_quirk_rows", "merge_rows",
               "merge_input_rows"}


def test_selfplay_trainer_with_a_replay_window():
    """6x6, a one-block 64-filter net, 8 games, a two-batch search (32 simulations at batch 16):
    three iterations with a window of two."""
    import copy

    import rvz
    from rvz.pipeline import SelfPlayTrainer
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(6, 1, 64).cuda()
    kw = dict(games=8, num_simulations=32, batch_size=16, seed=0, train_batch=16)
    off = SelfPlayTrainer(copy.deepcopy(net), **kw, train_steps=1)
    assert off.buffer is None and set(off.generate()) == {"states", "policy_targets",
                                                          "value_targets"}
    r = off.run_iteration()
    assert set(r) == PARENT_KEYS | {"replay_rows", "replay_iterations_held"}
    assert r["replay_rows"] == 0 and r["replay_iterations_held"] == 0
    for bad in ("random", "all"):
        with pytest.raises(ValueError):
            SelfPlayTrainer(copy.deepcopy(net), **kw, replay_iterations=2, symmetries=bad)
    init = {k: v.clone() for k, v in net.state_dict().items()}
    spt = SelfPlayTrainer(net, **kw, replay_iterations=2)
    assert spt.buffer.capacity == 2 * 8 * 32 and spt.buffer.window_iterations == 2
    data = spt.generate()
    assert set(data) == {"mover", "opponent", "policy_targets", "value_targets"}
    assert len(spt.buffer) == 0                               # generate() alone appends nothing
    rs = [spt.run_iteration() for _ in range(3)]
    for i, r in enumerate(rs):
        assert set(r) == set(rs[0]) == PARENT_KEYS | {"replay_rows", "replay_iterations_held"}
        assert 8 * 8 < r["samples"] <= 8 * 32
        assert r["steps"] == -(-r["samples"] // 16)           # a pass over the new rows
        assert r["replay_iterations_held"] == min(i + 1, 2)
        assert np.isfinite(r["train/loss"])
    assert rs[0]["replay_rows"] == rs[0]["samples"]
    assert rs[1]["replay_rows"] == rs[0]["samples"] + rs[1]["samples"]
    assert rs[2]["replay_rows"] == rs[1]["samples"] + rs[2]["samples"] == len(spt.buffer)
    # the first iteration's rows are gone
    assert spt.buffer.rows_by_iteration() == [(1, rs[1]["samples"]), (2, rs[2]["samples"])]
    assert spt.buffer.start == rs[0]["samples"]
    moved = max((net.state_dict()[k].float() - init[k].float()).abs().max().item()
                for k in init if init[k].is_floating_point())
    assert moved > 0
    # replay_steps and train_steps
    spt.replay_steps, spt.train_steps = 5, None
    assert spt.run_iteration()["steps"] == 5
    spt.train_steps = 2
    assert spt.run_iteration()["steps"] == 2
