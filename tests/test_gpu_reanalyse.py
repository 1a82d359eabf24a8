"""Replay reanalysis on the device: rvz_replay_stale, rvz_replay_roots and rvz_replay_refresh
against the NumPy restatement (tests/reanalyse_ref.py) bit for bit at the shapes where the kernels
can go wrong, ReplayBuffer.reanalyse end to end against a plain Python loop over the same engine,
and SelfPlayTrainer(reanalyse_rows=...)."""
import numpy as np
import pytest
import torch

import reanalyse_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -77
TILE = 1024                      # the compaction tile of rvz_replay_stale


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stale(stamp, start, live, n, lo, below):
    """rvz_replay_stale through the C-ABI on pre-filled outputs and a dirty scratch."""
    import rvz
    lib = rvz.load()
    st = _cuda(np.asarray(stamp, np.int32))
    size = lib.rvz_replay_stale_scratch_size(len(stamp), below - lo)
    scratch = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    slot = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    count = torch.full((2,), SENTINEL, dtype=torch.int32, device="cuda")
    rc = lib.rvz_replay_stale(len(stamp), st.data_ptr(), start, live, n, lo, below,
                              scratch.data_ptr(), size, slot.data_ptr(), count.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return slot.cpu().numpy(), count.cpu().numpy()


def _same_stale(stamp, start, live, n, lo, below):
    want = R.stale(stamp, start, live, n, lo, below)
    if n == 0:                                   # no launch: nothing is written
        import rvz
        slot, count = rvz.replay_stale(_cuda(np.asarray(stamp, np.int32)), start, live, 0, lo,
                                       below)
        assert slot.shape == (0,) and count.tolist() == [0, 0]
        return want
    got = _stale(stamp, start, live, n, lo, below)
    assert got[0].dtype == np.int32 and got[0].tolist() == want[0].tolist(), (n, lo, below)
    assert got[1].tolist() == want[1].tolist(), (n, lo, below)
    again = _stale(stamp, start, live, n, lo, below)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()
    return want


CAP, START, LIVE = 64, 50, 40    # the live rows wrap: slots 50 .. 63, 0 .. 25


def _patterns():
    """name -> (stamp [CAP], lo, below); slots 26 .. 49 hold no row and must never be read: they
    carry stamps that would be selected first, and a negative one."""
    rng = np.random.default_rng(3)
    dead = np.arange(26, 50)
    out = {}
    s = np.full(CAP, 3, np.int32)
    out["equal"] = (s, 0, 5)
    s = rng.integers(5, 9, CAP).astype(np.int32)
    out["none eligible"] = (s, 2, 5)
    s = rng.integers(0, 6, CAP).astype(np.int32)                # 0 .. 3 share class 0
    out["below lo"] = (s, 3, 6)
    s = rng.integers(0, 7, CAP).astype(np.int32)
    s[60] = -3
    s[7] = -2 ** 31
    out["out of range"] = (s, 1, 6)
    s = rng.integers(0, 70000, CAP).astype(np.int32)
    out["wide"] = (s, 100, 100 + 65536)
    for stamp, lo, _ in out.values():
        stamp[dead] = lo
        stamp[30] = -1
    return out


@pytest.mark.parametrize("name", list(_patterns()))
def test_stale_on_a_wrapped_ring(name):
    stamp, lo, below = _patterns()[name]
    counts = [_same_stale(stamp, START, LIVE, n, lo, below)[1].tolist() for n in (0, 1, 7, 40, 64)]
    if name == "equal":
        assert counts == [[0, 0], [1, 0], [7, 0], [40, 0], [40, 0]]
    if name == "none eligible":
        assert all(c == [0, 0] for c in counts)
    if name == "out of range":
        assert counts[-1][1] == 2 and counts[-1][0] <= 38


@pytest.mark.parametrize("tiles", (1, 3))
def test_stale_ties_across_tile_boundaries(tiles):
    """A ring of `tiles` compaction tiles and one row: a run of threshold-class rows lies across
    every tile boundary (and the ring's end), and n cuts inside each run, at its ends and right
    at a boundary, so the rank carried from tile to tile decides which rows are taken."""
    cap = tiles * TILE + 1
    start = 7                                    # logical row i in slot (7 + i) % cap
    rng = np.random.default_rng(tiles)
    logical = rng.choice(np.array([2, 3, 4, 9], np.int32), cap)  # above the threshold class, or out
    early = rng.choice(cap, 10, replace=False)
    logical[early] = 0
    run = np.zeros(cap, bool)
    for k in range(1, tiles + 1):
        run[k * TILE - 3:k * TILE + 3] = True
    run[early] = False
    logical[run] = 1
    stamp = np.empty(cap, np.int32)
    stamp[(start + np.arange(cap)) % cap] = logical
    runs = int(run.sum())
    at_boundary = 10 + int(run[:TILE].sum())     # the last row taken is the tile's last row
    ns = sorted({1, 10, 11, at_boundary - 1, at_boundary, at_boundary + 1, 10 + runs - 1,
                 10 + runs, 10 + runs + 1, cap, cap + 5})
    for n in ns:
        want, count = _same_stale(stamp, start, cap, n, 0, 5)
        assert count[0] == min(n, int((logical < 5).sum()))
    # the same rows behind a shorter live range that ends inside the first run
    _same_stale(stamp, start, TILE - 1, 10 + 2, 0, 5)
    _same_stale(stamp, start, TILE, 10 + 2, 0, 5)


def _positions(bs, n):
    """n real positions of the engine's own rules as (mover, opponent) int64 device tensors."""
    import rvz
    o = rvz.openings(bs, 4)
    b, w, side = o["black"][:n], o["white"][:n], o["status"][:n, 0]
    assert b.numel() == n
    return torch.where(side == 1, b, w).contiguous(), torch.where(side == 1, w, b).contiguous()


@pytest.mark.parametrize("bs", (6, 8))
def test_roots(bs):
    import rvz
    cap = 12
    mover, opponent = _positions(bs, cap)
    opponent[5] |= mover[5] & -mover[5]                         # one square held by both
    slot = torch.tensor([3, -1, 0, cap, 5, -5, 11, 2], dtype=torch.int32, device="cuda")
    b, w, st, bad = rvz.replay_roots(mover, opponent, slot, bs)
    want = R.roots(mover.cpu().numpy(), opponent.cpu().numpy(), slot.tolist(), bs)
    assert b.cpu().numpy().view(np.uint64).tolist() == want[0].tolist()
    assert w.cpu().numpy().view(np.uint64).tolist() == want[1].tolist()
    assert st.dtype == torch.int32 and st.cpu().numpy().tolist() == want[2].tolist()
    assert bad.tolist() == want[3].tolist() == [3]
    assert st[:, 1].tolist() == [0, 1, 0, 1, 1, 1, 0, 0]
    eng = rvz.Engine(8, num_simulations=8, batch_size=8, board_size=bs)
    eng.set_state(b, w, st)
    gb, gw, gs = eng.get_state()
    assert torch.equal(gb, b) and torch.equal(gw, w) and torch.equal(gs, st)
    legal = eng.legal()
    assert torch.equal(legal, rvz.board_legal(b, w, st, bs))
    live = st[:, 1] == 0
    assert bool((legal[live] != 0).all())
    # the mover is black: the same mask as the position's own legal mask for its mover
    side1 = torch.tensor([[1, 0, -1, 0]] * 4, dtype=torch.int32, device="cuda")
    assert torch.equal(legal[live], rvz.board_legal(mover[[3, 0, 11, 2]].contiguous(),
                                                    opponent[[3, 0, 11, 2]].contiguous(), side1,
                                                    bs))
    # and a second call on the same inputs gives the same bytes
    again = rvz.replay_roots(mover, opponent, slot, bs)
    assert all(torch.equal(x, y) for x, y in zip((b, w, st, bad), again))


def _p_rows(n, npol, seed):
    rng = np.random.default_rng(seed)
    visits = rng.integers(0, 50, (n, npol)).astype(np.float64)
    visits[:, rng.integers(0, npol)] += 1
    return visits / visits.sum(1, keepdims=True)


def _refresh(policy, stamp, slot, p, idx, new_stamp):
    import rvz
    pol, st = _cuda(policy), _cuda(stamp)
    counts = rvz.replay_refresh(pol, st, _cuda(np.asarray(slot, np.int32)), _cuda(p),
                                _cuda(np.asarray(idx, np.int32)), new_stamp)
    return pol.cpu().numpy(), st.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("bs", (6, 8))
def test_refresh(bs):
    npol, cap, n = bs * bs + 1, 40, 16
    rng = np.random.default_rng(bs)
    policy = rng.random((cap, npol)).astype(np.float32)
    policy[0, :2] = np.array([0x7FC12345, 0x80000000], np.uint32).view(np.float32)
    stamp = rng.integers(0, 3, cap).astype(np.int32)
    p = _p_rows(n, npol, bs)
    slot = [4, -1, 9, 17, 9, 22, 30, 31, 9, 39, 0, 12, cap, 13, -3, 5]
    idx = [3] * n
    idx[3] = -2                                  # the engine treated the game as over
    idx[15] = npol - 1                           # the pass
    p[5, 2] = np.nan
    p[6, 1], p[6, 2] = p[6, 1] + p[6, 2] + 0.25, -0.25          # sums to 1, one entry negative
    p[7, npol - 1] += 1e-6                       # the sum is off (in the last entry)
    p[9, 0] = np.inf
    p[11] = p[11] * (1 + 1e-12)                  # within 1e-9 of 1: written
    assert not R.skipped(cap, 12, p[11], 0) and R.skipped(cap, 31, p[7], 0)
    want = R.refresh(policy, stamp, slot, p, idx, 9)
    got = _refresh(policy, stamp, slot, p, idx, 9)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tolist() == want[1].tolist()
    assert got[2].tolist() == want[2].tolist() == [6, 8]
    written = [4, 9, 0, 12, 13, 5]
    assert np.flatnonzero(got[1] != stamp).tolist() == sorted(written)     # no old stamp is 9
    keep = np.setdiff1d(np.arange(cap), written)
    assert got[0][keep].tobytes() == policy[keep].tobytes()
    assert got[1][keep].tolist() == stamp[keep].tolist()
    assert got[0][9].tobytes() == p[8].astype(np.float32).tobytes()        # the last of three
    assert got[0][5].tobytes() == p[15].astype(np.float32).tobytes()
    # another order of the rows with the same last occurrence of every slot: the same ring
    order = [4, 2, 0, 1, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 8, 15]
    assert order.index(8) > max(order.index(2), order.index(4))
    again = _refresh(policy, stamp, [slot[r] for r in order], p[order], [idx[r] for r in order], 9)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tolist() == got[1].tolist()
    assert again[2].tolist() == [6, 8]
    # a batch of more rows than the ring has slots: every slot many times, the last row wins
    n = 5 * cap + 3
    slot = rng.integers(0, cap, n)
    p = _p_rows(n, npol, 77)
    want = R.refresh(policy, stamp, slot, p, [0] * n, 4)
    got = _refresh(policy, stamp, slot, p, [0] * n, 4)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tolist() == want[1].tolist()
    assert got[2].tolist() == want[2].tolist() and got[2][1] == 0 and got[2][0] > cap // 2


@pytest.fixture(scope="module")
def played():
    """An 8x8 1x64 net through LeafEvaluator, an 8-game engine at 200 simulations (fewer give
    one-hot policies) and 24 ring rows from three plies of its self-play, stamped 0 .. 2. At this
    search size a re-search finds the played policy again bit for bit, with this net or another
    (four batches: the visits are decided by the batches' virtual losses), so the ring holds each
    policy row rolled by one square: a target that is visibly stale and still sums to 1."""
    import rvz
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(8, 1, 64).cuda().eval()
    ev = rvz.LeafEvaluator(net)
    eng = rvz.Engine(8, num_simulations=200, batch_size=64)
    eng.reset(list(range(2000, 2008)))
    rows = []
    for ply in range(3):
        b, w, st = (t.clone() for t in eng.get_state())
        eng.search(ev)
        idx, p = eng.act(1.0, apply=True)
        black = st[:, 0] == 1
        rows.append((torch.where(black, b, w), torch.where(black, w, b), p.float().roll(1, 1),
                     torch.where(black, 1.0, -1.0).float(), ply))
    eng.check()
    return ev, eng, rows


def _ring(rows):
    import rvz
    buf = rvz.ReplayBuffer(24, 8, "cuda", stamps=True)
    for mover, opponent, policy, value, ply in rows:
        buf.append(mover, opponent, policy, value, iteration=ply, stamp=ply)
    return buf


def test_reanalyse_end_to_end(played):
    import rvz
    ev, eng, rows = played
    buf = _ring(rows)
    before = {k: getattr(buf, k).clone() for k in ("mover", "opponent", "policy", "value", "stamp")}
    want_slot, want_count = R.stale(before["stamp"].cpu().numpy(), buf.start, len(buf), 12, 0, 2)
    assert want_count.tolist() == [12, 0] and want_slot.tolist() == list(range(12))

    # the plain loop: torch indexing, the engine, .float() and an indexed assignment
    policy, stamp = before["policy"].clone(), before["stamp"].clone()
    u = torch.full((8,), 0.5, dtype=torch.float64, device="cuda")
    for at in (0, 8):
        sl = torch.tensor(want_slot[at:at + 8].tolist(), dtype=torch.int64, device="cuda")
        k = sl.numel()
        b = torch.zeros(8, dtype=torch.int64, device="cuda")
        w = torch.zeros(8, dtype=torch.int64, device="cuda")
        st = torch.tensor([R.OVER_ROW] * 8, dtype=torch.int32, device="cuda")
        b[:k], w[:k] = before["mover"][sl], before["opponent"][sl]
        st[:k] = torch.tensor(R.LIVE_ROW, dtype=torch.int32, device="cuda")
        eng.set_state(b, w, st)
        eng.search(ev)
        idx, p = eng.act(1.0, u=u, apply=False)
        assert idx[:k].min().item() >= 0 and (idx[k:] == -2).all()
        policy[sl] = p[:k].float()
        stamp[sl] = 5
    eng.check()
    changed = (policy != before["policy"]).any(1)
    assert changed.tolist() == [True] * 12 + [False] * 12       # every refreshed row moved

    out = buf.reanalyse(eng, ev, rows=12, lo=0, below=2, new_stamp=5, with_old=True)
    eng.check()
    assert out["slot"].tolist() == want_slot.tolist() and out["selected"].tolist() == [12, 0]
    assert out["counts"].tolist() == [12, 4] and out["bad"].tolist() == [0]
    assert torch.equal(out["old_policy"].view(torch.int32), before["policy"][:12].view(torch.int32))
    assert torch.equal(buf.policy.view(torch.int32), policy.view(torch.int32))
    assert torch.equal(buf.stamp, stamp) and stamp.tolist() == [5] * 12 + [1] * 4 + [2] * 8
    for k in ("mover", "opponent", "value"):
        assert torch.equal(getattr(buf, k).view(torch.int32), before[k].view(torch.int32)), k
    sums = buf.policy[:12].double().sum(1)
    assert float((sums - 1).abs().max()) < 1e-6

    # the evaluator's rows do not depend on their batch: neither does the result on the chunks
    buf4 = _ring(rows)
    eng4 = rvz.Engine(4, num_simulations=200, batch_size=64)
    out4 = buf4.reanalyse(eng4, ev, rows=12, lo=0, below=2, new_stamp=5)
    eng4.check()
    assert out4["slot"].tolist() == want_slot.tolist() and out4["counts"].tolist() == [12, 0]
    assert torch.equal(buf4.policy.view(torch.int32), policy.view(torch.int32))
    assert torch.equal(buf4.stamp, stamp)

    # refusals that need an engine (a fresh one: eng4 is still inside its last search)
    other = rvz.Engine(4, num_simulations=8, batch_size=8)
    other.temperature_schedule(10, 0.0)
    with pytest.raises(ValueError, match="schedule"):
        buf4.reanalyse(other, ev, 4, 0, 2, 6)
    other.temperature_schedule(None)
    other.root_noise(0.3, 0.25)
    with pytest.raises(ValueError, match="noise"):
        buf4.reanalyse(other, ev, 4, 0, 2, 6)
    assert torch.equal(buf4.stamp, stamp)


def test_selfplay_trainer_reanalyses():
    """6x6, a one-block 64-filter net, 8 games, a two-batch search: four iterations with a window
    of three. A refreshed row must still be held when the next iteration trains: the rows the
    next append drops are left out of the selection."""
    import rvz
    from rvz.pipeline import SelfPlayTrainer
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(6, 1, 64).cuda()
    spt = SelfPlayTrainer(net, games=8, num_simulations=32, batch_size=16, seed=0, train_batch=16,
                          train_steps=2, replay_iterations=3, reanalyse_rows=8, reanalyse_age=1)
    buf = spt.buffer
    assert buf.stamps
    rs, ns = [], []
    for t in range(4):
        if t == 3:
            # what iteration 2 refreshed (stamp 2 on rows that iteration 1 played) ...
            refreshed = [(int(buf.mover[s]), int(buf.opponent[s]))
                         for s in range(ns[0], ns[0] + 8)]
            assert buf.stamp[ns[0]:ns[0] + 8].tolist() == [2] * 8
        rs.append(spt.run_iteration())
        ns.append(rs[-1]["samples"])
        r = rs[-1]
        assert {"reanalyse/rows", "reanalyse/skipped", "reanalyse/policy_kl",
                "reanalyse_s"} <= set(r)
        assert r["reanalyse_s"] >= 0 and r["train_s"] >= 0 and np.isfinite(r["train/loss"])
        assert r["reanalyse/skipped"] == 0 and 0.0 <= r["reanalyse/policy_kl"] < 20.0
        if t == 1:      # iteration 0's oldest rows, which iteration 2's append keeps
            n0, n1 = ns
            assert r["reanalyse/rows"] == 8
            assert buf.stamp[:n0 + n1].tolist() == [1] * 8 + [0] * (n0 - 8) + [1] * n1
        if t == 2:      # iteration 0 leaves at the next append: iteration 1's rows are taken
            n0, n1, n2 = ns
            assert r["reanalyse/rows"] == 8 and buf.rows_leaving(3) == n0
            assert buf.stamp[:n0 + n1 + n2].tolist() == \
                [1] * 8 + [0] * (n0 - 8) + [2] * 8 + [1] * (n1 - 8) + [2] * n2
    assert rs[0]["reanalyse/rows"] == 0 and rs[0]["reanalyse/policy_kl"] == 0.0
    # ... was held, with its new stamp, while iteration 3 trained
    assert buf.rows_by_iteration()[0] == (1, ns[1]) and len(buf) == ns[1] + ns[2] + ns[3]
    first = buf.start
    assert first == ns[0]
    assert [(int(buf.mover[s]), int(buf.opponent[s])) for s in range(first, first + 8)] == refreshed
    assert (buf.stamp[first:first + 8] >= 2).all()
    sums = buf.policy[first:first + 8].double().sum(1)
    assert float((sums - 1).abs().max()) < 1e-6
