"""The final-ownership targets on the device against the NumPy restatements
(tests/ownership_ref.py): rvz_records_final array for array on the engine's own autoreset records
and on hand-made rows, rvz_replay_ownership bit for bit and against a real draw's state planes,
rvz_ownership_loss within the policy loss's float64 bound, the three calls in one HIP graph, and
SelfPlayTrainer(ownership_coef=...) end to end, lockstep and continuous.

The loss's bound: every float64 output within 1e-12 of the reference, the project's tolerance for
rvz_policy_value_loss (tests/test_gpu_loss.py has its derivation; here every term (tanh - t)^2 is
at most 4 and a row sums 36 or 64 of them, so the scale is 1). A float32 gradient is the float64
value rounded once, so kernel and reference agree or are adjacent float32 numbers, provided the
two tanh, an ulp apart at most, leave 1 - tanh^2 that close too: the factor loses
log2(1 / (1 - tanh^2)) bits to cancellation, so the test's logits are either within [-8, 8]
(1 - tanh^2 >= 4.5e-7, an ulp of tanh moves it by 2.5e-10 relative, 1/240 of a float32 ulp) or
at and beyond +-25, where tanh is exactly +-1 in float64 and the gradient exactly 0.
Outputs are pre-filled (NaN, or a sentinel) before every raw call, so a comparison also shows
which elements were written."""
import functools

import numpy as np
import pytest
import torch

import ownership_ref as OR
import records_games_ref as RG

pytestmark = pytest.mark.gpu

SENTINEL = -0x0123456789ABCDEF


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64) \
        if t.dtype.is_floating_point else t


# ---------------------------------------------------------------- rvz_records_final
def _net(bs, head=False):
    import rvz
    torch.manual_seed(0)
    return rvz.AlphaZeroNetwork(bs, 1, 64, ownership_head=head).cuda().eval()


@functools.lru_cache(maxsize=None)
def _engine_window(bs):
    """64 slots by S*S - 4 + 8 plies of the engine's own autoreset play behind the runner's empty
    carry of 8 plies, which hold no record: game boundaries, passes, early ends and open tails.
    48 simulations in three batches of 16: a search of one or two batches gives a one-hot
    policy, and every slot would play the same full-length game. Returns the five record tensors
    on the device."""
    import rvz
    K = bs * bs - 4 + 8
    eng = rvz.Engine(64, 48, 16, board_size=bs, compact_leaves=True, memo=True)
    run = rvz.SelfPlayRunner(eng, rvz.LeafEvaluator(_net(bs)), record=True, max_plies=K,
                             fused=True, autoreset=True, carry_plies=8, skip_last_eval=True)
    run.start()
    run.play_record(K)
    run.check()
    return tuple(t.clone() for t in (run.rec_black, run.rec_white, run.rec_side, run.rec_idx,
                                     run.rec_p))


@functools.lru_cache(maxsize=None)
def _window_reference(bs):
    """The reference's walk from every record of _engine_window(bs), once."""
    from oracle import oracle as O
    O.lib()
    b, w, s, i = (t.cpu().numpy() for t in _engine_window(bs)[:4])
    P, G = i.shape
    return OR.final(O, bs, b.view(np.uint64), w.view(np.uint64), s, i, np.arange(P * G))


def _raw_final(bs, win, src, count, n=None):
    """rvz_records_final through the C-ABI on sentinel-filled outputs."""
    import rvz
    lib = rvz.load()
    b, w, s, i = (t.contiguous() for t in win[:4])
    P, G = i.shape
    n = src.numel() if n is None else n
    fm = torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda")
    fo = torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda")
    ok = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    stats = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    rc = lib.rvz_records_final(bs, P, G, b.data_ptr(), w.data_ptr(), s.data_ptr(), i.data_ptr(),
                               n, src.data_ptr(), None if count is None else count.data_ptr(),
                               fm.data_ptr(), fo.data_ptr(), ok.data_ptr(), stats.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return fm, fo, ok, stats


def _same_final(got, ref, rows=None, what=""):
    fm, fo, ok, stats = got
    rfm, rfo, rok, rstats = ref[:4]
    sel = slice(None) if rows is None else rows
    assert np.array_equal(fm.cpu().numpy().view(np.uint64)[sel], rfm[sel]), what
    assert np.array_equal(fo.cpu().numpy().view(np.uint64)[sel], rfo[sel]), what
    assert np.array_equal(ok.cpu().numpy()[sel], rok[sel]), what
    assert stats.tolist() == rstats.tolist(), (what, stats.tolist(), rstats.tolist())


@pytest.mark.parametrize("bs", [6, 8])
def test_records_final_on_the_engines_window(bs):
    """src = every record, and src / count = records_games' out_src / out_m passed straight
    through: array for array the reference's."""
    import rvz
    win = _engine_window(bs)
    ref = _window_reference(bs)
    P, G = win[3].shape
    every = torch.arange(P * G, dtype=torch.int32, device="cuda")
    _same_final(_raw_final(bs, win, every, None), ref, what="every record")
    stats = ref[3].tolist()
    print("window", bs, "stats", stats, "records", int((win[3] >= 0).sum()), "of", P * G,
          "moves", int(win[3].min()), "..", int(win[3].max()))
    assert stats[0] == P * G and stats[1] > 0 and stats[2] > 0      # finished games, open tails
    assert stats[3] == 8 * G                                        # the empty carry's plies
    # through the Python surface, with records_games' outputs and no host read in between
    games = rvz.records_games(*win, bs, emit_from=0)
    out = rvz.records_final(*win[:4], games["src"], games["m"], bs)
    m = int(games["m"])
    assert 0 < m < P * G and int(games["stats"][1]) >= G            # game boundaries inside
    src = games["src"][:m].cpu().numpy().astype(np.int64)
    assert np.array_equal(out["final_mover"][:m].cpu().numpy().view(np.uint64), ref[0][src])
    assert np.array_equal(out["final_opponent"][:m].cpu().numpy().view(np.uint64), ref[1][src])
    assert bool((out["ok"][:m] == 1).all()) and ref[2][src].all()
    assert out["stats"].tolist() == [m, m, 0, 0]
    # the rows at and above *out_m are not written
    raw = _raw_final(bs, win, games["src"], games["m"])
    assert bool((raw[0][m:] == SENTINEL).all()) and bool((raw[1][m:] == SENTINEL).all())
    assert bool((raw[2][m:] == -7).all()) and torch.equal(raw[0][:m], out["final_mover"][:m])
    # the final position decides the game: the margin's sign is records_games' value target
    fm, fo = (out[k][:m].cpu().numpy().view(np.uint64) for k in ("final_mover", "final_opponent"))
    margin = np.array([bin(int(a)).count("1") - bin(int(c)).count("1") for a, c in zip(fm, fo)])
    assert np.array_equal(np.sign(margin), games["value"][:m].cpu().numpy())


@pytest.mark.parametrize("bs", [6, 8])
def test_records_final_hand_made_rows(oracle, bs):
    """A negative src, one past the window, one on a gap, a broken chain, a malformed record, and
    a count below n (also 0, negative and above n) with the rows beyond it untouched."""
    nsq = bs * bs
    P, G = nsq + 6, 9
    black, white, side, idx, p = RG.window(oracle, bs, P, G, 21, gaps={4: (6, 7, 20)})
    # slot 5: record 9 becomes the start position with its first move (a broken chain for the
    # rows before it); slot 2: a side of 3 at ply 11; slot 3: a disc of both colours at ply 5
    black[9, 5], white[9, 5], side[9, 5], idx[9, 5] = black[0, 5], white[0, 5], 1, idx[0, 5]
    side[11, 2] = 3
    white[5, 3] = np.uint64(int(white[5, 3]) | (int(black[5, 3]) & -int(black[5, 3])))
    win = RG.tensors(black, white, side, idx, p, device="cuda")
    src = np.concatenate([[-1, -2 ** 31, P * G, 2 ** 31 - 1, 6 * G + 4, 20 * G + 4],
                          np.arange(P * G)]).astype(np.int32)
    ref = OR.final(oracle, bs, black, white, side, idx, src)
    code = ref[5]
    assert (code[:6] == 3).all() and not ref[2][:6].any()
    at = lambda ply, g: 6 + ply * G + g
    # (record 9 itself is followed by a record that does not continue it)
    assert all(code[at(q, 5)] == 3 for q in range(10)) and code[at(10, 5)] in (1, 2)
    assert all(code[at(q, 2)] == 3 for q in range(12)) and code[at(12, 2)] in (1, 2)
    assert all(code[at(q, 3)] == 3 for q in range(6))
    assert code[at(5, 4)] == 1 and code[at(8, 4)] == 1               # the walk crosses the gaps
    assert (code == 1).sum() > P and (code == 2).sum() > G
    t_src = torch.from_numpy(src).cuda()
    _same_final(_raw_final(bs, win, t_src, None), ref, what="hand-made")
    n = len(src)
    for count in (n // 3, 0, -5, n, n + 100):
        refc = OR.final(oracle, bs, black, white, side, idx, src, count)
        got = _raw_final(bs, win, t_src, torch.tensor([count], dtype=torch.int32, device="cuda"))
        bound = refc[4]
        _same_final(got, refc, rows=slice(0, bound), what=f"count={count}")
        assert bool((got[0][bound:] == SENTINEL).all()) and bool((got[2][bound:] == -7).all())
    a, b = _raw_final(bs, win, t_src, None), _raw_final(bs, win, t_src, None)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---------------------------------------------------------------- rvz_replay_ownership
@functools.lru_cache(maxsize=None)
def _final_ring(bs, cap=50):
    """Random final positions, host arrays; slot 5 overlaps, slot 6 (6x6) leaves the board."""
    rng = np.random.default_rng(31 + bs)
    nsq = bs * bs
    pick = rng.integers(0, 3, (cap, nsq))
    fm = np.array([sum(1 << s for s in range(nsq) if pick[r, s] == 1) for r in range(cap)],
                  np.uint64)
    fo = np.array([sum(1 << s for s in range(nsq) if pick[r, s] == 2) for r in range(cap)],
                  np.uint64)
    fo[5] |= np.uint64(int(fm[5]) & -int(fm[5]))
    if bs == 6:
        fm[6] |= np.uint64(1 << 40)
    return fm, fo


def _raw_ownership(bs, fm, fo, slot, sym):
    import rvz
    lib = rvz.load()
    nb = slot.numel()
    own = torch.full((nb, bs * bs), float("nan"), device="cuda")
    margin = torch.full((nb,), float("nan"), device="cuda")
    rc = lib.rvz_replay_ownership(bs, fm.numel(), fm.data_ptr(), fo.data_ptr(), nb,
                                  slot.data_ptr(), sym.data_ptr(), own.data_ptr(),
                                  margin.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return own, margin


@pytest.mark.parametrize("nb", [1, 64, 65])
@pytest.mark.parametrize("bs", [6, 8])
def test_replay_ownership_against_the_reference(bs, nb):
    fm, fo = _final_ring(bs)
    cap = len(fm)
    rng = np.random.default_rng(nb)
    slot = rng.integers(0, cap, nb).astype(np.int32)
    sym = (np.arange(nb) % 8).astype(np.int32)                      # all eight symmetries
    if nb >= 64:
        slot[3], slot[4], slot[9], slot[10], slot[11] = -1, cap, 5, 6, -2 ** 31
        sym[3], sym[12], sym[13], sym[14] = -1, 9, 8, -1
        slot[16:24] = 7                                             # one slot under every T_k
    else:
        sym[0] = 6
    want_own, want_margin = OR.ownership(bs, fm, fo, slot, sym)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int64) if a.dtype == np.uint64
                                                          else a)).cuda()
    own, margin = _raw_ownership(bs, dev(fm), dev(fo), dev(slot), dev(sym))
    assert own.cpu().numpy().tobytes() == want_own.tobytes()        # +0.0 where the reference's
    assert margin.cpu().numpy().tobytes() == want_margin.tobytes()
    assert torch.equal(own.sum(1), margin)
    if nb >= 64:
        for r in (3, 4, 9, 11, 12, 13, 14) + ((10,) if bs == 6 else ()):
            assert not own[r].any() and margin[r].item() == 0, r
        import rvz
        again = rvz.replay_ownership(dev(fm), dev(fo), dev(slot).long(), dev(sym), bs)
        assert torch.equal(_bits(again[0]), _bits(own)) and torch.equal(again[1], margin)


@pytest.mark.parametrize("kind", ["uniform", "weighted", "prioritized"])
def test_ownership_of_a_real_draw_covers_the_state_planes(kind):
    """Discs are never removed in Reversi: every square occupied in a drawn row's state planes
    is owned in the row's ownership target. That pins the symmetry's direction to the batch
    kernel's. And a zero row of the draw is a zero row here."""
    import rvz
    bs = 6
    win = _engine_window(bs)
    games = rvz.records_games(*win, bs, emit_from=0)
    fin = rvz.records_final(*win[:4], games["src"], games["m"], bs)
    m = int(games["m"])
    kw = {"weighted": dict(weighted=True), "prioritized": dict(prioritized=True)}.get(kind, {})
    buf = rvz.ReplayBuffer(m + 7, bs, ownership=True, **kw)
    half = m // 2
    for it, rows in ((0, slice(0, half)), (1, slice(half, m)), (2, slice(0, 40))):   # wraps
        buf.append(games["mover"][rows], games["opponent"][rows], games["policy"][rows],
                   games["value"][rows], it, final_mover=fin["final_mover"][rows],
                   final_opponent=fin["final_opponent"][rows])
    out = buf.sample(512, 9, 1, **({"with_prob": True} if kind == "prioritized" else {}))
    states, value, slot, sym, own, margin = out[0], out[2], out[3], out[4], out[-2], out[-1]
    assert own.shape == (512, 36) and margin.shape == (512,)
    assert bool((slot >= 0).all()) and sorted(sym.unique().tolist()) == list(range(8))
    occupied = (states[:, 0] + states[:, 1]).reshape(512, 36) > 0
    assert bool((own[occupied] != 0).all())
    assert bool((own.abs().sum(1) >= occupied.sum(1)).all()) and torch.equal(own.sum(1), margin)
    assert torch.equal(torch.sign(margin), value.reshape(-1))      # the winner has more discs
    # the definition, row by row, from the ring's own columns
    want, _ = OR.ownership(bs, buf.final_mover.cpu().numpy().view(np.uint64),
                           buf.final_opponent.cpu().numpy().view(np.uint64),
                           slot.cpu().numpy(), sym.cpu().numpy())
    assert np.array_equal(own.cpu().numpy(), want)
    bad = buf.sample(4, 9, 2, idx=torch.tensor([0, -1, 10 ** 6, 1]),
                     sym=torch.tensor([0, 1, 2, 9]))
    assert bad[3].tolist()[1:3] == [-1, -1] and bad[4].tolist()[1:] == [-1, -1, -1]
    assert bad[-2][0].any() and not bad[-2][1:].any() and not bad[-1][1:].any()


# ---------------------------------------------------------------- rvz_ownership_loss
MALFORMED = 6                         # malformed rows in _loss_inputs at n >= 65 (3 need a weight)


@functools.lru_cache(maxsize=None)
def _loss_inputs(bs, n, weighted):
    """The shared inputs of one case, host arrays; never modified."""
    nsq = bs * bs
    g = np.random.default_rng(100 * bs + n)
    o = np.clip(g.standard_normal((n, nsq)) * 2.5, -8.0, 8.0)
    sat = g.random((n, nsq)) < 0.05
    o[sat] = g.choice(np.array([25.0, -25.0, 1e4, -300.0]), int(sat.sum()))
    o[g.random((n, nsq)) < 0.02] = 0.0
    o = o.astype(np.float32)
    t = g.integers(-1, 2, (n, nsq)).astype(np.float32)
    if n >= 2:
        t[n // 2] = 0.0                                      # a row without an owned square
    w = None
    if weighted:
        w = g.integers(1, 4097, n).astype(np.float32)
        w[g.random(n) < 0.1] = 0.0
    if n >= 65:
        o[10, 3], o[11, nsq - 1] = np.nan, -np.inf
        t[12, 5] = 0.5
        if w is not None:
            w[13], w[14], w[15] = -1.0, np.inf, np.nan
    for a in (o, t) + (() if w is None else (w,)):
        a.setflags(write=False)
    return o, t, w


@functools.lru_cache(maxsize=None)
def _loss_reference(bs, n, weighted):
    return OR.loss(*_loss_inputs(bs, n, weighted))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw_loss(bs, dev, rows=True, grads=True):
    """rvz_ownership_loss through the C-ABI on NaN-filled outputs and a scratch of NaN bits."""
    import rvz
    from rvz._lib import ptr
    lib = rvz.load()
    o, t, w = dev
    n, nsq = o.shape
    out = (torch.full((8,), float("nan"), dtype=torch.float64, device="cuda"),
           torch.full((n, 2), float("nan"), dtype=torch.float64, device="cuda"),
           torch.full((n, nsq), float("nan"), device="cuda"))
    scratch = torch.full((lib.rvz_ownership_loss_scratch_size(bs, n),), 0xFF, dtype=torch.uint8,
                         device="cuda")
    rc = lib.rvz_ownership_loss(bs, n, o.data_ptr(), t.data_ptr(),
                                None if w is None else w.data_ptr(), ptr(scratch),
                                out[0].data_ptr(), out[1].data_ptr() if rows else None,
                                out[2].data_ptr() if grads else None,
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def _adjacent(got, want):
    up = np.nextafter(want, np.float32(np.inf))
    down = np.nextafter(want, np.float32(-np.inf))
    return (got == want) | (got == up) | (got == down)


def _compare_loss(got, ref, what):
    out_loss, rows, grad = (x.cpu().numpy() for x in got)
    err = np.abs(out_loss - ref["out_loss"])
    print(what, "out_loss err", err.max(), "rows err", np.abs(rows - ref["rows"]).max())
    assert np.isfinite(out_loss).all() and np.isfinite(rows).all() and np.isfinite(grad).all()
    assert (err <= 1e-12).all(), (what, err)
    assert (np.abs(rows - ref["rows"]) <= 1e-12).all(), what
    for k in (2, 3, 4, 6, 7):                                # zeros, W on integer weights, count
        assert out_loss[k] == ref["out_loss"][k], (what, k)
    assert out_loss[0] == out_loss[1]
    assert _adjacent(grad, ref["grad_logits"]).all(), what


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [1, 65, 4097])
@pytest.mark.parametrize("bs", [8, 6])
def test_ownership_loss_against_the_reference(bs, n, weighted):
    host = _loss_inputs(bs, n, weighted)
    ref = _loss_reference(bs, n, weighted)
    if n >= 65:
        assert ref["out_loss"][6] == (MALFORMED if weighted else MALFORMED - 3)
        assert ref["grad_logits"].any() and not ref["grad_logits"][10:13].any()
    dev = [_dev(a) for a in host]
    got = _raw_loss(bs, dev)
    _compare_loss(got, ref, (bs, n, weighted))
    again = _raw_loss(bs, dev)
    for x, y in zip(got, again):                             # the same bytes on every call
        assert torch.equal(_bits(x), _bits(y))
    off = _raw_loss(bs, dev, rows=False, grads=False)
    assert torch.isnan(off[1]).all() and torch.isnan(off[2]).all()
    assert torch.equal(_bits(off[0]), _bits(got[0]))


def test_ownership_loss_zero_weights_and_autograd():
    import rvz
    bs, n = 6, 65
    o, t, w = (_dev(a) for a in _loss_inputs(bs, n, True))
    zero = _raw_loss(bs, (o, t, torch.zeros_like(w)))
    assert not zero[0][:6].any() and not zero[2].any()
    plain = rvz.ownership_loss(o, t, w, bs, rows=True)
    _compare_loss((plain["out_loss"], plain["rows"], plain["grad_logits"]),
                  _loss_reference(bs, n, True), "python surface")
    for k, i in (("loss", 0), ("weight_sum", 4), ("agreement", 5), ("malformed", 6)):
        assert plain[k].dim() == 0 and plain[k].item() == plain["out_loss"][i].item()
    og = o.clone().requires_grad_(True)
    loss, stats = rvz.full_ownership_loss(og, t, w, bs)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    assert loss.item() == plain["loss"].float().item()
    assert set(stats) == {"agreement", "weight_sum", "malformed"}
    (loss * 3.0).backward()
    assert torch.equal(og.grad, plain["grad_logits"] * 3.0)


# ---------------------------------------------------------------- graph capture
def test_three_calls_in_one_graph():
    """records_final, replay_ownership and ownership_loss captured in one HIP graph and replayed
    twice: the eager bytes."""
    import rvz
    bs = 6
    win = _engine_window(bs)
    games = rvz.records_games(*win, bs, emit_from=0)
    n = games["src"].numel()
    slot = torch.arange(256, dtype=torch.int32, device="cuda") * 3
    sym = torch.arange(256, dtype=torch.int32, device="cuda") % 8
    logits = _dev(_loss_inputs(bs, 257, True)[0])[:256].contiguous()

    def calls():
        fin = rvz.records_final(*win[:4], games["src"], games["m"], bs)
        own, margin = rvz.replay_ownership(fin["final_mover"], fin["final_opponent"], slot, sym,
                                           bs)
        loss = rvz.ownership_loss(logits, own, None, bs, rows=True)
        return (fin["final_mover"], fin["final_opponent"], fin["ok"], fin["stats"], own, margin,
                loss["out_loss"], loss["rows"], loss["grad_logits"])

    eager = [x.clone() for x in calls()]
    assert int(eager[3][1]) == int(games["m"]) < n and eager[4].any() and eager[8].any()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = calls()
    for _ in range(2):
        for x in out:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, (x, y) in enumerate(zip(out, eager)):
            assert torch.equal(_bits(x), _bits(y)), k


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("continuous", [None, 32], ids=["lockstep", "continuous"])
def test_selfplay_trainer_with_the_ownership_target(continuous):
    """6x6, 16 games, 16 simulations, one 64-filter block, replay_iterations=2,
    ownership_coef=0.5, two iterations: the metrics are there and finite, nothing is dropped, and
    the first iteration's self-play records are those of a head-less copy of the net."""
    import rvz
    from rvz.pipeline import SelfPlayTrainer
    kw = dict(num_simulations=16, batch_size=8, seed=5, train_steps=2, train_batch=32,
              replay_iterations=2, policy_target="full", continuous_plies=continuous)
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(6, 1, 64, ownership_head=True).cuda()
    torch.manual_seed(0)
    bare = rvz.AlphaZeroNetwork(6, 1, 64).cuda()
    for k, v in bare.state_dict().items():
        assert torch.equal(v, net.state_dict()[k]), k
    with pytest.raises(ValueError, match="ownership"):
        SelfPlayTrainer(bare, 16, ownership_coef=0.5, **kw)
    spt = SelfPlayTrainer(net, 16, ownership_coef=0.5, **kw)
    ref = SelfPlayTrainer(bare, 16, **kw)
    ref.generate()
    want = [t.clone() for t in (ref.runner.rec_black, ref.runner.rec_white, ref.runner.rec_side,
                                ref.runner.rec_idx, ref.runner.rec_p)]
    for it in range(2):
        out = spt.run_iteration()
        if it == 0:
            run = spt.runner
            got = (run.rec_black, run.rec_white, run.rec_side, run.rec_idx, run.rec_p)
            for a, b in zip(got, want):     # (continuous: both windows have rolled on alike)
                assert torch.equal(a, b)
        print(continuous, it, {k: v for k, v in out.items() if "ownership" in k or k == "steps"})
        assert out["ownership_dropped"] == 0 and out["samples"] > 0 and out["steps"] == 2
        for k in ("train/loss", "train/policy_loss", "train/value_loss", "train/ownership_loss",
                  "train/ownership_agreement"):
            assert k in out and np.isfinite(out[k]), k
        assert out["train/ownership_loss"] > 0 and 0 <= out["train/ownership_agreement"] <= 1
    buf = spt.buffer
    assert buf.ownership and len(buf) > 0
    live = (torch.arange(len(buf), device="cuda") + buf.start) % buf.capacity
    fm, fo = buf.final_mover[live], buf.final_opponent[live]
    assert bool((fm & fo == 0).all()) and bool(((fm | fo) != 0).all())
    # discs are never removed: a row's own discs are owned in its final position
    assert bool((((buf.mover[live] | buf.opponent[live]) & ~(fm | fo)) == 0).all())
