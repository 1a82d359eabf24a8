"""rvz_solve_window (csrc/rvz_solve.hip: k_solve_window), the windowed / win-draw-loss endgame
solve with optional move ordering, on the GPU against the host references of tests/solve_ref.py
(unpruned negamax) and tests/solve_window_ref.py (the same fail-soft search in index order, node
for node), and endgame adjudication in SelfPlayTrainer."""
import copy

import numpy as np
import pytest
import torch

import solve_ref as R
import solve_window_ref as W

pytestmark = pytest.mark.gpu

BIG = 2 ** 40        # a node limit no row of these tests reaches

# test_gpu_solve.py's position sets: (board size, seeds, empties) -> the offsets (lo, hi) of the
# middle window (med + lo, med + hi) around the set's median host score. (-8, -2) where it has 4
# rows below, inside and above; the 16 rows at 8 empties (scores -14 .. 16, median 2) put only 3
# below and 2 inside it, so there the offsets are (-4, +2): 5 below, 5 inside, 6 above.
SETS = {
    "8x8e6": (8, range(64), 6, (-8, -2)),
    "8x8e8": (8, range(16), 8, (-4, 2)),
    "6x6e6": (6, range(64), 6, (-8, -2)),
}


def set_rows(name):
    bs, seeds, empties, _ = SETS[name]
    return bs, [R.position(s, empties, bs)[0] for s in seeds], \
        [R.solved(s, empties, bs) for s in seeds]


def set_windows(name):
    """The windows of a set, after asserting on the host values alone that each separates the
    rows: at least 4 below it, 4 inside where its width allows and 4 above (the two fixed
    windows as far as they can: (-64, 64) holds every row, and (-1, 1) holds only the draws,
    of which these seeds have 3, 1 and 2)."""
    bs, seeds, empties, (lo, hi) = SETS[name]
    v = [R.solved(s, empties, bs)[0] for s in seeds]
    med = int(np.median(v))
    out = [(-1, 1), (-64, 64), (med, med + 1), (med + lo, med + hi), (med + 2, 64)]
    for alpha, beta in out:
        below = sum(x <= alpha for x in v)
        inside = sum(alpha < x < beta for x in v)
        above = sum(x >= beta for x in v)
        if (alpha, beta) == (-64, 64):
            assert inside == len(v)
            continue
        assert below >= 4, (name, alpha, beta, below)
        if beta < 64:
            assert above >= 4, (name, alpha, beta, above)
        if (alpha, beta) == (-1, 1):
            assert inside >= 1
        elif beta - alpha >= 2:
            assert inside >= 4, (name, alpha, beta, inside)
    return out


def gpu_window(games, bs, alpha, beta, order=0, max_empties=None, node_limit=BIG):
    import rvz
    from rvz._lib import RVZ_SOLVE_MAX_EMPTIES
    b, w, st = R.to_device(games)
    s, m, k = rvz.solve_window(b, w, st, bs, RVZ_SOLVE_MAX_EMPTIES if max_empties is None else
                               max_empties, node_limit, alpha, beta, order)
    assert s.dtype == torch.int32 and m.dtype == torch.int32 and k.dtype == torch.int64
    assert s.is_cuda and m.is_cuda and k.is_cuda
    return s.cpu().numpy(), m.cpu().numpy(), k.cpu().numpy()


def gpu_solve(games, bs):
    import rvz
    b, w, st = R.to_device(games)
    return tuple(t.cpu().numpy() for t in rvz.solve(b, w, st, bs, 14, BIG))


@pytest.mark.parametrize("name", list(SETS))
def test_windows_ordering_off(name):
    bs, seeds, empties, _ = SETS[name]
    wins = set_windows(name)
    _, games, host = set_rows(name)
    fs, fm, fk = gpu_solve(games, bs)
    assert [(int(a), int(b)) for a, b in zip(fs, fm)] == [h[:2] for h in host]
    for alpha, beta in wins:
        score, move, nodes = gpu_window(games, bs, alpha, beta)
        for i, s in enumerate(seeds):
            v = host[i][0]
            W.check_result(games[i], bs, alpha, beta, v, score[i], move[i])
            want = W.window_ab_seed(s, empties, bs, alpha, beta)
            assert (score[i], move[i], nodes[i]) == want, (name, alpha, beta, s, want)
            assert nodes[i] <= fk[i], (name, alpha, beta, s, nodes[i], fk[i])
            if (alpha, beta) == (-64, 64):
                assert score[i] == fs[i] and (v <= -64 or move[i] == fm[i])
            if (alpha, beta) == (-1, 1):
                assert np.sign(score[i]) == np.sign(v)


@pytest.mark.parametrize("order", [1, 4])
@pytest.mark.parametrize("name", list(SETS))
def test_windows_ordering_on(name, order):
    bs, seeds, empties, _ = SETS[name]
    _, games, host = set_rows(name)
    for alpha, beta in set_windows(name):
        got = gpu_window(games, bs, alpha, beta, order)
        again = gpu_window(games, bs, alpha, beta, order)
        for a, b in zip(got, again):
            assert np.array_equal(a, b), (name, alpha, beta)
        score, move, nodes = got
        for i, s in enumerate(seeds):
            W.check_result(games[i], bs, alpha, beta, host[i][0], score[i], move[i],
                           W.child_values_seed(s, empties, bs))
            assert nodes[i] >= 1
            if (alpha, beta) == (-64, 64):
                assert score[i] == host[i][0]


@pytest.mark.parametrize("order", [None, 0, 1, 4])
def test_solve_wld(order):
    import rvz
    for name in SETS:
        bs, games, host = set_rows(name)
        b, w, st = R.to_device(games)
        kw = {} if order is None else {"order_min_empties": order}
        out, move, nodes = rvz.solve_wld(b, w, st, bs, 14, BIG, **kw)
        assert out.dtype == torch.int32 and move.dtype == torch.int32
        assert [int(x) for x in out.cpu()] == [int(np.sign(h[0])) for h in host], name
        m = move.cpu().numpy()
        assert all((m[i] == -6) == (host[i][0] < 0) for i in range(len(host)))   # a loss
    # unsolved rows report 0
    deep = [R.position(0, 7, 8)[0], R.position(1, 6, 8)[0]]
    b, w, st = R.to_device(deep)
    out, move, _ = rvz.solve_wld(b, w, st, 8, 6, BIG, **kw)
    assert int(move[0]) == -3 and int(out[0]) == 0
    out, move, _ = rvz.solve_wld(b, w, st, 8, 7, 1, **kw)
    assert [int(x) for x in move.cpu()] == [-4, -4] and not bool(out.any())


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("bs,seeds", [(8, (12, 25)), (6, (9, 15))])
def test_root_cases(bs, seeds, order):
    """test_gpu_solve.py's root cases under the window (-1, 1)."""
    c = R.RootCases(bs, seeds)
    want = gpu_window(c.plain, bs, -1, 1, order)
    score, move, nodes = gpu_window(c.mixed, bs, -1, 1, order, max_empties=6)
    for got, w in zip((score, move, nodes), want):
        assert np.array_equal(got[c.keep], w)
    for i, j in c.where.items():
        es, em, ends = c.expect[j]
        assert move[i] == em, (j, move[i], em)
        if ends:
            assert score[i] == es, (j, score[i], es)
        else:       # a pass that does not end the game: fail-soft in (-1, 1)
            W.check_result(c.mixed[i], bs, -1, 1, es, score[i], move[i])
            if order == 0:
                assert (score[i], move[i], nodes[i]) == W.window_ab(c.mixed[i], bs, -1, 1)
        assert (nodes[i] == 0) if move[i] in (-3, -5) else (nodes[i] >= 1)
    s0, m0, _ = gpu_window(c.zero, bs, -1, 1, order, max_empties=0)
    c.check_zero(bs, s0, m0)


def test_batch_shape_independence():
    """A row's answer and node count do not depend on the batch it is in, ordering on: size 1,
    63, 65 and 130 batches built by repeating and permuting the 64 rows, on a second stream."""
    games = [R.position(s, 6, 8)[0] for s in range(64)]
    rng = np.random.RandomState(5)
    for order in (1, 4):
        base = gpu_window(games, 8, -1, 1, order)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for n in (1, 63, 65, 130):
                idx = np.concatenate([rng.permutation(64) for _ in range(-(-n // 64))])[:n]
                got = gpu_window([games[i] for i in idx], 8, -1, 1, order)
                for a, b in zip(got, base):
                    assert np.array_equal(a, b[idx]), (order, n)
        side.synchronize()


def test_node_limit():
    seeds = range(64)
    games = [R.position(s, 6, 8)[0] for s in seeds] + [R.position(3, 0, 8)[0]]
    host = [W.window_ab_seed(s, 6, 8, -1, 1) for s in seeds]
    score, move, nodes = gpu_window(games, 8, -1, 1)
    assert [int(k) for k in nodes[:64]] == [h[2] for h in host]
    again = gpu_window(games, 8, -1, 1, node_limit=max(h[2] for h in host))
    for a, b in zip(again, (score, move, nodes)):
        assert np.array_equal(a, b)
    i = int(np.argmax(nodes > 1))
    k = host[i][2]
    assert k > 1
    s1, m1, k1 = gpu_window([games[i]], 8, -1, 1, node_limit=k)
    assert (s1[0], m1[0], k1[0]) == host[i]
    s1, m1, k1 = gpu_window([games[i]], 8, -1, 1, node_limit=k - 1)
    assert (s1[0], m1[0], k1[0]) == (0, -4, k - 1)
    for order in (0, 4):
        s1, m1, _ = gpu_window(games, 8, -1, 1, order, node_limit=1)
        assert list(m1[:64]) == [-4] * 64 and not s1[:64].any()
        assert (s1[64], m1[64]) == (score[64], -2)


def test_api_errors():
    import rvz
    lib = rvz.load()
    EINVAL = -22
    games = [R.position(s, 6, 8)[0] for s in range(4)]
    b, w, st = R.to_device(games)
    sc = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    mv = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    nd = torch.full((4,), 77, dtype=torch.int64, device="cuda")
    p = [t.data_ptr() for t in (b, w, st, sc, mv, nd)]

    def call(bs=8, n=4, me=6, limit=1000, alpha=-1, beta=1, order=0, ptrs=p):
        return lib.rvz_solve_window(bs, n, ptrs[0], ptrs[1], ptrs[2], me, limit, alpha, beta,
                                    order, ptrs[3], ptrs[4], ptrs[5], None)

    assert call(bs=7) == EINVAL and call(n=-1) == EINVAL and call(me=15) == EINVAL
    assert call(limit=0) == EINVAL and call(order=-1) == EINVAL
    for alpha, beta in ((0, 0), (1, -1), (-65, 0), (0, 65)):
        assert call(alpha=alpha, beta=beta) == EINVAL
    for k in range(5):
        assert call(ptrs=[None if j == k else q for j, q in enumerate(p)]) == EINVAL
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in (sc, mv, nd))        # nothing was launched
    for kw in (dict(alpha=3, beta=3), dict(alpha=-65), dict(beta=65), dict(order_min_empties=-1),
               dict(max_empties=15), dict(node_limit=0)):
        with pytest.raises(rvz.RvzError):
            rvz.solve_window(b, w, st, 8, **kw)
    with pytest.raises(rvz.RvzError):
        rvz.solve_wld(b, w, st, 8, order_min_empties=-1)
    s0, m0, k0 = rvz.solve_wld(b[:0], w[:0], st[:0], 8)
    assert s0.numel() == m0.numel() == k0.numel() == 0
    # out_nodes is nullable
    assert call(me=14, limit=BIG, ptrs=p[:5] + [None]) == 0
    torch.cuda.synchronize()
    assert [int(x) for x in mv.cpu()] == [W.window_ab_seed(s, 6, 8, -1, 1)[1] for s in range(4)]
    assert bool((nd == 77).all())
    net = rvz.AlphaZeroNetwork(6, 1, 64).cuda()
    from rvz.pipeline import SelfPlayTrainer
    for bad in (-1, 15, 32):
        with pytest.raises(ValueError):
            SelfPlayTrainer(net, games=4, num_simulations=16, batch_size=16,
                            adjudicate_empties=bad)


def test_engine_solve_wld():
    import rvz
    games = [R.position(s, 6, 8)[0] for s in range(16)]
    b, w, st = R.to_device(games)
    eng = rvz.Engine(16, num_simulations=16, batch_size=16, device="cuda:0")
    eng.set_state(b, w, st)
    before = [t.clone() for t in eng.get_state()]
    for order in (None, 0, 4):
        got = eng.solve_wld(8, node_limit=BIG, order_min_empties=order)
        assert [int(x) for x in got[0].cpu()] == \
            [int(np.sign(R.solved(s, 6, 8)[0])) for s in range(16)]
        if order is not None:
            want = rvz.solve_wld(b, w, st, 8, 8, BIG, order)
            for a, c in zip(got, want):
                assert torch.equal(a, c)
    for a, c in zip(before, eng.get_state()):
        assert torch.equal(a, c)
    eng.check()


def popcount(a):
    return np.array([bin(int(x)).count("1") for x in a])


@pytest.mark.parametrize("fused", [True, False])
def test_adjudicated_iteration(fused):
    """SelfPlayTrainer(adjudicate_empties=6) on 6x6 against the full run of the same net and
    seeds: the first 26 plies' records are byte-identical, the data holds exactly the kept
    records of those plies (all with more than 6 empties), and every value target is the sign of
    the host negamax of the game's stopping position, relative to the row's side. 64 games at 48
    simulations (three leaf batches: at 32 every game is one game, see test_gpu_solve.py)."""
    import rvz
    from rvz.pipeline import SelfPlayTrainer
    N, bs, G = 6, 6, 64
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(bs, 1, 64).cuda()
    kw = dict(games=G, num_simulations=48, batch_size=16, seed=0, train_steps=1, train_batch=16,
              fused=fused)
    full = SelfPlayTrainer(copy.deepcopy(net), **kw)
    zero = SelfPlayTrainer(copy.deepcopy(net), adjudicate_empties=0, **kw)
    adj = SelfPlayTrainer(copy.deepcopy(net), adjudicate_empties=N, adjudicate_node_limit=BIG,
                          **kw)
    assert full.fused == fused
    d_full, d_zero, d_adj = full.generate(), zero.generate(), adj.generate()
    # off is the parent
    assert set(d_full) == set(d_zero) == {"states", "policy_targets", "value_targets"}
    for k in d_full:
        assert torch.equal(d_full[k], d_zero[k]), k
    # the condition of this test: nothing abandoned
    assert int(d_adj["adjudicate_unsolved"]) == 0
    assert int(d_adj["adjudicated"]) + int(d_adj["already_over"]) == G
    assert int(d_adj["adjudicated"]) >= G // 2
    K = bs * bs - 4 - N
    fr, ar = full.runner, adj.runner
    for name in ("rec_black", "rec_white", "rec_side", "rec_idx", "rec_p"):
        assert torch.equal(getattr(fr, name)[:K], getattr(ar, name)[:K]), name
    # the rows: the full run's rows of plies < K, in order
    live = (fr.rec_idx >= 0).t()                                   # [G, P]
    early = (torch.arange(live.shape[1], device=live.device) < K).expand_as(live)[live]
    assert int(early.sum()) == d_adj["states"].shape[0] < d_full["states"].shape[0]
    assert torch.equal(d_full["states"][early], d_adj["states"])
    assert torch.equal(d_full["policy_targets"][early], d_adj["policy_targets"])
    lv = live[:, :K].reshape(-1).cpu().numpy()
    rb = ar.rec_black[:K].t().reshape(-1).cpu().numpy()[lv].view(np.uint64)
    rw = ar.rec_white[:K].t().reshape(-1).cpu().numpy()[lv].view(np.uint64)
    rs = ar.rec_side[:K].t().reshape(-1).cpu().numpy()[lv]
    game_of = np.repeat(np.arange(G), K)[lv]
    assert len(rb) == d_adj["states"].shape[0]
    assert (bs * bs - popcount(rb | rw)).min() > N
    # value targets of 8 sampled games
    b, w, st = (t.cpu().numpy() for t in adj.eng.get_state())
    v = d_adj["value_targets"].reshape(-1).cpu().numpy()
    outcomes = set()
    for g in range(0, G, 8):
        pos = R.O.Game(int(b[g:g + 1].view(np.uint64)[0]), int(w[g:g + 1].view(np.uint64)[0]),
                       int(st[g, 0]), int(st[g, 1]), int(st[g, 2]), int(st[g, 3]))
        if pos.over:
            winner = pos.winner
        else:
            assert R.empties(pos, bs) == N
            s = R.negamax(pos, bs)[0]
            winner = pos.side if s > 0 else (3 - pos.side if s < 0 else 0)
        rows = np.flatnonzero(game_of == g)
        assert len(rows) >= K // 2
        for i in rows:
            want = 0.0 if winner == 0 else (1.0 if rs[i] == winner else -1.0)
            assert v[i] == want, (g, i, v[i], want)
        outcomes.add(winner)
    assert len(outcomes) >= 2
    r = adj.run_iteration()                # iteration 0 again: the same games
    assert r["adjudicate_unsolved"] == 0 and r["adjudicated"] == int(d_adj["adjudicated"])
    assert r["already_over"] == int(d_adj["already_over"]) and r["board_steps"] <= G * K


@pytest.mark.parametrize("order", [0, 4])
@pytest.mark.parametrize("bs", [8, 6])
def test_synthetic_rows(bs, order):
    """rvz_solve_window's fail-soft contract on solve_ref.synthetic_rows (positions no playout
    reaches, pass roots and roots where neither side can move among them) at (-1, 1) and
    (-64, 64); with ordering off also node for node the host's search in index order."""
    R.check_synthetic_kinds(bs)
    games, host = R.synthetic_rows(bs), R.synthetic_solved(bs)
    values = [W.child_values(g, bs) for g in games]
    for alpha, beta in ((-1, 1), (-64, 64)):
        score, move, nodes = gpu_window(games, bs, alpha, beta, order,
                                        max_empties=R.SYNTHETIC_MAX_EMPTIES)
        for i, g in enumerate(games):
            W.check_result(g, bs, alpha, beta, host[i][0], score[i], move[i], values[i])
            assert nodes[i] >= 1
            if order == 0:
                want = W.window_ab(g, bs, alpha, beta)
                assert (score[i], move[i], nodes[i]) == want, (bs, alpha, beta, g.astuple(), want)
