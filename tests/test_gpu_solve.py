"""rvz_solve (csrc/rvz_solve.hip), the exact endgame solver, on the GPU against the host reference
of tests/solve_ref.py: the unpruned negamax over the CPU oracle's legal / make_move, i.e. the
definition in include/rvz.h with the reference's rule quirks."""
import numpy as np
import pytest
import torch

import solve_ref as R
import solve_window_ref as W

pytestmark = pytest.mark.gpu

BIG = 2 ** 40        # a node limit no row of these tests reaches


def gpu_solve(games, bs, max_empties=None, node_limit=BIG):
    import rvz
    from rvz._lib import RVZ_SOLVE_MAX_EMPTIES
    b, w, st = R.to_device(games)
    s, m, k = rvz.solve(b, w, st, bs, RVZ_SOLVE_MAX_EMPTIES if max_empties is None else
                        max_empties, node_limit)
    assert s.dtype == torch.int32 and m.dtype == torch.int32 and k.dtype == torch.int64
    assert s.is_cuda and m.is_cuda and k.is_cuda
    return s.cpu().numpy(), m.cpu().numpy(), k.cpu().numpy()


def check_exact(bs, seeds, empties):
    games = [R.position(s, empties, bs)[0] for s in seeds]
    score, move, nodes = gpu_solve(games, bs)
    for i, s in enumerate(seeds):
        hs, hm, hk = R.solved(s, empties, bs)
        assert (score[i], move[i]) == (hs, hm), (bs, empties, s, score[i], move[i], hs, hm)
        assert 1 <= nodes[i] <= hk, (bs, empties, s, nodes[i], hk)
        # node for node the host's fail-soft search in index order with the open window
        want = W.window_ab_seed(s, empties, bs, -W.INF, W.INF)[2]
        assert nodes[i] == want, (bs, empties, s, nodes[i], want)


def quirk_roots(bs, seeds, empties):
    n = 0
    for s in seeds:
        g, _ = R.position(s, empties, bs)
        P, Q = (g.black, g.white) if g.side == 1 else (g.white, g.black)
        n += (not g.over) and R.mover_mask(g, bs) != R.standard_legal(P, Q, bs)
    return n


def test_exact_8x8():
    # a standard-rules solver cannot pass: 24 of these roots have another legal mask than
    # standard Othello's
    assert quirk_roots(8, range(64), 6) >= 16
    check_exact(8, range(64), 6)
    check_exact(8, range(16), 8)


def test_exact_6x6():
    assert quirk_roots(6, range(64), 6) >= 16
    check_exact(6, range(64), 6)


def test_batch_shape_independence():
    """A row's answer and node count do not depend on the batch it is in: size 1, 63, 65 and 130
    batches built by repeating and permuting the 64 rows, once more on another stream."""
    games = [R.position(s, 6, 8)[0] for s in range(64)]
    base = gpu_solve(games, 8)
    rng = np.random.RandomState(5)

    def check(n):
        idx = np.concatenate([rng.permutation(64) for _ in range(-(-n // 64))])[:n]
        got = gpu_solve([games[i] for i in idx], 8)
        for a, b in zip(got, base):
            assert np.array_equal(a, b[idx]), n

    for n in (1, 63, 65, 130):
        check(n)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        check(130)
    side.synchronize()


@pytest.mark.parametrize("bs,seeds", [(8, (12, 25)), (6, (9, 15))])
def test_root_cases(bs, seeds):
    c = R.RootCases(bs, seeds)
    want = gpu_solve(c.plain, bs)
    score, move, nodes = gpu_solve(c.mixed, bs, max_empties=6)
    for got, w in zip((score, move, nodes), want):
        assert np.array_equal(got[c.keep], w)
    for i in c.keep:
        assert nodes[i] == W.window_ab(c.mixed[i], bs, -W.INF, W.INF)[2], i
    for i, j in c.where.items():
        assert (score[i], move[i]) == c.expect[j][:2], (j, score[i], move[i], c.expect[j])
        if move[i] in (-3, -5):
            assert nodes[i] == 0
        elif move[i] == bs * bs:            # a pass root
            assert nodes[i] == W.window_ab(c.mixed[i], bs, -W.INF, W.INF)[2], j
        else:
            assert nodes[i] >= 1
    s0, m0, _ = gpu_solve(c.zero, bs, max_empties=0)
    c.check_zero(bs, s0, m0)


def test_node_limit():
    games = [R.position(s, 6, 8)[0] for s in range(64)] + [R.position(3, 0, 8)[0]]
    score, move, nodes = gpu_solve(games, 8)
    again = gpu_solve(games, 8, node_limit=int(nodes.max()))
    for a, b in zip(again, (score, move, nodes)):
        assert np.array_equal(a, b)
    i = int(np.argmax(nodes > 1))
    assert nodes[i] > 1
    s1, m1, k1 = gpu_solve([games[i]], 8, node_limit=int(nodes[i]))
    assert (s1[0], m1[0], k1[0]) == (score[i], move[i], nodes[i])
    s1, m1, k1 = gpu_solve([games[i]], 8, node_limit=int(nodes[i]) - 1)
    assert (s1[0], m1[0]) == (0, -4)
    # one position per row: only a root that is over has an answer
    s1, m1, _ = gpu_solve(games, 8, node_limit=1)
    assert list(m1[:64]) == [-4] * 64 and not s1[:64].any()
    assert (s1[64], m1[64]) == (score[64], -2) and move[64] == -2


def test_deeper_roots_against_host_alphabeta():
    """10 empties on 8x8: brute force is too slow on the host, so the reference is an alpha-beta
    whose root children get the full window (about 5 s for these four rows)."""
    seeds = range(4)
    games = [R.position(s, 10, 8)[0] for s in seeds]
    score, move, nodes = gpu_solve(games, 8)
    for i, g in enumerate(games):
        hs, hm = R.alphabeta(g, 8)
        assert (score[i], move[i]) == (hs, R.expected_move(g, hm, 8)), i
        assert nodes[i] >= 1


def test_api_errors():
    import rvz
    from rvz._lib import RVZ_SOLVE_MAX_EMPTIES
    lib = rvz.load()
    EINVAL = -22
    games = [R.position(s, 6, 8)[0] for s in range(4)]
    b, w, st = R.to_device(games)
    sc = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    mv = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    nd = torch.full((4,), 77, dtype=torch.int64, device="cuda")
    p = [t.data_ptr() for t in (b, w, st, sc, mv, nd)]

    def call(bs=8, n=4, me=6, limit=1000, ptrs=p):
        return lib.rvz_solve(bs, n, ptrs[0], ptrs[1], ptrs[2], me, limit, ptrs[3], ptrs[4],
                             ptrs[5], None)

    for bs in (7, 0, 10):
        assert call(bs=bs) == EINVAL
    assert call(n=-1) == EINVAL
    assert call(me=-1) == EINVAL and call(me=RVZ_SOLVE_MAX_EMPTIES + 1) == EINVAL
    assert call(limit=0) == EINVAL and call(limit=-5) == EINVAL
    for k in range(5):
        assert call(ptrs=[None if j == k else q for j, q in enumerate(p)]) == EINVAL
    assert call(n=0) == 0 and call(n=0, ptrs=[None] * 6) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in (sc, mv, nd))        # nothing was launched
    with pytest.raises(rvz.RvzError):
        rvz.solve(b, w, st, 8, RVZ_SOLVE_MAX_EMPTIES + 1)
    with pytest.raises(rvz.RvzError):
        rvz.solve(b, w, st, 8, 6, 0)
    s0, m0, k0 = rvz.solve(b[:0], w[:0], st[:0], 8)
    assert s0.numel() == m0.numel() == k0.numel() == 0
    # out_nodes is nullable
    assert call(me=RVZ_SOLVE_MAX_EMPTIES, limit=BIG, ptrs=p[:5] + [None]) == 0
    torch.cuda.synchronize()
    assert [int(x) for x in mv.cpu()] == [R.solved(s, 6, 8)[1] for s in range(4)]
    assert bool((nd == 77).all())


def test_engine_solve():
    import rvz
    games = [R.position(s, 6, 8)[0] for s in range(16)]
    b, w, st = R.to_device(games)
    eng = rvz.Engine(16, num_simulations=16, batch_size=16, device="cuda:0")
    eng.set_state(b, w, st)
    before = [t.clone() for t in eng.get_state()]
    got = eng.solve(8, node_limit=BIG)
    want = rvz.solve(b, w, st, 8, 8, BIG)
    for a, c in zip(got, want):
        assert torch.equal(a, c)
    assert [int(x) for x in got[0].cpu()] == [R.solved(s, 6, 8)[0] for s in range(16)]
    for a, c in zip(before, eng.get_state()):
        assert torch.equal(a, c)
    eng.check()


def test_trainer_hook():
    """SelfPlayTrainer(exact_endgame=6) against exact_endgame=0, same net and seeds: states and
    policy targets bit-equal; value targets differ only on rows with at most 6 empties, where
    they are the sign of the host negamax, and at least one target really changes.
    48 simulations at batch 16, seed base 0. At 32 simulations a search is two leaf batches, so
    every policy is one-hot (mcts.py:96-97): the 8 games are one game whatever the seed base, and
    in 84 such games tried (net seeds 0..71, and seed bases 0..11 with root noise) no late
    blunder flipped a winner, so no target changed. Three batches make the moves sampled and the
    games distinct; the first seed base, 0, then changes 8 of the 48 late targets."""
    import copy

    import rvz
    from rvz.pipeline import SelfPlayTrainer
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(6, 1, 64).cuda()
    kw = dict(games=8, num_simulations=48, batch_size=16, seed=0, train_steps=1, train_batch=16)
    off = SelfPlayTrainer(copy.deepcopy(net), exact_endgame=0, **kw)
    on = SelfPlayTrainer(copy.deepcopy(net), exact_endgame=6, **kw)
    d0, d1 = off.generate(), on.generate()
    assert set(d0) == {"states", "policy_targets", "value_targets"}
    assert torch.equal(d0["states"], d1["states"])
    assert torch.equal(d0["policy_targets"], d1["policy_targets"])
    assert d1["value_targets"].dtype == torch.float32 and d1["value_targets"].shape == \
        d0["value_targets"].shape
    run = on.runner
    live = (run.rec_idx >= 0).t().reshape(-1).cpu().numpy()
    rb = run.rec_black.t().reshape(-1).cpu().numpy()[live].view(np.uint64)
    rw = run.rec_white.t().reshape(-1).cpu().numpy()[live].view(np.uint64)
    rs = run.rec_side.t().reshape(-1).cpu().numpy()[live]
    v0 = d0["value_targets"].reshape(-1).cpu().numpy()
    v1 = d1["value_targets"].reshape(-1).cpu().numpy()
    assert len(rb) == len(v0) == len(v1)
    late = changed = 0
    for i in range(len(rb)):
        g = R.O.Game(int(rb[i]), int(rw[i]), int(rs[i]), 0, -1, 0)
        if R.empties(g, 6) <= 6:
            late += 1
            assert v1[i] == np.sign(R.negamax(g, 6)[0]), i
            changed += v1[i] != v0[i]
        else:
            assert v1[i] == v0[i], i
    assert late >= 8 and changed >= 1, (late, changed)
    assert d1["exact_rows"].dim() == 0 and d1["exact_unsolved"].dim() == 0
    assert int(d1["exact_rows"]) == late and int(d1["exact_unsolved"]) == 0
    r = on.run_iteration()                 # iteration 0 again: the same games
    assert r["exact_rows"] == late and r["exact_unsolved"] == 0
    r = off.run_iteration()
    assert r["exact_rows"] == 0 and r["exact_unsolved"] == 0


@pytest.mark.parametrize("bs", [8, 6])
def test_synthetic_rows(bs):
    """Positions no playout reaches (solve_ref.synthetic_rows: the synthetic fixture's rows with
    at most 7 empties, both sides to move, and the 6x6 twin): score and move equal the unpruned
    negamax, and rvz_solve (full window, index order) visits no more positions than it."""
    R.check_synthetic_kinds(bs)
    games, host = R.synthetic_rows(bs), R.synthetic_solved(bs)
    score, move, nodes = gpu_solve(games, bs, max_empties=R.SYNTHETIC_MAX_EMPTIES)
    for i, (g, (hs, hm, hk)) in enumerate(zip(games, host)):
        assert (score[i], move[i]) == (hs, R.expected_move(g, hm, bs)), \
            (bs, i, g.astuple(), score[i], move[i], hs, hm)
        assert 1 <= nodes[i] <= hk, (bs, i, g.astuple(), nodes[i], hk)
        assert nodes[i] == W.window_ab(g, bs, -W.INF, W.INF)[2], (bs, i, g.astuple())
    # max_empties = 0: the empty board and the one-colour boards with one empty square are not
    # searched (-3), a full board is
    nsq = bs * bs
    full = (1 << nsq) - 1
    zero = [R.O.Game(0, 0, 1, 0, -1, 0), R.O.Game(full ^ 1, 0, 2, 0, -1, 0),
            R.O.Game(0, full ^ 1 << nsq - 1, 1, 0, -1, 1), R.O.Game(full, 0, 2, 0, -1, 0)]
    s0, m0, k0 = gpu_solve(zero, bs, max_empties=0)
    assert list(m0[:3]) == [-3] * 3 and not s0[:3].any() and not k0[:3].any()
    hs, hm, hk = R.negamax(zero[3], bs)
    assert hm == -1 and (s0[3], m0[3]) == (hs, nsq) == (-nsq, nsq) and 1 <= k0[3] <= hk
