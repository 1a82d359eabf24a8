"""rvz_solve_moves (csrc/rvz_solve.hip: k_solve_moves), the value of every root move, on the GPU
against the host reference of tests/solve_moves_ref.py (the definition applied literally:
make_move per legal square, then the windowed reference on the child) and, with move ordering on,
against rvz.solve_window called on the children built on the device."""
import copy

import numpy as np
import pytest
import torch

import solve_moves_ref as V
import solve_ref as R
import solve_window_ref as W
from test_gpu_solve_window import SETS

pytestmark = pytest.mark.gpu

BIG = 2 ** 40        # a node limit no move of these tests reaches
GARBAGE = 0x5A5A5A5A
NOT_A_MOVE, ABANDONED = V.NOT_A_MOVE, V.ABANDONED


def set_games(name):
    bs, seeds, empties, _ = SETS[name]
    return bs, [R.position(s, empties, bs)[0] for s in seeds]


def set_windows(name):
    """(-64, 64), (-1, 1) and the set's middle window of test_gpu_solve_window.py."""
    bs, seeds, empties, (lo, hi) = SETS[name]
    med = int(np.median([R.solved(s, empties, bs)[0] for s in seeds]))
    return [(-64, 64), (-1, 1), (med + lo, med + hi)]


def raw_moves(b, w, st, bs, alpha=-64, beta=64, order=0, max_empties=14, node_limit=BIG,
              stream=None, out=None):
    """lib.rvz_solve_moves into outputs pre-filled with a garbage pattern: an element the call
    does not write keeps it and fails the comparison. Returns the three device tensors."""
    import rvz
    n, npol = b.numel(), bs * bs + 1
    if out is None:
        out = (torch.empty(n, npol, dtype=torch.int32, device="cuda"),
               torch.empty(n, dtype=torch.int32, device="cuda"),
               torch.empty(n, npol, dtype=torch.int64, device="cuda"))
    for t in out:
        t.fill_(GARBAGE)
    rc = rvz.load().rvz_solve_moves(bs, n, b.data_ptr(), w.data_ptr(), st.data_ptr(), max_empties,
                                    node_limit, alpha, beta, order, out[0].data_ptr(),
                                    out[1].data_ptr(), out[2].data_ptr(), stream)
    assert rc == 0, rc
    return out


def gpu_moves(games, bs, **kw):
    out = raw_moves(*R.to_device(games), bs, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def same(got, want, what=""):
    for name, a, b in zip(("scores", "count", "nodes"), got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (what, name, bad[:4].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


@pytest.mark.parametrize("name", list(SETS))
def test_sets_ordering_off(name):
    import rvz
    bs, seeds, empties, _ = SETS[name]
    _, games = set_games(name)
    b, w, st = R.to_device(games)
    for alpha, beta in set_windows(name):
        want = V.stack([V.moves_ab_seed(s, empties, bs, alpha, beta) for s in seeds])
        same(gpu_moves(games, bs, alpha=alpha, beta=beta), want, (name, alpha, beta))
        # the Python surface is the same call
        got = rvz.solve_moves(b, w, st, bs, 14, BIG, alpha, beta)
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.int32
        assert got[2].dtype == torch.int64 and all(t.is_cuda for t in got)
        same([t.cpu().numpy() for t in got], want, (name, alpha, beta, "rvz.solve_moves"))
        if (alpha, beta) == (-1, 1):
            out, cnt, nodes = rvz.solve_moves_wld(b, w, st, bs, 14, BIG, 0)
            sc = want[0]
            assert np.array_equal(out.cpu().numpy(), np.where(sc <= ABANDONED, sc, np.sign(sc)))
            assert out.dtype == torch.int32 and np.array_equal(nodes.cpu().numpy(), want[2])
            # best_moves on device tensors: the moves of the best win / draw / loss class
            best, mask, complete = rvz.best_moves(out, cnt, -1, 1)
            assert bool(complete.all()) and mask.is_cuda
            for i, s in enumerate(seeds):
                values = W.child_values_seed(s, empties, bs)
                top = max(np.sign(m) for m in values.values())
                assert int(best[i]) == top
                assert [j for j in range(bs * bs + 1) if mask[i, j]] == \
                    [j for j, m in values.items() if np.sign(m) == top], (name, s)


def composition(b, w, st, bs, max_empties, node_limit, alpha, beta, order):
    """The per-move answer built from the public pieces: the children by rvz.board_legal and
    rvz.board_apply, rvz.solve_window on them with the mapped windows. Rows must be live roots
    with a legal square. Returns (row, sq, score, nodes) per child, score in the root's terms."""
    import rvz
    legal = rvz.board_legal(b, w, st, bs)
    bits = torch.arange(64, dtype=torch.int64, device=b.device)
    row, sq = torch.nonzero((legal.unsqueeze(1) >> bits) & 1, as_tuple=True)
    cb, cw, cs = b[row].contiguous(), w[row].contiguous(), st[row].contiguous()
    assert bool((rvz.board_apply(cb, cw, cs, sq.to(torch.int32), bs) != 0).all())
    kept = cs[:, 0] == st[row, 0]                  # auto-pass, or the game is over
    score = torch.empty_like(sq, dtype=torch.int32)
    nodes = torch.empty_like(sq)
    for sel, (lo, hi), sign in ((kept, (alpha, beta), 1), (~kept, (-beta, -alpha), -1)):
        s, m, k = rvz.solve_window(cb[sel], cw[sel], cs[sel], bs, max_empties, node_limit, lo, hi,
                                   order)
        score[sel] = torch.where(m == -4, torch.full_like(s, ABANDONED), sign * s)
        nodes[sel] = k
    return row, sq, score, nodes


@pytest.mark.parametrize("name", list(SETS))
def test_ordering_on_is_solve_window_of_the_children(name):
    bs, seeds, empties, _ = SETS[name]
    _, games = set_games(name)
    b, w, st = R.to_device(games)
    kinds = set()
    for alpha, beta in set_windows(name):
        scores, count, nodes = raw_moves(b, w, st, bs, alpha=alpha, beta=beta, order=4)
        row, sq, cscore, cnodes = composition(b, w, st, bs, 14, BIG, alpha, beta, 4)
        want_s = torch.full_like(scores, NOT_A_MOVE)
        want_k = torch.zeros_like(nodes)
        want_s[row, sq] = cscore
        want_k[row, sq] = cnodes
        assert torch.equal(scores, want_s), (name, alpha, beta)
        assert torch.equal(nodes, want_k), (name, alpha, beta)
        assert torch.equal(count.long(), torch.bincount(row, minlength=len(games)))
        # and the contract against the exact values, whatever ordering visits
        sc = scores.cpu().numpy()
        for i, s in enumerate(seeds):
            for j, m in W.child_values_seed(s, empties, bs).items():
                assert V.clamp(int(sc[i, j]), alpha, beta) == V.clamp(m, alpha, beta)
        if (alpha, beta) == (-64, 64):          # ordering really changes the search
            off = raw_moves(b, w, st, bs, alpha=alpha, beta=beta, order=0)[2]
            kinds.add(bool((off != nodes).any()))
    assert kinds == {True}


def child_kinds(g, bs):
    """Which kinds of child the root's moves make: 'ends', 'autopass', 'plain'."""
    out = set()
    for sq in R.squares(R.mover_mask(g, bs)):
        c = g.copy()
        assert R.O.make_move(c, sq, bs)
        out.add("ends" if c.over else ("autopass" if c.side == g.side else "plain"))
    return out


@pytest.mark.parametrize("bs,seeds", [(8, (12, 25)), (6, (9, 15))])
def test_special_rows_in_one_batch(bs, seeds):
    c = R.RootCases(bs, seeds)
    games = list(c.mixed)
    # on the host values alone: every kind of row is in the batch
    codes = [c.expect[j][1] for j in c.where.values()]
    assert -2 in codes and -3 in codes and codes.count(-5) == (6 if bs == 6 else 4)
    assert {c.expect[j][2] for j in c.where.values() if c.expect[j][1] == bs * bs} == {True, False}
    # the sets' playouts, continued: the 6-empties sets hold no move that ends the game (the
    # first are at 1 empty) and few that make the other side pass
    pool = [R.position(s, e, bs)[0] for e in (6, 4, 3, 2, 1) for s in range(64)]
    extra = {}
    for g in pool:
        if not g.over:
            for kind in child_kinds(g, bs) & {"ends", "autopass"}:
                extra.setdefault(kind, g)
    assert set(extra) == {"ends", "autopass"}
    games += [extra["ends"], extra["autopass"]]
    for alpha, beta in ((-64, 64), (-1, 1)):
        want = V.stack([V.moves_ab(g, bs, alpha, beta, max_empties=6) for g in games])
        assert {-2, -3, -5, 1} <= set(want[1].tolist()) and want[1].max() > 1
        same(gpu_moves(games, bs, alpha=alpha, beta=beta, max_empties=6), want, (bs, alpha, beta))
    # max_empties = 0: one task per row; only full or finished boards have an answer
    want = V.stack([V.moves_ab(g, bs, -1, 1, max_empties=0) for g in c.zero])
    assert want[1].tolist()[:3] == [1, -2, -3] and want[0][0, bs * bs] > ABANDONED
    same(gpu_moves(c.zero, bs, alpha=-1, beta=1, max_empties=0), want, (bs, "zero"))


def test_node_limit_bounds_every_move_on_its_own():
    name = "8x8e6"
    bs, seeds, empties, _ = SETS[name]
    _, games = set_games(name)
    free = V.stack([V.moves_ab_seed(s, empties, bs, -64, 64) for s in seeds])
    per_move = free[2][free[2] > 0]
    limit = int(np.median(per_move))
    assert (per_move > limit).sum() >= 16 and (per_move <= limit).sum() >= 16
    want = V.stack([V.moves_ab(g, bs, -64, 64, node_limit=limit) for g in games])
    over = free[2] > limit
    assert np.array_equal(want[0][over], np.full(over.sum(), ABANDONED))
    assert np.array_equal(want[2][over], np.full(over.sum(), limit))
    assert np.array_equal(want[0][~over], free[0][~over])
    assert np.array_equal(want[2][~over], free[2][~over])
    same(gpu_moves(games, bs, node_limit=limit), want, limit)
    # node_limit 1: every searched move is abandoned at its first position, a move that ends
    # the game still scores
    want = V.stack([V.moves_ab(g, bs, -64, 64, node_limit=1) for g in games])
    same(gpu_moves(games, bs, node_limit=1), want, 1)


def test_row_independence():
    """A row's outputs do not depend on the batch: permuted and repeated batches of 1, 63, 65
    and 130 rows (not multiples of the workgroup's 128 lanes), single-row calls, another stream."""
    bs, games = set_games("8x8e6")
    rng = np.random.RandomState(5)
    for alpha, beta, order in ((-64, 64, 0), (-1, 1, 4)):
        base = gpu_moves(games, bs, alpha=alpha, beta=beta, order=order)
        for n in (1, 63, 65, 130):
            idx = np.concatenate([rng.permutation(64) for _ in range(-(-n // 64))])[:n]
            got = gpu_moves([games[i] for i in idx], bs, alpha=alpha, beta=beta, order=order)
            same(got, [a[idx] for a in base], (order, n))
        for i in (0, 17, 63):
            same(gpu_moves([games[i]], bs, alpha=alpha, beta=beta, order=order),
                 [a[i:i + 1] for a in base], (order, "single", i))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        import rvz
        got = rvz.solve_moves(*R.to_device(games), bs, 14, BIG, -1, 1, 4)
    side.synchronize()
    same([t.cpu().numpy() for t in got], base, "side stream")


def test_lanes_take_further_tasks():
    """More tasks than the launch has lanes. The grid is min(4 workgroups x CU count,
    ceil(tasks / 128)) workgroups of 128 lanes and a row makes max(1, max_empties) = 14 tasks, so
    with n > 4 * CUs * 128 / 14 rows lanes have to come back for a further task; the 64 rows are
    tiled to 1.5 times that. Every tile must equal the first."""
    bs, games = set_games("8x8e6")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lanes = 4 * cus * 128
    tiles = (3 * lanes // 2) // (14 * 64) + 1
    assert tiles * 64 * 14 > lanes
    b, w, st = (t.repeat(tiles, *([1] * (t.dim() - 1))) for t in R.to_device(games))
    out = raw_moves(b, w, st, bs, alpha=-1, beta=1, order=4)
    torch.cuda.synchronize()
    first = gpu_moves(games, bs, alpha=-1, beta=1, order=4)
    for t, f in zip(out, first):
        t = t.reshape(tiles, 64, *t.shape[1:])
        assert bool((t == torch.from_numpy(f).cuda().unsqueeze(0)).all())


def test_api_errors():
    import rvz
    lib = rvz.load()
    EINVAL = -22
    bs, games = 8, [R.position(s, 6, 8)[0] for s in range(4)]
    b, w, st = R.to_device(games)
    sc = torch.full((4, 65), 77, dtype=torch.int32, device="cuda")
    cn = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    nd = torch.full((4, 65), 77, dtype=torch.int64, device="cuda")
    p = [t.data_ptr() for t in (b, w, st, sc, cn, nd)]

    def call(bs=8, n=4, me=6, limit=1000, alpha=-1, beta=1, order=0, ptrs=p):
        return lib.rvz_solve_moves(bs, n, ptrs[0], ptrs[1], ptrs[2], me, limit, alpha, beta,
                                   order, ptrs[3], ptrs[4], ptrs[5], None)

    assert call(bs=7) == EINVAL and call(n=-1) == EINVAL
    assert call(me=15) == EINVAL and call(me=-1) == EINVAL
    assert call(limit=0) == EINVAL and call(order=-1) == EINVAL
    for alpha, beta in ((0, 0), (1, -1), (-65, 0), (0, 65)):
        assert call(alpha=alpha, beta=beta) == EINVAL
    for k in range(5):            # black, white, status, out_scores, out_count
        assert call(ptrs=[None if j == k else q for j, q in enumerate(p)]) == EINVAL
    assert call(n=(2 ** 31 - 1) // 65 + 1) == EINVAL          # n * (S*S + 1) past int32
    assert call(bs=6, n=(2 ** 31 - 1) // 37 + 1) == EINVAL
    assert call(n=0) == 0 and call(n=0, ptrs=[None] * 6) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in (sc, cn, nd))        # nothing was launched
    for kw in (dict(alpha=3, beta=3), dict(alpha=-65), dict(beta=65), dict(order_min_empties=-1),
               dict(max_empties=15), dict(node_limit=0)):
        with pytest.raises(rvz.RvzError):
            rvz.solve_moves(b, w, st, 8, **kw)
    with pytest.raises(rvz.RvzError):
        rvz.solve_moves_wld(b, w, st, 8, order_min_empties=-1)
    with pytest.raises(rvz.RvzError):
        rvz.solve_moves(b, w, st[:3], 8)
    for f in (rvz.solve_moves, rvz.solve_moves_wld):
        s0, c0, k0 = f(b[:0], w[:0], st[:0], 8)
        assert s0.shape == k0.shape == (0, 65) and c0.shape == (0,)
    # out_nodes is nullable
    assert call(me=14, limit=BIG, ptrs=p[:5] + [None]) == 0
    torch.cuda.synchronize()
    want = V.stack([V.moves_ab_seed(s, 6, 8, -1, 1) for s in range(4)])
    assert np.array_equal(sc.cpu().numpy(), want[0]) and np.array_equal(cn.cpu().numpy(), want[1])
    assert bool((nd == 77).all())
    net = rvz.AlphaZeroNetwork(6, 1, 64).cuda()
    from rvz.pipeline import SelfPlayTrainer
    for bad in (-1, 15):
        with pytest.raises(ValueError):
            SelfPlayTrainer(net, games=4, num_simulations=16, batch_size=16, exact_policy=bad)


def test_graph_capture():
    bs, games = set_games("8x8e6")
    b, w, st = R.to_device(games)
    eager = [t.clone() for t in raw_moves(b, w, st, bs, alpha=-1, beta=1, order=4)]   # warm
    torch.cuda.synchronize()
    out = tuple(torch.empty_like(t) for t in eager)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw_moves(b, w, st, bs, alpha=-1, beta=1, order=4, out=out,
                  stream=torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        for t in out:
            t.fill_(GARBAGE + 1)
        graph.replay()
        torch.cuda.synchronize()
        for a, e in zip(out, eager):
            assert torch.equal(a, e)


def test_solve_and_solve_window_are_unchanged():
    import rvz
    bs, seeds, empties, _ = SETS["8x8e6"]
    _, games = set_games("8x8e6")
    b, w, st = R.to_device(games)
    s, m, k = (t.cpu().numpy() for t in rvz.solve(b, w, st, bs, 14, BIG))
    for i, sd in enumerate(seeds):
        assert (s[i], m[i]) == R.solved(sd, empties, bs)[:2]
        assert k[i] == W.window_ab_seed(sd, empties, bs, -W.INF, W.INF)[2]
    s, m, k = (t.cpu().numpy() for t in rvz.solve_window(b, w, st, bs, 14, BIG, -1, 1))
    for i, sd in enumerate(seeds):
        assert (s[i], m[i], k[i]) == W.window_ab_seed(sd, empties, bs, -1, 1)


def test_engine_solve_moves():
    import rvz
    games = [R.position(s, 6, 8)[0] for s in range(16)]
    b, w, st = R.to_device(games)
    eng = rvz.Engine(16, num_simulations=16, batch_size=16, device="cuda:0")
    eng.set_state(b, w, st)
    before = [t.clone() for t in eng.get_state()]
    got = eng.solve_moves(8, node_limit=BIG)
    same([t.cpu().numpy() for t in got],
         V.stack([V.moves_ab_seed(s, 6, 8, -64, 64) for s in range(16)]))
    for order in (None, 0):
        got = eng.solve_moves_wld(8, node_limit=BIG, order_min_empties=order)
        want = rvz.solve_moves_wld(b, w, st, 8, 8, BIG, **({} if order is None else
                                                            {"order_min_empties": order}))
        for a, c in zip(got, want):
            assert torch.equal(a, c)
        sc = V.stack([V.moves_ab_seed(s, 6, 8, -1, 1) for s in range(16)])[0]
        assert np.array_equal(got[0].cpu().numpy(), np.where(sc <= ABANDONED, sc, np.sign(sc)))
    for a, c in zip(before, eng.get_state()):
        assert torch.equal(a, c)
    eng.check()


def test_trainer_exact_policy():
    """SelfPlayTrainer(exact_policy=6) against exact_policy=0 on 6x6, same net and seeds (the
    setting of test_gpu_solve.py's trainer test): states and value targets bit-equal; the policy
    rows with at most 6 empties are uniform over the host's best moves, every other row is the
    MCTS target bit for bit, and at least one row's argmax really changes."""
    import rvz
    from rvz.pipeline import SelfPlayTrainer
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(6, 1, 64).cuda()
    kw = dict(games=8, num_simulations=48, batch_size=16, seed=0, train_steps=1, train_batch=16)
    off = SelfPlayTrainer(copy.deepcopy(net), exact_policy=0, **kw)
    on = SelfPlayTrainer(copy.deepcopy(net), exact_policy=6, exact_node_limit=BIG, **kw)
    d0, d1 = off.generate(), on.generate()
    assert set(d0) == {"states", "policy_targets", "value_targets"}
    assert set(d1) == set(d0) | {"exact_policy_rows", "exact_policy_unsolved"}
    assert torch.equal(d0["states"], d1["states"])
    assert torch.equal(d0["value_targets"], d1["value_targets"])
    run = on.runner
    live = (run.rec_idx >= 0).t().reshape(-1).cpu().numpy()
    rb = run.rec_black.t().reshape(-1).cpu().numpy()[live].view(np.uint64)
    rw = run.rec_white.t().reshape(-1).cpu().numpy()[live].view(np.uint64)
    rs = run.rec_side.t().reshape(-1).cpu().numpy()[live]
    p0, p1 = d0["policy_targets"].cpu(), d1["policy_targets"].cpu()
    assert p1.dtype == torch.float32 and p1.shape == p0.shape and len(rb) == len(p0)
    late = changed = 0
    for i in range(len(rb)):
        g = R.O.Game(int(rb[i]), int(rw[i]), int(rs[i]), 0, -1, 0)
        if R.empties(g, 6) <= 6:
            late += 1
            values = W.child_values(g, 6)
            top = max(values.values())
            want = torch.zeros(37)
            best = [j for j, m in values.items() if m == top]
            want[best] = 1.0 / len(best)
            assert torch.equal(p1[i], want), i
            changed += int(p0[i].argmax()) not in best
        else:
            assert torch.equal(p1[i], p0[i]), i
    assert late >= 8 and changed >= 1, (late, changed)
    assert d1["exact_policy_rows"].dim() == 0 and d1["exact_policy_unsolved"].dim() == 0
    assert int(d1["exact_policy_rows"]) == late and int(d1["exact_policy_unsolved"]) == 0


@pytest.mark.parametrize("bs", [8, 6])
def test_synthetic_rows(bs):
    """Every entry of rvz_solve_moves on solve_ref.synthetic_rows (positions no playout reaches)
    against solve_moves_ref.moves_ab, at (-64, 64) and (-1, 1)."""
    R.check_synthetic_kinds(bs)
    games = R.synthetic_rows(bs)
    me = R.SYNTHETIC_MAX_EMPTIES
    for alpha, beta in ((-64, 64), (-1, 1)):
        want = V.stack([V.moves_ab(g, bs, alpha, beta, max_empties=me) for g in games])
        same(gpu_moves(games, bs, alpha=alpha, beta=beta, max_empties=me), want,
             (bs, alpha, beta))
    nsq = bs * bs
    empty = [R.O.Game(0, 0, 1, 0, -1, 0)]
    scores, count, nodes = gpu_moves(empty, bs, max_empties=0)
    assert count[0] == -3 and (scores == NOT_A_MOVE).all() and not nodes.any()
    scores, count, nodes = gpu_moves(empty, bs, max_empties=14)
    assert count[0] == -3                              # 36 or 64 empties: above any max_empties
    assert scores.shape == (1, nsq + 1)
