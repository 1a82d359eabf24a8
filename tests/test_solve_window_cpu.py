"""The windowed / WLD endgame solve's host side, without a GPU: the host reference of
tests/solve_window_ref.py against the unpruned negamax (bounds, move rule, and the nesting
property: a narrower window never visits more positions in the same move order), adjudicate and
records_to_training(exact_wld=...) with injected host solvers, and rvz_solve_window's argument
refusals (checked before any HIP call)."""
import numpy as np
import pytest
import torch

import solve_ref as R
import solve_window_ref as W
from test_solve_cpu import _train, played_records

SETS = [(8, range(64), 6), (6, range(64), 6)]


def windows(scores):
    med = int(np.median(scores))
    return [(-1, 1), (-64, 64), (med, med + 1), (med - 8, med - 2), (med + 2, 64)]


@pytest.mark.parametrize("bs,seeds,empties", SETS)
def test_host_window_reference(bs, seeds, empties):
    scores = [R.solved(s, empties, bs)[0] for s in seeds]
    for s in seeds:
        g, _ = R.position(s, empties, bs)
        v, vm, _ = R.solved(s, empties, bs)
        values = W.child_values_seed(s, empties, bs)
        full = W.window_ab_seed(s, empties, bs, -W.INF, W.INF)
        assert full[:2] == (v, vm), (bs, s)            # rvz_solve's own search
        for alpha, beta in windows(scores):
            r, move, nodes = W.window_ab_seed(s, empties, bs, alpha, beta)
            W.check_result(g, bs, alpha, beta, v, r, move, values)
            if 0 <= move < bs * bs:                    # the lowest qualifying square
                ok = [sq for sq, m in sorted(values.items())
                      if ((m == v) if r < beta else (m >= beta))]
                assert move == ok[0], (bs, s, alpha, beta, move, ok)
            if alpha < v < beta:
                assert move == vm, (bs, s, alpha, beta)
            if (alpha, beta) == (-1, 1):
                assert np.sign(r) == np.sign(v)
            # the nesting argument: same move order, narrower window, no more nodes
            assert 1 <= nodes <= full[2], (bs, s, alpha, beta, nodes, full[2])


def test_host_window_reference_root_cases():
    over, _ = R.position(3, 0, 8)
    assert W.window_ab(over, 8, -1, 1) == (R.discs_diff(over), -2, 1)
    g = R.last_auto_pass(25, 0, 8)
    g.side = 3 - g.side
    for passed in (0, 1):
        g.passed = passed
        v, m, k = R.negamax(g, 8)
        assert m == -1
        for alpha, beta in ((-1, 1), (-64, 64), (v, v + 1), (v - 1, v)):
            r, move, nodes = W.window_ab(g, 8, alpha, beta)
            W.check_result(g, 8, alpha, beta, v, r, move)
            assert move == 64 and 2 <= nodes <= k


def host_wld(black, white, status, board_size, max_empties, unsolved=()):
    score, move, nodes = R.host_solver(black, white, status, board_size, max_empties, unsolved)
    return torch.sign(score), move, nodes


def _adjudicate_case(bs):
    live = [R.position(s, 6, bs)[0] for s in range(8)]
    over = [R.position(s, 0, bs)[0] for s in (3, 4)]
    assert all(not g.over and R.empties(g, bs) == 6 for g in live) and all(g.over for g in over)
    games = live[:3] + over[:1] + live[3:] + over[1:]
    b, w, st = (torch.from_numpy(a) for a in R.to_arrays(games))
    return games, b, w, st


@pytest.mark.parametrize("bs", [8, 6])
def test_adjudicate(bs):
    from rvz.trainer import adjudicate
    games, b, w, st = _adjudicate_case(bs)
    unsolved = 5
    assert not games[unsolved].over
    calls = []

    def solver(bb, ww, ss, board_size, max_empties):
        calls.append((board_size, max_empties, bb.numel()))
        return host_wld(bb, ww, ss, board_size, max_empties, unsolved={unsolved})

    before = st.clone()
    final, keep, stats = adjudicate(b, w, st, bs, solver=solver)
    assert calls == [(bs, 14, len(games))]
    assert torch.equal(st, before)                       # the input is not edited
    assert final.dtype == torch.int32 and final.shape == (len(games), 4)
    assert keep.dtype == torch.bool and keep.shape == (len(games),)
    winners = set()
    for i, g in enumerate(games):
        row = [int(x) for x in final[i]]
        if g.over:
            assert row == [g.side, 1, g.winner, g.passed] and bool(keep[i])
        elif i == unsolved:
            assert not bool(keep[i]) and row == [g.side, 0, g.winner, g.passed]
        else:
            v = R.negamax(g, bs)[0]
            want = g.side if v > 0 else (3 - g.side if v < 0 else 0)
            assert row == [g.side, 1, want, g.passed] and bool(keep[i]), (i, row, v)
            winners.add(want)
    assert len(winners) >= 2                             # both colours win somewhere
    assert all(stats[k].dim() == 0 and stats[k].dtype == torch.int64 for k in stats)
    assert {k: int(x) for k, x in stats.items()} == {
        "adjudicated": 7, "adjudicate_unsolved": 1, "already_over": 2}
    # a solver returning scores (records_to_training's convention) gives the same answer
    f2, k2, s2 = adjudicate(b, w, st, bs, solver=lambda *a: R.host_solver(*a, unsolved={unsolved}))
    assert torch.equal(f2, final) and torch.equal(k2, keep)


def test_adjudicate_refuses_deep_games():
    from rvz.trainer import adjudicate
    games = [R.position(0, 6, 8)[0], R.position(1, 15, 8)[0]]
    assert R.empties(games[1], 8) == 15
    b, w, st = (torch.from_numpy(a) for a in R.to_arrays(games))
    with pytest.raises(ValueError):
        adjudicate(b, w, st, 8, solver=host_wld)
    # unchecked, the deep game is dropped instead
    final, keep, stats = adjudicate(b, w, st, 8, solver=host_wld, check_depth=False)
    assert [bool(k) for k in keep] == [True, False] and int(stats["adjudicated"]) == 1
    assert int(final[1, 1]) == 0


@pytest.mark.parametrize("bs,N", [(8, 5), (6, 6)])
def test_exact_wld_gives_the_same_targets(bs, N, monkeypatch):
    import rvz.trainer as T
    rec = played_records(range(4), bs)
    base = _train(rec, bs, exact_endgame=N, solver=R.host_solver)
    wld = _train(rec, bs, exact_endgame=N, solver=host_wld, exact_wld=True)
    assert set(base) == set(wld)
    for k in base:
        assert base[k].dtype == wld[k].dtype and torch.equal(base[k], wld[k]), k
    # without an injected solver, exact_wld chooses between the module's two solvers
    used = []

    def fake(name, fn):
        def f(b, w, s, board_size, max_empties, node_limit):
            used.append((name, node_limit))
            return fn(b, w, s, board_size, max_empties)
        return f

    monkeypatch.setattr(T, "solve", fake("solve", R.host_solver))
    monkeypatch.setattr(T, "solve_wld", fake("solve_wld", host_wld))
    a = _train(rec, bs, exact_endgame=N, exact_node_limit=123)
    b = _train(rec, bs, exact_endgame=N, exact_node_limit=456, exact_wld=True)
    assert used == [("solve", 123), ("solve_wld", 456)]
    for k in base:
        assert torch.equal(a[k], base[k]) and torch.equal(b[k], base[k]), k
    # exact_wld alone (exact_endgame off) changes nothing
    off = _train(rec, bs, exact_wld=True)
    assert set(off) == {"states", "policy_targets", "value_targets"} and len(used) == 2


def test_rvz_solve_window_refuses_bad_arguments_without_a_gpu():
    """The argument checks run before any HIP call: never-dereferenced pointers, no GPU."""
    import rvz
    from rvz._lib import RVZ_SOLVE_MAX_EMPTIES
    lib = rvz.load()
    EINVAL = -22
    p = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000]

    def call(bs=8, n=4, me=6, limit=1000, alpha=-1, beta=1, order=0, ptrs=p):
        return lib.rvz_solve_window(bs, n, ptrs[0], ptrs[1], ptrs[2], me, limit, alpha, beta,
                                    order, ptrs[3], ptrs[4], ptrs[5], None)

    for bs in (7, 0, 10, -8):
        assert call(bs=bs) == EINVAL
    assert call(n=-1) == EINVAL
    assert call(me=-1) == EINVAL and call(me=RVZ_SOLVE_MAX_EMPTIES + 1) == EINVAL
    assert call(limit=0) == EINVAL and call(limit=-1) == EINVAL
    for alpha, beta in ((0, 0), (1, -1), (-65, 0), (0, 65), (64, 64), (-64, -64), (5, 4)):
        assert call(alpha=alpha, beta=beta) == EINVAL, (alpha, beta)
    assert call(order=-1) == EINVAL
    for k in range(5):
        assert call(ptrs=[None if j == k else q for j, q in enumerate(p)]) == EINVAL
    for bs in (6, 8):
        for alpha, beta in ((-64, 64), (-1, 1), (63, 64), (-64, -63)):
            assert call(bs=bs, n=0, alpha=alpha, beta=beta, order=7) == 0
        assert call(bs=bs, n=0, ptrs=[None] * 6) == 0
    assert callable(rvz.solve_window) and callable(rvz.solve_wld)
    assert callable(rvz.Engine.solve_wld)
