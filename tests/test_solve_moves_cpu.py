"""The per-move endgame solve's host side, without a GPU: the host reference of
tests/solve_moves_ref.py against the unpruned negamax and the windowed reference, rvz.best_moves
on CPU tensors, records_to_training's exact_policy hook with an injected host solver, and
rvz_solve_moves' argument refusals (checked before any HIP call)."""
import numpy as np
import pytest
import torch

import solve_moves_ref as V
import solve_ref as R
import solve_window_ref as W
from test_gpu_solve_window import SETS
from test_solve_cpu import _train

NOT_A_MOVE, ABANDONED = V.NOT_A_MOVE, V.ABANDONED


def middle_window(name):
    bs, seeds, empties, (lo, hi) = SETS[name]
    med = int(np.median([R.solved(s, empties, bs)[0] for s in seeds]))
    return med + lo, med + hi


@pytest.mark.parametrize("name", list(SETS))
def test_reference_consistency(name):
    """At the full window every entry is the move's exact value; their maximum and its lowest
    index are rvz_solve's answer."""
    bs, seeds, empties, _ = SETS[name]
    for s in seeds:
        g, _ = R.position(s, empties, bs)
        scores, count, nodes = V.moves_ab_seed(s, empties, bs, -64, 64)
        values = W.child_values_seed(s, empties, bs)
        assert count == len(values) >= 1, (name, s)
        assert {i: x for i, x in enumerate(scores) if x != NOT_A_MOVE} == values, (name, s)
        assert all((k >= 1) == (i in values) for i, k in enumerate(nodes)), (name, s)
        best = max(values.values())
        assert (best, min(i for i, x in values.items() if x == best)) == \
            R.solved(s, empties, bs)[:2], (name, s)


@pytest.mark.parametrize("name", list(SETS))
def test_clamp_property(name):
    """clamp(entry) == clamp(exact value) at (-1, 1) and the set's middle window; some moves
    really lie below, inside (the middle window) and above."""
    bs, seeds, empties, _ = SETS[name]
    for alpha, beta in ((-1, 1), middle_window(name)):
        kinds = set()
        for s in seeds:
            scores, count, _ = V.moves_ab_seed(s, empties, bs, alpha, beta)
            values = W.child_values_seed(s, empties, bs)
            assert count == len(values)
            for i, x in enumerate(scores):
                if i not in values:
                    assert x == NOT_A_MOVE
                    continue
                m = values[i]
                assert V.clamp(x, alpha, beta) == V.clamp(m, alpha, beta), (name, s, i, x, m)
                if alpha < m < beta:
                    assert x == m
                elif m <= alpha:
                    assert m <= x <= alpha
                else:
                    assert beta <= x <= m
                kinds.add((m > alpha) + (m >= beta))
        assert kinds == {0, 1, 2}, (name, alpha, beta, kinds)


def special_rows(alpha, beta, bs=8):
    """(games, max_empties, node_limit, kinds): set rows at 6 empties, then a pass root that is
    searched, one that ends the game, an over root, a row above max_empties, and a node limit
    under which the first row has an abandoned move at that window."""
    plain = [R.position(s, 6, bs)[0] for s in range(6)]
    searched, ending = None, None
    for g in R.pass_roots(bs, (12, 25)):
        for passed in (0, 1):
            c = g.copy()
            c.passed = passed
            child = c.copy()
            assert R.O.make_move(child, -1, bs)
            if child.over or R.mover_mask(child, bs) == 0:
                ending = ending or c
            else:
                searched = searched or c
    assert searched is not None and ending is not None
    over = R.position(3, 0, bs)[0]
    deep = R.position(0, 7, bs)[0]
    assert over.over and R.empties(deep, bs) == 7
    k0 = [k for k in V.moves_ab(plain[0], bs, alpha, beta)[2] if k]
    limit = sorted(k0)[len(k0) // 2] - 1
    assert min(k0) <= limit < max(k0)
    return plain + [searched, ending, over, deep], 6, limit


@pytest.mark.parametrize("alpha,beta", [(-64, 64), (-1, 1), (-6, 2)])
def test_best_moves_on_cpu_tensors(alpha, beta):
    import rvz
    games, me, limit = special_rows(alpha, beta)
    rows = [V.moves_ab(g, 8, alpha, beta, max_empties=me, node_limit=None if i else limit)
            for i, g in enumerate(games)]
    counts = [r[1] for r in rows]
    assert counts[-2:] == [-2, -3] and counts[-4:-2] == [1, 1]
    assert ABANDONED in rows[0][0] and any(x > ABANDONED for x in rows[0][0])
    assert any(ABANDONED not in r[0] and r[1] > 1 for r in rows)
    scores, count, _ = (torch.from_numpy(a) for a in V.stack(rows))
    best, mask, complete = rvz.best_moves(scores, count, alpha, beta)
    assert best.dtype == torch.int32 and mask.dtype == torch.bool and complete.dtype == torch.bool
    assert mask.shape == scores.shape and best.shape == complete.shape == count.shape
    for i, (s, c, _) in enumerate(rows):
        hb, hm, hc = V.host_best_moves(s, c, alpha, beta)
        assert (int(best[i]), [bool(x) for x in mask[i]], bool(complete[i])) == (hb, hm, hc), i
    assert not bool(complete[0]) and bool(complete[1]) and bool(complete[-3])
    assert not bool(complete[-1]) and not bool(complete[-2])
    assert [bool(x) for x in mask[-4]] == [False] * 64 + [True]         # a pass root
    # at the full window the mask is the set of best moves, its first index rvz_solve's move
    if (alpha, beta) == (-64, 64):
        for i in range(1, 6):
            v, m, _ = R.solved(i, 6, 8)
            values = W.child_values_seed(i, 6, 8)
            assert int(best[i]) == v and int(mask[i].int().argmax()) == m
            assert [j for j in range(65) if mask[i, j]] == [j for j, x in values.items() if x == v]
    with pytest.raises(rvz.RvzError):
        rvz.best_moves(scores, count, 3, 3)
    assert rvz.SOLVE_NOT_A_MOVE == NOT_A_MOVE and rvz.SOLVE_ABANDONED == ABANDONED


def synthetic_records(bs=8, N=5):
    """One game column whose plies are hand-picked positions: rows within N empties, rows above,
    and a pass root; random policies. Seeds 4 and 8 have two best moves at 5 empties on 8x8."""
    late = [R.position(s, N, bs)[0] for s in (0, 1, 4, 8)] + [R.position(4, 3, bs)[0]]
    assert not any(g.over for g in late)
    early = [R.position(s, N + 2, bs)[0] for s in range(3)]
    passing = R.pass_roots(bs, (12,))[0]
    assert R.empties(passing, bs) <= N
    games = [late[0], early[0], late[1], passing, early[1], late[2], late[3], early[2], late[4]]
    P, npol = len(games), bs * bs + 1
    rng = np.random.RandomState(1)
    p = rng.dirichlet(np.ones(npol), size=P).reshape(P, 1, npol)
    b, w, st = R.to_arrays(games)
    rec = dict(rec_black=torch.from_numpy(b).reshape(P, 1),
               rec_white=torch.from_numpy(w).reshape(P, 1),
               rec_side=torch.from_numpy(st[:, 0].copy()).reshape(P, 1),
               rec_idx=torch.zeros(P, 1, dtype=torch.int32), rec_p=torch.from_numpy(p),
               final_status=torch.tensor([[1, 1, 1, 0]], dtype=torch.int32))
    return games, rec


@pytest.mark.parametrize("wld", [False, True])
def test_exact_policy_replaces_the_solved_rows(wld):
    bs, N = 8, 5
    games, rec = synthetic_records(bs, N)
    alpha, beta = (-1, 1) if wld else (-64, 64)
    abandoned = {5}
    calls = []

    def solver(b, w, st, board_size, max_empties):
        calls.append((board_size, max_empties, b.numel()))
        return V.host_moves_solver(b, w, st, board_size, max_empties, alpha, beta, abandoned)

    base = _train(rec, bs)
    off = _train(rec, bs, exact_policy=0, moves_solver=solver)
    assert not calls and set(off) == set(base) == {"states", "policy_targets", "value_targets"}
    for k in base:
        assert off[k].dtype == base[k].dtype and torch.equal(off[k], base[k]), k
    out = _train(rec, bs, exact_policy=N, moves_solver=solver, exact_wld=wld)
    assert calls == [(bs, N, len(games))]
    assert set(out) == set(base) | {"exact_policy_rows", "exact_policy_unsolved"}
    assert torch.equal(out["states"], base["states"])
    assert torch.equal(out["value_targets"], base["value_targets"])
    p0, p1 = base["policy_targets"], out["policy_targets"]
    assert p1.dtype == torch.float32 and p1.shape == p0.shape
    replaced = several = 0
    for i, g in enumerate(games):
        within = R.empties(g, bs) <= N
        if not within or i in abandoned:
            assert torch.equal(p1[i], p0[i]), i
            continue
        replaced += 1
        if R.mover_mask(g, bs) == 0:
            want = [bs * bs]
        else:
            values = W.child_values(g, bs)
            top = max(V.clamp(m, alpha, beta) for m in values.values())
            want = [sq for sq, m in values.items() if V.clamp(m, alpha, beta) == top]
            if not wld:
                assert int(p1[i].argmax()) == R.negamax(g, bs)[1]
        several += len(want) > 1
        expect = torch.zeros_like(p1[i])
        expect[want] = 1.0 / len(want)
        assert torch.equal(p1[i], expect), (i, want)
        assert abs(float(p1[i].sum()) - 1.0) < 1e-6 and int(p1[i].argmax()) == min(want)
    assert replaced == 5 and several >= 1
    for k in ("exact_policy_rows", "exact_policy_unsolved"):
        assert out[k].dim() == 0 and out[k].dtype == torch.int64
    assert int(out["exact_policy_rows"]) == replaced and int(out["exact_policy_unsolved"]) == 1
    # independent of exact_endgame: both on is each one's change
    both = _train(rec, bs, exact_policy=N, moves_solver=solver, exact_wld=wld, exact_endgame=N,
                  solver=R.host_solver)
    value = _train(rec, bs, exact_endgame=N, solver=R.host_solver)
    assert torch.equal(both["policy_targets"], p1)
    assert torch.equal(both["value_targets"], value["value_targets"])
    assert torch.equal(value["policy_targets"], p0)


def test_default_moves_solver_follows_exact_wld(monkeypatch):
    import rvz.trainer as T
    games, rec = synthetic_records()
    used = []

    def fake(name, alpha, beta):
        def f(b, w, s, board_size, max_empties, node_limit):
            used.append((name, node_limit))
            return V.host_moves_solver(b, w, s, board_size, max_empties, alpha, beta)
        return f

    monkeypatch.setattr(T, "solve_moves", fake("solve_moves", -64, 64))
    monkeypatch.setattr(T, "solve_moves_wld", fake("solve_moves_wld", -1, 1))
    a = _train(rec, 8, exact_policy=5, exact_node_limit=123)
    b = _train(rec, 8, exact_policy=5, exact_node_limit=456, exact_wld=True)
    assert used == [("solve_moves", 123), ("solve_moves_wld", 456)]
    assert int(a["exact_policy_rows"]) == int(b["exact_policy_rows"]) == 6
    # every full-window optimum is a WLD optimum
    assert bool(((a["policy_targets"] > 0) <= (b["policy_targets"] > 0)).all())


def test_rvz_solve_moves_refuses_bad_arguments_without_a_gpu():
    """The argument checks run before any HIP call: never-dereferenced pointers, no GPU."""
    import os
    import re

    import rvz
    from rvz._lib import RVZ_SOLVE_MAX_EMPTIES
    lib = rvz.load()
    EINVAL = -22
    p = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000]

    def call(bs=8, n=4, me=6, limit=1000, alpha=-1, beta=1, order=0, ptrs=p):
        return lib.rvz_solve_moves(bs, n, ptrs[0], ptrs[1], ptrs[2], me, limit, alpha, beta,
                                   order, ptrs[3], ptrs[4], ptrs[5], None)

    for bs in (7, 0, 10, -8):
        assert call(bs=bs) == EINVAL
    assert call(n=-1) == EINVAL
    assert call(me=-1) == EINVAL and call(me=RVZ_SOLVE_MAX_EMPTIES + 1) == EINVAL
    assert call(limit=0) == EINVAL and call(limit=-1) == EINVAL
    for alpha, beta in ((0, 0), (1, -1), (-65, 0), (0, 65), (64, 64), (-64, -64), (5, 4)):
        assert call(alpha=alpha, beta=beta) == EINVAL, (alpha, beta)
    assert call(order=-1) == EINVAL
    for k in range(5):            # black, white, status, out_scores, out_count
        assert call(ptrs=[None if j == k else q for j, q in enumerate(p)]) == EINVAL
    # n * (S*S + 1) must fit in int32
    assert call(bs=8, n=(2 ** 31 - 1) // 65 + 1) == EINVAL
    assert call(bs=6, n=(2 ** 31 - 1) // 37 + 1) == EINVAL
    for bs in (6, 8):
        assert call(bs=bs, n=0) == 0 and call(bs=bs, n=0, ptrs=[None] * 6) == 0
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "include", "rvz.h")).read()
    assert int(re.search(r"#define RVZ_SOLVE_NOT_A_MOVE \((-\d+)\)", hdr).group(1)) == NOT_A_MOVE
    assert int(re.search(r"#define RVZ_SOLVE_ABANDONED \((-\d+)\)", hdr).group(1)) == ABANDONED
    for f in (rvz.solve_moves, rvz.solve_moves_wld, rvz.best_moves, rvz.Engine.solve_moves,
              rvz.Engine.solve_moves_wld):
        assert callable(f)
    from rvz.pipeline import SelfPlayTrainer
    import inspect
    assert inspect.signature(SelfPlayTrainer.__init__).parameters["exact_policy"].default == 0
