"""The exact endgame solver's host side, without a GPU: records_to_training's exact_endgame hook
with an injected host solver, rvz_solve's argument refusals (checked before any HIP call), and a
self-check of the host reference the GPU tests compare against (tests/solve_ref.py)."""
import random

import numpy as np
import pytest
import torch

import solve_ref as R


def _oracle_canonical(black, white, status, bs):
    O = R.O
    out = np.zeros((black.numel(), 3, bs, bs), np.float32)
    b, w, s = black.numpy().view(np.uint64), white.numpy().view(np.uint64), status.numpy()
    for i in range(len(b)):
        out[i] = O.canonical(O.Game(int(b[i]), int(w[i]), int(s[i, 0])), bs)
    return torch.from_numpy(out)


def played_records(seeds, bs=8):
    """Random playouts recorded in the engine's layout ([plies, G] black / white / side / move /
    policy, final status [G, 4]); a game shorter than the longest leaves -2 in rec_idx."""
    O = R.O
    P, G, npol = bs * bs - 4, len(seeds), bs * bs + 1
    black, white = np.zeros((P, G), np.uint64), np.zeros((P, G), np.uint64)
    side, idx = np.zeros((P, G), np.int32), np.full((P, G), -2, np.int32)
    p = np.zeros((P, G, npol))
    final = np.zeros((G, 4), np.int32)
    for j, seed in enumerate(seeds):
        rng = random.Random(seed)
        g = O.new_game(bs)
        k = 0
        while not g.over:
            black[k, j], white[k, j], side[k, j] = g.black, g.white, g.side
            sq = rng.choice(list(R.squares(R.mover_mask(g, bs))))
            idx[k, j] = sq
            p[k, j, sq] = 1.0
            assert O.make_move(g, sq, bs)
            k += 1
        final[j] = (g.side, g.over, g.winner, g.passed)
    return dict(rec_black=torch.from_numpy(black.view(np.int64)),
                rec_white=torch.from_numpy(white.view(np.int64)),
                rec_side=torch.from_numpy(side), rec_idx=torch.from_numpy(idx),
                rec_p=torch.from_numpy(p), final_status=torch.from_numpy(final))


def _train(rec, bs, **kw):
    from rvz.trainer import records_to_training
    return records_to_training(rec["rec_black"], rec["rec_white"], rec["rec_side"],
                               rec["rec_idx"], rec["rec_p"], rec["final_status"], bs,
                               canonical=_oracle_canonical, **kw)


def _kept_games(rec):
    """The kept rows' positions in records_to_training's order (games in order, plies in order)."""
    live = (rec["rec_idx"] >= 0).t().reshape(-1).numpy()
    b = rec["rec_black"].t().reshape(-1).numpy()[live].view(np.uint64)
    w = rec["rec_white"].t().reshape(-1).numpy()[live].view(np.uint64)
    s = rec["rec_side"].t().reshape(-1).numpy()[live]
    return [R.O.Game(int(b[i]), int(w[i]), int(s[i]), 0, -1, 0) for i in range(len(b))]


@pytest.mark.parametrize("bs", [8, 6])
def test_exact_endgame_off_is_byte_identical(bs):
    rec = played_records(range(4), bs)
    base = _train(rec, bs)
    off = _train(rec, bs, exact_endgame=0, solver=R.host_solver)
    assert set(base) == set(off) == {"states", "policy_targets", "value_targets"}
    for k in base:
        assert base[k].dtype == off[k].dtype and torch.equal(base[k], off[k]), k


@pytest.mark.parametrize("bs,N", [(8, 5), (6, 6)])
def test_exact_endgame_replaces_the_late_rows(bs, N):
    """Random play decides these games by late blunders: on some rows with at most N empties
    the played outcome is not the position's value (asserted). Exactly the rows with at most N
    empties get sign(negamax); everything else is untouched."""
    rec = played_records(range(4), bs)
    base = _train(rec, bs)
    calls = []

    def solver(b, w, st, board_size, max_empties):
        calls.append((board_size, max_empties, b.numel()))
        return R.host_solver(b, w, st, board_size, max_empties)

    out = _train(rec, bs, exact_endgame=N, solver=solver)
    games = _kept_games(rec)
    assert calls == [(bs, N, len(games))]
    assert torch.equal(out["states"], base["states"])
    assert torch.equal(out["policy_targets"], base["policy_targets"])
    v0, v1 = base["value_targets"], out["value_targets"]
    assert v1.dtype == torch.float32 and v1.shape == v0.shape == (len(games), 1)
    late = mislabelled = 0
    for i, g in enumerate(games):
        if R.empties(g, bs) <= N:
            late += 1
            want = float(np.sign(R.negamax(g, bs)[0]))
            assert v1[i, 0].item() == want, i
            mislabelled += v0[i, 0].item() != want
        else:
            assert v1[i, 0].item() == v0[i, 0].item(), i
    assert late >= 4 * (N - 1) and mislabelled >= 1, (late, mislabelled)
    assert out["exact_rows"].dim() == 0 and int(out["exact_rows"]) == late
    assert out["exact_unsolved"].dim() == 0 and int(out["exact_unsolved"]) == 0


def test_an_abandoned_row_keeps_its_outcome_target():
    bs, N = 8, 5
    rec = played_records(range(4), bs)
    base = _train(rec, bs)
    games = _kept_games(rec)
    late = [i for i, g in enumerate(games) if R.empties(g, bs) <= N]
    full = _train(rec, bs, exact_endgame=N, solver=R.host_solver)
    # abandon a row whose exact target differs from the played outcome, and one more
    differs = [i for i in late if full["value_targets"][i, 0] != base["value_targets"][i, 0]]
    unsolved = {differs[0], late[-1]}
    assert len(unsolved) == 2

    def solver(b, w, st, board_size, max_empties):
        return R.host_solver(b, w, st, board_size, max_empties, unsolved=unsolved)

    out = _train(rec, bs, exact_endgame=N, solver=solver)
    for i in range(len(games)):
        src = base if i in unsolved else full
        assert out["value_targets"][i, 0] == src["value_targets"][i, 0], i
    assert int(out["exact_unsolved"]) == 2 and int(out["exact_rows"]) == len(late) - 2
    assert torch.equal(out["states"], base["states"])
    assert torch.equal(out["policy_targets"], base["policy_targets"])


def test_rvz_solve_refuses_bad_arguments_without_a_gpu():
    """The argument checks run before any HIP call: never-dereferenced pointers, no GPU."""
    import rvz
    from rvz._lib import RVZ_SOLVE_MAX_EMPTIES
    lib = rvz.load()
    EINVAL = -22
    assert RVZ_SOLVE_MAX_EMPTIES >= 12
    p = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000]

    def call(bs=8, n=4, me=6, limit=1000, ptrs=p):
        return lib.rvz_solve(bs, n, ptrs[0], ptrs[1], ptrs[2], me, limit, ptrs[3], ptrs[4],
                             ptrs[5], None)

    for bs in (7, 0, 10, -8):
        assert call(bs=bs) == EINVAL
    assert call(n=-1) == EINVAL
    assert call(me=-1) == EINVAL and call(me=RVZ_SOLVE_MAX_EMPTIES + 1) == EINVAL
    assert call(limit=0) == EINVAL and call(limit=-1) == EINVAL
    for k in range(5):
        assert call(ptrs=[None if j == k else q for j, q in enumerate(p)]) == EINVAL
    for bs in (6, 8):
        assert call(bs=bs, n=0) == 0 and call(bs=bs, n=0, ptrs=[None] * 6) == 0
    # the header's constant and the Python mirror agree
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "include", "rvz.h")).read()
    assert int(re.search(r"#define RVZ_SOLVE_MAX_EMPTIES (\d+)", hdr).group(1)) == \
        RVZ_SOLVE_MAX_EMPTIES


# (board size, seed, empties) -> (score, move, nodes) of tests/solve_ref.py's generator and
# unpruned negamax, recorded from this code on the CPU: guards the helper against drift
TABLE = {
    (8, 0, 6): (-4, 41, 1127),
    (8, 1, 6): (6, 63, 1792),
    (8, 2, 6): (-8, 5, 518),
    (8, 3, 6): (0, 40, 655),
    (8, 4, 6): (4, 23, 835),
    (8, 5, 6): (4, 25, 1303),
    (8, 0, 8): (2, 41, 30232),
    (8, 1, 8): (8, 63, 74033),
    (6, 0, 6): (20, 30, 732),
    (6, 1, 6): (4, 30, 486),
    (6, 2, 6): (-4, 12, 515),
    (6, 3, 6): (2, 0, 1908),
    (6, 0, 7): (-14, 2, 4011),
    (6, 1, 7): (-2, 7, 4664),
}


def test_host_reference_self_check():
    assert len(TABLE) >= 12
    for (bs, seed, empties), want in TABLE.items():
        g, _ = R.position(seed, empties, bs)
        assert R.empties(g, bs) == empties and not g.over
        assert R.solved(seed, empties, bs) == want, (bs, seed, empties)
        assert R.alphabeta(g, bs) == R.negamax(g, bs)[:2], (bs, seed, empties)
    # a root that passes, and one that is over
    g = R.last_auto_pass(25, 0, 8)
    g.side = 3 - g.side
    g.passed = 0
    s, m, k = R.negamax(g, 8)
    assert m == -1 and R.expected_move(g, m, 8) == 64 and k >= 3
    over, _ = R.position(3, 0, 8)
    assert over.over and R.negamax(over, 8) == (R.discs_diff(over), None, 1)
    assert R.expected_move(over, None, 8) == -2
