"""tests/openings_ref.py itself, on the CPU: its levels against a literal enumeration with the
oracle's legal / make_move, the counts the GPU cases rely on (duplicates at every ply they use,
finished children where they claim some), the index draw, and the argument rules the Python
wrappers check before any device call."""
import inspect

import numpy as np
import pytest

import openings_ref as OR
import replay_ref as RR

EINVAL = -22                                        # include/rvz.h RVZ_EINVAL

# (board, plies) of tests/test_gpu_openings.py's exact comparisons
GPU_CASES = [(8, 0), (8, 1), (8, 4), (8, 6), (6, 0), (6, 4), (6, 6), (6, 7), (6, 8)]


def _candidates(O, bs, rows):
    """Level k's rows -> level k + 1's candidates in (parent, square) order and the finished
    children, written out with the oracle directly."""
    cand, finished = [], 0
    for b, w, s in rows:
        mask = O.legal(b, w, bs) if s == 1 else O.legal(w, b, bs)
        for sq in range(bs * bs):
            if not mask >> sq & 1:
                continue
            g = O.Game(b, w, s, 0, -1, 0)
            assert O.make_move(g, sq, bs)
            if g.over:
                finished += 1
            else:
                cand.append((int(g.black), int(g.white), int(g.side)))
    return cand, finished


@pytest.mark.parametrize("bs", [8, 6])
def test_levels_against_a_literal_enumeration(oracle, bs):
    lv = OR.levels(bs, 5)
    first = oracle.new_game(bs)
    assert lv[0]["rows"] == [(int(first.black), int(first.white), 1)]
    for k in range(5):
        cand, finished = _candidates(oracle, bs, lv[k]["rows"])
        nxt = lv[k + 1]
        assert nxt["candidates"] == len(cand) and nxt["dropped"] == finished
        want = sorted(set(cand), key=cand.index)            # first occurrences, in order
        assert nxt["rows"] == want and nxt["dups"] == len(cand) - len(want)
        assert all(not (b & w) and s in (1, 2) for b, w, s in want)
    # the first plies of Othello's perft; from ply 3 on, transpositions merge
    assert [x["candidates"] for x in lv[:4]] == [1, 4, 12, 56]
    assert [len(x["rows"]) for x in lv[:4]] == [1, 4, 12, 54]
    for plies in range(6):
        o = OR.openings(bs, plies)
        assert o["stats"][0] == len(lv[plies]["rows"]) == len(o["black"]) == len(o["white"])
        assert o["stats"][1] == lv[plies]["candidates"]
        assert o["stats"][4] == max(x["candidates"] for x in lv[:plies + 1])
        assert (o["status"][:, 1:] == [0, -1, 0]).all()
        assert o["status"][:, 0].tolist() == [r[2] for r in lv[plies]["rows"]]


def test_the_gpu_cases_hold_what_they_are_there_for():
    """Every ply >= 4 the GPU test compares has duplicates to remove; ply 6 and deeper has more
    candidates than one workgroup's scan chunk (1,024) and, for the lane-per-row kernels, than
    one workgroup (256); 6x6 at ply 8 is the shallowest level with finished children (none on 8x8
    through ply 8), so that case is there for the dropped count."""
    for bs, plies in GPU_CASES:
        st = OR.openings(bs, plies)["stats"]
        if plies >= 4:
            assert st[3] > 0, (bs, plies)
        if plies >= 6:
            assert st[1] > 4 * 1024 and st[0] > 4 * 1024, (bs, plies)
        assert (st[2] > 0) == ((bs, plies) == (6, 8)), (bs, plies, st[2])
    assert OR.openings(6, 8)["stats"].tolist() == [235673, 266062, 2, 35800, 266062, 0, 0, 0]
    assert OR.openings(8, 6)["stats"].tolist() == [7092, 7572, 0, 542, 7572, 0, 0, 0]
    # the sides: black after an even number of plies, white after an odd one (no auto-pass yet)
    assert set(OR.openings(6, 7)["status"][:, 0].tolist()) == {2}
    assert set(OR.openings(8, 4)["status"][:, 0].tolist()) == {1}


def test_opening_index_draw():
    assert OR.opening_index(0, 0, 1) == 0 and OR.opening_index(2 ** 32 - 1, 9, 1) == 0
    for n in (2, 7, 2 ** 20):
        got = [OR.opening_index(s, 3, n) for s in range(400)]
        assert min(got) >= 0 and max(got) < n and len(set(got)) > 1
        x0 = RR.philox4x32_10((5, 3), (0, 0, 0, 1))[0]
        assert OR.opening_index(5, 3, n) == x0 * n >> 32
    # its own block: not the root noise's (counter word 3 = 0), and the salt is part of the key
    assert RR.philox4x32_10((5, 3), (0, 0, 0, 1)) != RR.philox4x32_10((5, 3), (0, 0, 0, 0))
    n = 2 ** 20
    assert [OR.opening_index(s, 0, n) for s in range(8)] != \
        [OR.opening_index(s, 1, n) for s in range(8)]
    counts = np.bincount([OR.opening_index(s, 0, 7) for s in range(7000)], minlength=7)
    assert counts.min() > 800 and counts.max() < 1200          # 1000 each, +- 6 sigma


def test_wrapper_argument_rules():
    import rvz
    from rvz.records import OPENINGS_DEFAULT_MAX_ROWS, check_openings_args
    assert check_openings_args(8, 8, None) == OPENINGS_DEFAULT_MAX_ROWS >= 303386
    assert check_openings_args(6, 0, 5) == 5
    for bs, plies, rows in ((7, 1, None), (8, -1, None), (8, 61, 10), (6, 33, 10), (8, 9, None),
                            (8, 1, 0), (8, 1, 2 ** 29), (8, 1.0, None), (8, 1, True)):
        with pytest.raises(rvz.RvzError):
            check_openings_args(bs, plies, rows)
    with pytest.raises(rvz.RvzError):
        rvz.opening_suite(8, 2, depth=2)                        # no default threshold
    with pytest.raises(rvz.RvzError):
        rvz.opening_suite(8, 2, max_abs_score=3)
    from rvz.arena import Arena
    from rvz.pipeline import SelfPlayTrainer
    assert list(inspect.signature(Arena.play_games).parameters)[1:] == \
        ["black_ids", "white_ids", "openings", "draw_order"]
    assert "openings" in inspect.signature(SelfPlayTrainer.__init__).parameters
    assert "openings" in inspect.signature(rvz.SelfPlayRunner.__init__).parameters


def test_entry_points_refuse_bad_arguments_without_a_device():
    """RVZ_EINVAL before any HIP call: these run on a machine without a GPU."""
    import ctypes as C
    import rvz
    lib = rvz.load()
    buf = (C.c_char * 4096)()
    p = (C.addressof(buf) + 15) & ~15
    good = dict(bs=8, plies=2, rows=8, scratch=p, m=p, b=p, w=p, st=p, stats=p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.rvz_openings(a["bs"], a["plies"], a["rows"], a["scratch"], a["m"], a["b"],
                                a["w"], a["st"], a["stats"], None)
    for kw in (dict(bs=7), dict(bs=0), dict(plies=-1), dict(plies=61), dict(bs=6, plies=33),
               dict(rows=0), dict(rows=-4), dict(rows=2 ** 29), dict(scratch=None),
               dict(scratch=p + 8), dict(m=None), dict(b=None), dict(w=None), dict(st=None),
               dict(stats=None)):
        assert call(**kw) == EINVAL, kw
    assert lib.rvz_openings_scratch_size(7, 8) < 0 and lib.rvz_openings_scratch_size(8, 0) < 0
    assert lib.rvz_openings_scratch_size(8, 2 ** 29) < 0
    a, b = lib.rvz_openings_scratch_size(8, 1000), lib.rvz_openings_scratch_size(8, 1025)
    assert 0 < a < b and a % 16 == 0 and lib.rvz_openings_scratch_size(6, 1000) == a
    assert lib.rvz_openings_scratch_size(8, 2 ** 29 - 1) > 2 ** 34
    for n_pool, n, seeds, out in ((0, 4, p, p), (-1, 4, p, p), (5, -1, p, p), (5, 4, None, p),
                                  (5, 4, p, None)):
        assert lib.rvz_opening_index(n_pool, n, seeds, 0, out, None) == EINVAL
    assert lib.rvz_opening_index(5, 0, None, 0, None, None) == 0


def test_trainer_openings_rules():
    import torch
    from rvz.network import AlphaZeroNetwork
    from rvz.pipeline import SelfPlayTrainer
    net = AlphaZeroNetwork(6, 1, 16)
    o = OR.openings(6, 2)
    pool = (torch.from_numpy(o["black"].view(np.int64)), torch.from_numpy(o["white"].view(np.int64)),
            torch.from_numpy(o["status"][:, 0].copy()))
    for kw, says in ((dict(openings=pool, adjudicate_empties=4), "adjudicate_empties"),
                     (dict(openings=pool[:2]), "openings"),
                     (dict(openings=(*pool, 1, 2)), "openings")):
        with pytest.raises(ValueError) as err:
            SelfPlayTrainer(net, games=4, **kw)
        assert says in str(err.value), (kw, str(err.value))
