"""rvz_alphabeta without a GPU: the host reference checks itself, the default tables, the C-ABI's
argument checks (which run before any HIP call) and the arena's draw accounting with an
AlphaBetaPlayer in the schedule."""
import ctypes as C
import random
import types

import numpy as np
import pytest

import alphabeta_ref as A
import solve_ref as R

EINVAL = -22


def _positions(bs):
    """A dozen seeded positions per board, from the opening to 12 empties."""
    nsq = bs * bs
    stops = (nsq - 6, nsq - 12, nsq // 2, 12)
    return [R.position(s, stops[s % 4], bs)[0] for s in range(12)]


@pytest.mark.parametrize("bs", [8, 6])
@pytest.mark.parametrize("table", ["default", "asymmetric"])
def test_reference_alphabeta_equals_negamax(bs, table):
    wt = A.TABLES[table](bs)
    assert A.table_bound(wt, bs) <= A.HEUR_MAX
    for g in _positions(bs):
        for depth in (1, 2, 3):
            s, m, k = A.negamax(g, depth, wt, bs)
            assert A.alphabeta(g, depth, wt, bs) == (s, m), (bs, table, depth, g.astuple())
            assert k >= 2 and abs(s) < A.WIN - 64


def test_asymmetric_table_has_no_symmetry():
    """The table that catches transposed square indices differs from each of its seven images."""
    for bs in (8, 6):
        t = A.asymmetric_table(bs)[:-1]
        for k in range(1, 8):
            assert [t[_sym(s, k, bs)] for s in range(bs * bs)] != list(t), (bs, k)


@pytest.mark.parametrize("bs", [8, 6])
def test_reference_reaches_the_end_of_the_game(bs):
    """At a depth that reaches the end of the game the score is the solver's, pushed by WIN."""
    wt = A.asymmetric_table(bs)
    seen = set()
    for seed in range(12):
        g, _ = R.position(seed, 5, bs)
        hs, hm, _ = R.solved(seed, 5, bs)
        want = 0 if hs == 0 else (A.WIN + hs if hs > 0 else hs - A.WIN)
        for depth in (5, A.MAX_DEPTH):
            s, m = A.alphabeta(g, depth, wt, bs)
            assert (s, A.expected_move(g, m, bs)) == (want, hm), (bs, seed, depth)
        s, m, _ = A.negamax(g, 5, wt, bs)
        assert (s, A.expected_move(g, m, bs)) == (want, hm)
        seen.add(np.sign(hs))
    assert len(seen) >= 2


def _sym(s, k, bs):
    r, c = divmod(s, bs)
    if k & 4:
        r, c = c, r
    if k & 1:
        r = bs - 1 - r
    if k & 2:
        c = bs - 1 - c
    return r * bs + c


@pytest.mark.parametrize("bs", [8, 6])
def test_default_tables(bs):
    import rvz
    from rvz._lib import RVZ_AB_HEUR_MAX, RVZ_AB_MAX_DEPTH, RVZ_AB_WIN
    assert (RVZ_AB_MAX_DEPTH, RVZ_AB_WIN, RVZ_AB_HEUR_MAX) == (A.MAX_DEPTH, A.WIN, A.HEUR_MAX)
    assert (rvz.AB_MAX_DEPTH, rvz.AB_WIN, rvz.AB_HEUR_MAX) == (A.MAX_DEPTH, A.WIN, A.HEUR_MAX)
    nsq = bs * bs
    wt = rvz.alphabeta_weights(bs)
    assert isinstance(wt, list) and len(wt) == nsq + 1 and all(type(x) is int for x in wt)
    assert tuple(wt) == A.default_table(bs)
    assert A.table_bound(wt, bs) <= RVZ_AB_HEUR_MAX
    for k in range(8):
        assert [wt[_sym(s, k, bs)] for s in range(nsq)] == wt[:nsq], k
    corners = [0, bs - 1, nsq - bs, nsq - 1]
    xs = [bs + 1, 2 * bs - 2, nsq - 2 * bs + 1, nsq - bs - 2]
    assert all(wt[s] == max(wt[:nsq]) for s in corners)
    assert all(wt[s] == min(wt[:nsq]) for s in xs)
    assert sorted(s for s in range(nsq) if wt[s] == max(wt[:nsq])) == sorted(corners)
    assert sorted(s for s in range(nsq) if wt[s] == min(wt[:nsq])) == sorted(xs)
    assert wt[nsq] > 0
    with pytest.raises(rvz.RvzError):
        rvz.alphabeta_weights(7)


def test_argument_checks_without_gpu():
    """Every argument check of rvz_alphabeta runs before any HIP call: with never-dereferenced
    device pointers each bad call returns RVZ_EINVAL, and n = 0 returns RVZ_OK without a launch."""
    import rvz
    lib = rvz.load()
    b, w, st, sc, mv, nd = (0x10000 * k for k in range(1, 7))      # never dereferenced

    def table(values):
        return C.cast((C.c_int32 * len(values))(*values), C.c_void_p)

    good = {8: rvz.alphabeta_weights(8), 6: rvz.alphabeta_weights(6)}
    keep = []

    def call(bs=8, n=1, depth=4, wt="default", limit=1000, ptrs=(b, w, st, sc, mv, nd)):
        if wt == "default":
            wt = table(good.get(bs, good[8]))
        keep.append(wt)
        return lib.rvz_alphabeta(bs, n, ptrs[0], ptrs[1], ptrs[2], depth, wt, limit, ptrs[3],
                                 ptrs[4], ptrs[5], None)

    assert call(n=0) == 0 and call(bs=6, n=0) == 0
    assert call(n=0, ptrs=(None,) * 6) == 0
    assert call(n=0, depth=1) == 0 and call(n=0, depth=A.MAX_DEPTH) == 0
    assert call(depth=0) == EINVAL and call(depth=A.MAX_DEPTH + 1) == EINVAL
    assert call(n=0, depth=0) == EINVAL and call(n=0, depth=13) == EINVAL
    for bs in (7, 0, 10):
        assert call(bs=bs) == EINVAL and call(bs=bs, n=0) == EINVAL
    assert call(n=-1) == EINVAL
    assert call(limit=0) == EINVAL and call(limit=-5) == EINVAL and call(n=0, limit=0) == EINVAL
    assert call(wt=None) == EINVAL and call(n=0, wt=None) == EINVAL
    # the weight bound: exactly at it is accepted, one unit over is refused; in a square weight
    # and in the mobility weight, whose unit counts S*S times
    for bs in (8, 6):
        nsq = bs * bs
        at = [0] * (nsq + 1)
        at[3], at[nsq - 1], at[nsq] = -(A.HEUR_MAX - 5000 - nsq * 100), 5000, -100
        assert A.table_bound(at, bs) == A.HEUR_MAX
        assert call(bs=bs, n=0, wt=table(at)) == 0
        over = list(at)
        over[3] -= 1
        assert call(bs=bs, n=0, wt=table(over)) == EINVAL
        assert call(bs=bs, n=1, wt=table(over)) == EINVAL
        over = list(at)
        over[nsq - 1] += 1
        assert call(bs=bs, n=0, wt=table(over)) == EINVAL
        mob = [0] * nsq + [A.HEUR_MAX // nsq]
        assert call(bs=bs, n=0, wt=table(mob)) == 0
        mob[nsq] += 1
        assert call(bs=bs, n=0, wt=table(mob)) == EINVAL
        mob[nsq] = -mob[nsq]
        assert call(bs=bs, n=0, wt=table(mob)) == EINVAL
        assert call(bs=bs, n=0, wt=table([2 ** 31 - 1] * (nsq + 1))) == EINVAL
        assert call(bs=bs, n=0, wt=table([-2 ** 31] * (nsq + 1))) == EINVAL
    # a null array with n = 1 (out_nodes alone is nullable, but nothing is launched here)
    for k in range(5):
        ptrs = [b, w, st, sc, mv, nd]
        ptrs[k] = None
        assert call(ptrs=ptrs) == EINVAL, k
    # the Python surface raises on the same arguments before it touches a device
    import torch
    e = torch.zeros(0, dtype=torch.int64)
    e4 = torch.zeros(0, 4, dtype=torch.int32)
    for kw in (dict(depth=0), dict(depth=13), dict(board_size=7), dict(node_limit=0),
               dict(weights=[0] * 64), dict(weights=[1000] * 65)):
        with pytest.raises(rvz.RvzError):
            rvz.alphabeta(e, e, e4, **kw)
    s0, m0, k0 = rvz.alphabeta(e, e, e4)
    assert s0.numel() == m0.numel() == k0.numel() == 0


# ------------------------------------------------------------------ arena draw accounting
def _fake_game(g, kinds, u_of, choice_of):
    """A stand-in for one game's moves that consumes draws like an arena game: 12 moves, sides
    alternate; an MCTS move ("m") takes one uniform, a random move ("r") chooses among
    1 + (7 t + g) mod 9 squares and ends the game on square 0, an alpha-beta move ("x") draws
    nothing. Returns a result that depends on every draw."""
    h = g
    for t in range(12):
        kind = kinds[t % 2]
        if kind == "m":
            h = (h * 31 + int(u_of() * 1e6)) % 1000003
        elif kind == "r":
            m = choice_of(list(range(1 + (7 * t + g) % 9)))
            h = (h * 31 + m) % 1000003
            if m == 0:
                break
        else:
            h = (h * 31 + 17 * t) % 1000003
    return [0.0, 0.5, 1.0][h % 3]


KIND = {"a": "m", "b": "m", "r": "r", "x": "x", "y": "x"}


def _arena(seed=5):
    from rvz.arena import AlphaBetaPlayer, Arena
    arena = Arena(seed=seed)
    for pid, kind in KIND.items():
        if kind == "x":
            arena.players[pid] = AlphaBetaPlayer(pid, depth=2, device="cpu")
        else:
            arena.players[pid] = types.SimpleNamespace(
                model=None if kind == "r" else object(), board_size=8, device="cpu")
    return arena


def test_alphabeta_player_attributes():
    from rvz.arena import AlphaBetaPlayer, ELOPlayer
    import rvz
    p = AlphaBetaPlayer("x", depth=3, board_size=6, solve_empties=6)
    assert p.model is None and p.alphabeta is True and p.board_size == 6
    assert p.weights == rvz.alphabeta_weights(6) and p.depth == 3 and p.solve_empties == 6
    assert not getattr(ELOPlayer("r", model=None, device="cpu"), "alphabeta", False)
    for kw in (dict(depth=0), dict(depth=13), dict(solve_empties=-1), dict(solve_empties=15)):
        with pytest.raises(ValueError):
            AlphaBetaPlayer("x", **kw)
    arena = _arena()
    assert arena._board_size(["x"], ["r"]) == 8
    arena.players["x"] = AlphaBetaPlayer("x", board_size=6)
    assert arena._board_size(["x"], ["r"]) == 6 and arena._board_size(["r"], ["r"]) == 8
    with pytest.raises(ValueError):
        arena._board_size(["x"], ["a"])


def test_arena_draw_accounting_with_alphabeta(monkeypatch):
    """A schedule mixing MCTS, random and alpha-beta players, the game replaced by _fake_game (no
    GPU): results and both generators equal the sequential loop's, in which an alpha-beta move
    draws nothing; in both draw orders the alpha-beta moves leave the generators alone; and games
    without a random player are not serialised."""
    from rvz.arena import Arena

    played = []

    def fake_lockstep(self, black_ids, white_ids, games, draws, cache=None):
        played.extend(games)
        G = len(black_ids)
        draws.begin_ply(G)
        res = [None] * G
        for g in games:
            res[g] = _fake_game(g, (KIND[black_ids[g]], KIND[white_ids[g]]),
                                lambda: float(draws.uniforms(np.array([g]))[g]),
                                lambda sq: draws.choice(g, sq))
        return res

    monkeypatch.setattr(Arena, "_lockstep", fake_lockstep)
    passes = {}
    schedules = {
        "mcts": [("a", "b"), ("b", "a")] * 8,
        "mcts+ab": [("a", "b"), ("a", "x"), ("x", "b"), ("x", "y")] * 4,
        "ab": [("x", "y"), ("y", "x")] * 3,
        "all": [("a", "r"), ("x", "r"), ("a", "x"), ("r", "y"), ("a", "b"), ("r", "r"),
                ("y", "x")] * 3,
    }
    for name, pairs in schedules.items():
        arena = _arena()
        played.clear()
        black = [p[0] for p in pairs]
        white = [p[1] for p in pairs]
        got = arena.play_games(black, white)
        np_rng, py_rng = np.random.RandomState(5), random.Random(5)
        want = [_fake_game(g, (KIND[b], KIND[w]), lambda: float(np_rng.random_sample()),
                           py_rng.choice) for g, (b, w) in enumerate(pairs)]
        assert got == want, name
        assert arena.np_rng.random_sample() == np_rng.random_sample(), name
        assert arena.py_rng.random() == py_rng.random(), name
        passes[name] = arena.reference_order_passes
        n_rand = sum(1 for b, w in pairs if "r" in (b, w))
        assert arena.reference_order_passes <= n_rand + 3, (name, arena.reference_order_passes)
        if not n_rand:                                # fixed move counts: every game twice at most
            assert len(played) <= 2 * len(pairs), (name, len(played))
    # 12 of the 16 games of "mcts+ab" have an alpha-beta player: serialised, they would take a
    # pass each; they take what 16 MCTS-only games take
    assert passes["mcts+ab"] == passes["mcts"] <= 3, passes
    assert passes["ab"] == 1, passes                  # no draws at all: every input is exact
    # alpha-beta-only games leave both generators untouched, in both draw orders
    for order in ("reference", "batched"):
        arena = _arena(seed=9)
        arena.play_games(["x", "y"], ["y", "x"], draw_order=order)
        if order == "reference":
            assert arena.np_rng.random_sample() == np.random.RandomState(9).random_sample()
        assert arena.py_rng.random() == random.Random(9).random()
