"""Opening pools on the device: rvz_openings and rvz_opening_index against tests/openings_ref.py,
every comparison exact; the engine's resets from a pool (reset, masked reset, pull-style autoreset
and fused rvz_play with reset = 1, record for record); the arena's games from given openings
against a literal loop over tests/alphabeta_ref.py."""
import numpy as np
import pytest
import torch

import alphabeta_ref as A
import openings_ref as OR

pytestmark = pytest.mark.gpu

EINVAL = -22


def _raw(bs, plies, max_rows, fill=-7):
    """The entry point itself on pre-filled outputs and an unprepared scratch."""
    import rvz
    lib = rvz.load()
    dev = "cuda"
    out = {"m": torch.full((1,), fill, dtype=torch.int32, device=dev),
           "black": torch.full((max_rows,), fill, dtype=torch.int64, device=dev),
           "white": torch.full((max_rows,), fill, dtype=torch.int64, device=dev),
           "status": torch.full((max_rows, 4), fill, dtype=torch.int32, device=dev),
           "stats": torch.full((8,), fill, dtype=torch.int64, device=dev)}
    out["scratch"] = torch.empty(lib.rvz_openings_scratch_size(bs, max_rows), dtype=torch.uint8,
                                 device=dev).fill_(0xA5)

    def launch():
        return lib.rvz_openings(bs, plies, max_rows, out["scratch"].data_ptr(),
                                out["m"].data_ptr(), out["black"].data_ptr(),
                                out["white"].data_ptr(), out["status"].data_ptr(),
                                out["stats"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out, launch


def _same_rows(out, m, ref, what):
    assert out["black"][:m].cpu().numpy().tobytes() == ref["black"].tobytes(), what
    assert out["white"][:m].cpu().numpy().tobytes() == ref["white"].tobytes(), what
    assert np.array_equal(out["status"][:m].cpu().numpy(), ref["status"]), what


@pytest.mark.parametrize("bs,plies", [(8, 0), (8, 1), (8, 4), (8, 6), (6, 0), (6, 4), (6, 6),
                                      (6, 7), (6, 8)])
def test_openings_equal_the_reference(bs, plies):
    """Rows, order, status and the eight stats, at a max_rows that is exactly the largest level's
    candidate count and at a larger, odd one; rows at and above m keep their bytes. (6, 8) is
    the case with finished children (tests/test_openings_cpu.py)."""
    import rvz
    ref = OR.openings(bs, plies)
    m, need = int(ref["stats"][0]), int(ref["stats"][4])
    for max_rows in (need, 2 * need + 13):
        out, launch = _raw(bs, plies, max_rows)
        assert launch() == 0
        torch.cuda.synchronize()
        what = (bs, plies, max_rows)
        assert int(out["m"]) == m and out["stats"].tolist() == ref["stats"].tolist(), what
        _same_rows(out, m, ref, what)
        for k in ("black", "white", "status"):
            assert bool((out[k][m:] == -7).all()), (what, k)
    if plies <= 6:
        got = rvz.openings(bs, plies)                       # the wrapper, at its default max_rows
        assert got["stats"].tolist() == ref["stats"].tolist()
        _same_rows(got, m, ref, "wrapper")
        assert got["black"].shape == (m,) and got["status"].shape == (m, 4)


@pytest.mark.parametrize("bs,plies", [(8, 6), (6, 7)])
def test_overflow_is_found_on_the_device(bs, plies):
    import rvz
    ref = OR.openings(bs, plies)
    need = int(ref["stats"][4])
    # below the last level's count, and below an earlier level's (the later launches are no-ops)
    for max_rows in (need - 1, 100):
        out, launch = _raw(bs, plies, max_rows)
        assert launch() == 0
        torch.cuda.synchronize()
        assert int(out["m"]) == -1 and int(out["stats"][0]) == -1
        assert int(out["stats"][4]) > max_rows
    with pytest.raises(rvz.RvzError, match="candidates"):
        rvz.openings(bs, plies, max_rows=need - 1)


def test_graph_replay_gives_the_same_bytes():
    ref = OR.openings(8, 6)
    m = int(ref["stats"][0])
    out, launch = _raw(8, 6, 9000)
    assert launch() == 0                                    # warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert launch() == 0
    for _ in range(2):
        for k in ("m", "black", "white", "status", "stats"):
            out[k].fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        assert int(out["m"]) == m and out["stats"].tolist() == ref["stats"].tolist()
        _same_rows(out, m, ref, "replay")
        assert bool((out["black"][m:] == -3).all())


def test_refusals_without_a_launch():
    import rvz
    lib = rvz.load()
    out, _ = _raw(8, 2, 64)
    p = {k: t.data_ptr() for k, t in out.items()}

    def call(bs=8, plies=2, rows=64, **kw):
        a = dict(p, **kw)
        return lib.rvz_openings(bs, plies, rows, a["scratch"], a["m"], a["black"], a["white"],
                                a["status"], a["stats"], None)
    assert call(bs=7) == EINVAL and call(plies=-1) == EINVAL and call(plies=61) == EINVAL
    assert call(bs=6, plies=33) == EINVAL and call(rows=0) == EINVAL
    assert call(rows=2 ** 29) == EINVAL and call(scratch=p["scratch"] + 8) == EINVAL
    for k in p:
        assert call(**{k: None}) == EINVAL, k
    torch.cuda.synchronize()
    for k in ("m", "black", "white", "status", "stats"):
        assert bool((out[k] == -7).all()), k                # nothing ran


@pytest.mark.parametrize("n_pool", [1, 2, 7, 2 ** 20])
def test_opening_index_bit_for_bit(n_pool):
    import rvz
    rng = np.random.default_rng(n_pool)
    seeds = [0, 2 ** 32 - 1, 1, 2 ** 31, 2 ** 31 - 1] + rng.integers(0, 2 ** 32, 300).tolist()
    for salt in (0, 0xDEADBEEF):
        got = rvz.opening_index(n_pool, torch.tensor(seeds, dtype=torch.int64, device="cuda"),
                                salt)
        assert got.dtype == torch.int32
        assert got.tolist() == [OR.opening_index(s, salt, n_pool) for s in seeds], salt


# ---------------------------------------------------------------- the engine
G, S = 8, 200
SALT = 77


def _net():
    import rvz
    torch.manual_seed(0)
    return rvz.AlphaZeroNetwork(8, 6, 64).cuda().eval()


def _pool():
    """The ply-4 rows of 8x8 as device tensors (black, white, side) and as host rows."""
    ref = OR.openings(8, 4)
    b = torch.from_numpy(ref["black"].view(np.int64)).cuda()
    w = torch.from_numpy(ref["white"].view(np.int64)).cuda()
    side = torch.from_numpy(ref["status"][:, 0].copy()).cuda()
    rows = list(zip(ref["black"].tolist(), ref["white"].tolist(), ref["status"][:, 0].tolist()))
    return (b, w, side), rows


def _state(eng):
    b, w, st = eng.get_state()
    torch.cuda.synchronize()
    return b.cpu().numpy().view(np.uint64).tolist(), w.cpu().numpy().view(np.uint64).tolist(), \
        st.cpu().numpy().tolist()


def test_reset_takes_the_pool_row_of_the_seed(oracle):
    import rvz
    pool, rows = _pool()
    n = len(rows)
    eng = rvz.Engine(G, S, 64)
    eng.openings(*pool, salt=SALT)
    seeds = [0, 2 ** 32 - 1, 5, 6, 1000, 1001, 2 ** 31, 123456789]
    eng.reset(seeds)
    idx = rvz.opening_index(n, torch.tensor(seeds, device="cuda"), SALT).tolist()
    assert idx == [OR.opening_index(s, SALT, n) for s in seeds] and len(set(idx)) > 4
    b, w, st = _state(eng)
    for g in range(G):
        assert (b[g], w[g]) == rows[idx[g]][:2] and st[g] == [rows[idx[g]][2], 0, -1, 0], g
    assert eng.draws().tolist() == [0] * G                  # picking an opening draws nothing
    # a masked reset leaves the other games alone
    other = [s + 17 for s in seeds]
    mask = torch.tensor([1, 0, 1, 0, 0, 0, 0, 1], dtype=torch.uint8)
    eng.reset(other, mask)
    b2, w2, st2 = _state(eng)
    for g in range(G):
        i = OR.opening_index(other[g], SALT, n) if mask[g] else idx[g]
        assert (b2[g], w2[g], st2[g][0]) == rows[i], g
    # another salt, another draw; off: the start position again
    eng.openings(*pool, salt=SALT + 1)
    eng.reset(seeds)
    assert _state(eng)[0] == [rows[OR.opening_index(s, SALT + 1, n)][0] for s in seeds]
    eng.openings(None)
    eng.reset(seeds)
    first = oracle.new_game(8)
    b3, w3, st3 = _state(eng)
    assert b3 == [int(first.black)] * G and w3 == [int(first.white)] * G
    assert st3 == [[1, 0, -1, 0]] * G


def test_bad_pools_are_refused():
    import rvz
    pool, rows = _pool()
    eng = rvz.Engine(G, S, 64)
    eng.openings(*pool, salt=SALT)

    def bad(row, b=None, w=None, side=None):
        pb, pw, ps = (t.clone() for t in pool)
        if b is not None:
            pb[row] = b
        if w is not None:
            pw[row] = w
        if side is not None:
            ps[row] = side
        with pytest.raises(rvz.RvzError, match=rf"\(-22\).*row {row} "):
            eng.openings(pb, pw, ps)
    bad(3, b=int(pool[1][3]) | 1)                           # overlapping discs (and more)
    bad(5, side=3)
    bad(0, side=0)
    bad(9, b=1, w=-2 ** 63)                                 # the mover has no legal square
    pb, pw, ps = (t.clone() for t in pool)
    ps[7], ps[2] = 3, 0
    with pytest.raises(rvz.RvzError, match="row 2 "):       # the first bad row
        eng.openings(pb, pw, ps)
    with pytest.raises(rvz.RvzError):                       # 6x6 engine: a bit at or above 36
        rvz.Engine(2, S, 64, board_size=6).openings(*pool)
    # a refused pool leaves the setting as it was
    eng.reset([4] * G)
    assert _state(eng)[0] == [rows[OR.opening_index(4, SALT, len(rows))][0]] * G
    eng.search_begin()
    eng.search_step()
    with pytest.raises(rvz.RvzError, match="inside a search"):
        eng.openings(*pool)


def _records(run):
    return [t.cpu().numpy() for t in (run.rec_black, run.rec_white, run.rec_side, run.rec_idx,
                                      run.rec_p)]


def test_pull_and_fused_autoreset_records_agree_and_restart_from_the_pool(oracle):
    """8 games x 200 simulations, the 6x64 net, 62 plies with autoreset from the ply-4 pool (a game
    from there has at most 56 plies, so every slot restarts): the pull-style runner's records and
    the fused launch's are the same arrays; each record after a game end is the pool row of the
    slot's next seed; records_games calls exactly the emitted games headless, none of the pool's
    rows being the start position."""
    import rvz
    pool, rows = _pool()
    n, P, C, base = len(rows), 62, 2, 42
    ev = rvz.LeafEvaluator(_net())
    pull = rvz.SelfPlayRunner(rvz.Engine(G, S, 64, compact_leaves=True, memo=True), ev,
                              autoreset=True, seed_base=base, record=True, max_plies=P,
                              skip_last_eval=True, openings=(*pool, SALT))
    pull.start()
    for _ in range(P):
        pull.ply()
    pull.check()
    fused = rvz.SelfPlayRunner(rvz.Engine(G, S, 64, memo=True), ev, autoreset=True,
                               seed_base=base, record=True, max_plies=P, skip_last_eval=True,
                               fused=True, carry_plies=C, openings=(*pool, SALT))
    fused.start()
    fused.play_record(P)
    fused.check()
    a, f = _records(pull), [t[C:] for t in _records(fused)]
    for x, y, name in zip(a, f, ("black", "white", "side", "idx", "p")):
        assert x.tobytes() == y.tobytes(), name
    assert torch.equal(pull.seeds, fused.seeds) and torch.equal(pull._done, fused._done)
    for x, y in zip(pull.eng.get_state(), fused.eng.get_state()):
        assert torch.equal(x, y)
    done = pull._done.tolist()
    assert min(done) >= 1                                   # every slot restarted
    # every game opens on the pool row of its seed: the first record, and each one after an end
    black, white, side, idx, _ = a
    black = black.view(np.uint64)
    white = white.view(np.uint64)
    opened = 0
    for g in range(G):
        seed, cur = base + g, None
        for p in range(P):
            rec = (int(black[p, g]), int(white[p, g]), int(side[p, g]))
            if cur is None:
                assert rec == rows[OR.opening_index(seed, SALT, n)], (p, g)
                cur = oracle.Game(*rec, 0, -1, 0)
                opened += 1
            assert rec == (int(cur.black), int(cur.white), int(cur.side)), (p, g)
            i = int(idx[p, g])
            assert oracle.make_move(cur, -1 if i == 64 else i, 8)
            if cur.over:
                seed, cur = seed + G, None
        assert int(pull.seeds[g]) == seed
    assert opened == G + sum(done)
    out = rvz.records_games(*(torch.from_numpy(t).cuda() for t in a), 8)
    stats = out["stats"].tolist()
    start = oracle.new_game(8)
    assert (int(start.black), int(start.white), 1) not in rows
    assert stats[1] == sum(done) and stats[5] == stats[1] and stats[3] == stats[4] == 0


# ---------------------------------------------------------------- the arena
def _host_game(bs, row, black_depth, white_depth):
    """One game on the oracle from (black, white, side): (result for Black, final disc counts)."""
    wt = A.default_table(bs)
    g = A.O.Game(row[0], row[1], row[2], 0, -1, 0)
    while not g.over:
        depth = black_depth if g.side == 1 else white_depth
        assert A.O.make_move(g, A.alphabeta(g, depth, wt, bs)[1], bs)
    nb, nw = bin(g.black).count("1"), bin(g.white).count("1")
    return (1.0 if nb > nw else (0.0 if nw > nb else 0.5)), (nb, nw)


def test_arena_plays_an_opening_suite_both_colours():
    """6x6, depth 2 against depth 1 over the ply-3 openings (white to move in all of them: the
    white id moves first), both draw orders: results and final disc counts are the host games'."""
    import rvz
    from rvz.arena import AlphaBetaPlayer, Arena
    bs = 6
    b, w, side = rvz.opening_suite(bs, 3)
    ref = OR.openings(bs, 3)
    n = len(ref["black"])
    assert b.cpu().numpy().tobytes() == ref["black"].tobytes() and side.tolist() == [2] * n
    rows = list(zip(ref["black"].tolist(), ref["white"].tolist(), ref["status"][:, 0].tolist()))
    host = [(_host_game(bs, r, 2, 1), _host_game(bs, r, 1, 2)) for r in rows]
    want = [(a[0], 1.0 - c[0]) for a, c in host]
    assert len(set(want)) > 1                               # the openings matter
    for order in ("reference", "batched"):
        arena = Arena(seed=3)
        arena.add_player(AlphaBetaPlayer("d2", depth=2, board_size=bs))
        arena.add_player(AlphaBetaPlayer("d1", depth=1, board_size=bs))
        finals = []
        apply = rvz.Engine.apply

        def spy(eng, sq, finals=finals):
            r = apply(eng, sq)
            finals[:] = [eng.get_state()]
            return r
        rvz.Engine.apply = spy
        try:
            got = arena.play_openings("d2", "d1", (b, w, side), draw_order=order)
        finally:
            rvz.Engine.apply = apply
        assert got == want, order
        fb, fw, _ = finals[0]
        counts = [(bin(x & (2 ** 64 - 1)).count("1"), bin(y & (2 ** 64 - 1)).count("1"))
                  for x, y in zip(fb.tolist(), fw.tolist())]
        assert counts == [c for pair in host for c in (pair[0][1], pair[1][1])], order
        assert len(arena.elo.history) == 2 * n
        assert arena.elo.games_played == {"d2": 2 * n, "d1": 2 * n}
    # given rows through play_games: side 2 gives the first move to the white id
    arena = Arena(seed=3)
    arena.add_player(AlphaBetaPlayer("d2", depth=2, board_size=bs))
    arena.add_player(AlphaBetaPlayer("d1", depth=1, board_size=bs))
    res = arena.play_games(["d1"] * n, ["d2"] * n, openings=(b, w, side))
    assert res == [c[0] for _, c in host]
    with pytest.raises(ValueError):
        arena.play_games(["d1"], ["d2"], openings=(b, w, side))


def test_balanced_suite_keeps_the_small_scores():
    """6x6, ply 4, depth 2, |score| <= 6: the rows the host alpha-beta scores that way (26 of
    the 236), in openings' order."""
    import rvz
    bs, plies, depth, bound = 6, 4, 2, 6
    ref = OR.openings(bs, plies)
    wt = A.default_table(bs)
    keep = [abs(A.alphabeta(A.O.Game(int(b), int(w), int(st[0]), 0, -1, 0), depth, wt, bs)[0])
            <= bound for b, w, st in zip(ref["black"], ref["white"], ref["status"])]
    assert 0 < sum(keep) < len(keep)
    b, w, side = rvz.opening_suite(bs, plies, depth=depth, max_abs_score=bound)
    assert b.cpu().numpy().tobytes() == ref["black"][keep].tobytes()
    assert w.cpu().numpy().tobytes() == ref["white"][keep].tobytes()
    assert side.tolist() == [1] * sum(keep) and side.dtype == torch.int32


def test_trainer_self_play_from_a_pool():
    """6x6, 16 games, 64 simulations in batches of 16 (tests/test_gpu_records_games.py's shape),
    the ply-3 pool: a lockstep iteration's games open on pool rows, and with continuous_plies
    every emitted game counts as headless, none of the rows being the start position."""
    import rvz
    from rvz.pipeline import SelfPlayTrainer
    pool = rvz.opening_suite(6, 3)
    n = pool[0].numel()
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(6, 1, 64).cuda()
    spt = SelfPlayTrainer(net, 16, num_simulations=64, batch_size=16, seed=5, train_steps=1,
                          train_batch=32, openings=(*pool, 9))
    spt.generate()
    run = spt.runner
    want = [OR.opening_index(5 + g, 9, n) for g in range(16)]
    assert run.rec_black[0].tolist() == pool[0][want].tolist()
    assert run.rec_white[0].tolist() == pool[1][want].tolist()
    assert run.rec_side[0].tolist() == [2] * 16 and len(set(want)) > 4
    spt = SelfPlayTrainer(net, 16, num_simulations=64, batch_size=16, seed=5, train_steps=1,
                          train_batch=32, continuous_plies=24, replay_iterations=2,
                          policy_target="full", openings=(*pool, 9))
    emitted = 0
    for _ in range(2):
        out = spt.run_iteration()
        assert out["records_abandoned"] == 0
        assert out["records_headless_games"] == out["games_emitted"]
        emitted += out["games_emitted"]
    assert emitted == int(spt.runner.games_done.item()) > 0
