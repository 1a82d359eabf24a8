"""Searches rooted at positions set with rvz_env_set: roots no game from the start reaches (the
mover without a legal square, full boards, a root where neither side can move, a finished game)
and roots one to six empties from the end, where most traversals end on known terminals.

Pull-style (rvz_search_* / rvz_act / rvz_env_autoreset) and fused (rvz_play) runs against the
literal oracle (oracle_play.OracleGames started from the same positions): visits, f64 policy
vectors bitwise, indices, the state after each act, the draws consumed, the plies / done
counters. What a root without a legal square must give is the oracle's own answer, which restates
the reference (mcts.py:339, 567-579, 679-692; board.py:178-179): no visits, index 0, no draw, the
state left as it is, and the ply counted because the index is not negative.

The unread-rows rule of rvz_play (skip_last_eval) is placed one legal move below,
at and above its threshold, at batch sizes other than 64 and with a remainder batch."""
import random

import numpy as np
import pytest
import torch

import solve_ref as R
from oracle_play import OracleGames

pytestmark = pytest.mark.gpu

G = 32
SEED0, STRIDE = 900, G
PASS_SEEDS = {8: (12, 25), 6: (9, 15)}       # solve_ref.RootCases' pass-root playouts


def _net(board, seed=0):
    import rvz
    torch.manual_seed(seed)
    return rvz.AlphaZeroNetwork(board, 1, 64).cuda().eval()


@pytest.fixture(scope="module")
def evaluators():
    import rvz
    from evaluators import TableEvaluator
    cache = {}

    def get(kind, bs):
        if (kind, bs) not in cache:
            cache[kind, bs] = TableEvaluator() if kind == "table" else \
                rvz.LeafEvaluator(_net(bs))
        return cache[kind, bs]
    return get


def _live(seed0, empties, bs, count):
    """`count` playout positions with exactly `empties` empty squares that are not over."""
    out, s = [], seed0
    while len(out) < count:
        g, _ = R.position(s, empties, bs)
        if not g.over and R.empties(g, bs) == empties:
            out.append(g)
        s += 1
    return out


def roots(O, bs):
    """The 32 roots and, per root, its class."""
    nsq = bs * bs
    full = (1 << nsq) - 1
    rows = []
    for e, n in ((1, 3), (2, 3), (3, 3), (4, 3), (6, 4)):
        rows += [(f"e{e}", g) for g in _live(0, e, bs, n)]
    for g in R.pass_roots(bs, PASS_SEEDS[bs]):
        for passed in (0, 1):
            c = g.copy()
            c.passed = passed
            rows.append((f"pass{passed}", c))
    over = R.position(3, 0, bs)[0]
    assert over.over
    rows += [("over", over), ("over", R.position(5, 0, bs)[0])]
    even = full & 0x5555555555555555
    rows += [("full", O.Game(even, full ^ even, 1, 0, -1, 0)),
             ("full", O.Game(full & 0x0F0F0F0F0F0F0F0F, full & 0xF0F0F0F0F0F0F0F0, 2, 0, -1, 1))]
    # neither side can move: two discs far apart, one colour alone, the empty board
    rows += [("stuck", O.Game(1, 1 << (nsq - 1), 1, 0, -1, 0)),
             ("stuck", O.Game(1 << (nsq - 1), 1 << bs, 2, 0, -1, 1)),
             ("stuck", O.Game(0, full >> 9, 1, 0, -1, 0)),
             ("stuck", O.Game(0, 0, 2, 0, -1, 0))]
    rows += [(f"e{e}", g) for e in (5, 6) for g in _live(40, e, bs, 2)]
    assert len(rows) == G, len(rows)
    for kind, g in rows:
        lm = R.mover_mask(g, bs)
        if kind in ("pass0", "pass1", "full", "stuck"):
            assert not g.over and lm == 0
        if kind == "stuck":
            c = g.copy()
            c.side = 3 - c.side
            assert R.mover_mask(c, bs) == 0
        if kind[0] == "e":
            assert not g.over and lm
    return [k for k, _ in rows], [g for _, g in rows]


def _set(eng, games, seeds):
    eng.reset(seeds)
    eng.set_state(*R.to_device(games))


def _state(eng):
    b, w, st = eng.get_state()
    return b.cpu().numpy().view(np.uint64).copy(), w.cpu().numpy().view(np.uint64).copy(), \
        st.cpu().numpy().copy()


def oracle_run(O, ev, games, S, B, T, bs, plies, reset):
    """The oracle's plies from `games` with rvz_env_autoreset's bookkeeping restated: plies += 1
    for an index >= 0; with reset, a game that is over adds 1 to done, takes seed += STRIDE and
    restarts from the start position with np.random.seed(seed) (draws counted from there).
    Per ply: visits, idx, p, the position before (black, white, side), the games after (astuple),
    and the counters after."""
    seeds = [SEED0 + i for i in range(len(games))]
    orc = OracleGames(O, seeds, S, T, bs=bs, batch=B, games=games)
    n = len(games)
    nply, done, draws = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32)
    out = []
    for _ in range(plies):
        before = [g.astuple() for g in orc.games]
        vis, idx, p, _ = orc.ply(ev)
        log = [c.copy() for c in orc.leaf_log]
        for j in range(n):
            if before[j][3]:
                assert idx[j] == -2
                continue
            draws[j] += O.action_needs_draw(vis[j], T)
        nply += idx >= 0
        after = [g.astuple() for g in orc.games]
        if reset:
            for j, g in enumerate(orc.games):
                if g.over:
                    done[j] += 1
                    seeds[j] += STRIDE
                    orc.games[j] = O.new_game(bs)
                    orc.mts[j] = O.MT(seeds[j] & 0xFFFFFFFF)
                    draws[j] = 0
        out.append({"vis": vis, "idx": idx, "p": p, "before": before, "after": after,
                    "state": [g.astuple() for g in orc.games], "plies": nply.copy(),
                    "done": done.copy(), "draws": draws.copy(), "seeds": list(seeds),
                    "log": log})
    return out


def _check_state(eng, want, what):
    b, w, st = _state(eng)
    got = [(int(b[j]), int(w[j]), *map(int, st[j])) for j in range(len(want))]
    # Game.astuple(): black, white, side, over, winner, passed (the status layout's order)
    assert got == want, (what, [j for j in range(len(want)) if got[j] != want[j]])


def _check_pass_rows(kinds, ply0):
    """What the oracle gave at the roots without a legal square, spelled out (so a change of the
    oracle cannot quietly move the expectation): no visits, an all-zero p, index 0, no draw, the
    position unchanged, the ply counted."""
    for j, k in enumerate(kinds):
        if k in ("pass0", "pass1", "full", "stuck"):
            assert not ply0["vis"][j].any() and not ply0["p"][j].any()
            assert ply0["idx"][j] == 0 and ply0["draws"][j] == 0
            assert ply0["after"][j] == ply0["before"][j] and ply0["plies"][j] == 1
        if k == "over":
            assert ply0["idx"][j] == -2 and ply0["plies"][j] == 0
            assert ply0["after"][j] == ply0["before"][j]


SHAPES = [(200, 64), (48, 16), (100, 8)]


@pytest.mark.parametrize("S,B", SHAPES, ids=[f"s{s}b{b}" for s, b in SHAPES])
@pytest.mark.parametrize("bs,kind", [(8, "h2"), (6, "h2"), (8, "table")])
def test_pull_style_at_set_roots(oracle, evaluators, bs, kind, S, B):
    """Two plies (search, act with apply, autoreset without reset) from the 32 roots, at
    temperature 1 and 0, with the memo and compaction off and on: everything equals the oracle.
    The second search starts from the applied state; with the memo on it takes the carried link
    where the first search expanded the child, and none across a refused move."""
    import rvz
    O = oracle
    ev = evaluators(kind, bs)
    kinds, games = roots(O, bs)
    seeds = [SEED0 + i for i in range(G)]
    for T in (1.0, 0.0):
        want = oracle_run(O, ev, games, S, B, T, bs, 2, reset=False)
        _check_pass_rows(kinds, want[0])
        assert want[0]["draws"].any() == (T > 0)
        for on in (False, True):
            eng = rvz.Engine(G, S, B, board_size=bs, compact_leaves=on, memo=on)
            _set(eng, games, seeds)
            sd = torch.tensor(seeds, dtype=torch.int64, device="cuda")
            nply = torch.zeros(G, dtype=torch.int64, device="cuda")
            done = torch.zeros(G, dtype=torch.int64, device="cuda")
            for k, wk in enumerate(want):
                what = (bs, kind, S, B, T, on, k)
                eng.search(ev)
                vis = eng.visits().cpu().numpy().copy()
                idx, p = eng.act(T, apply=True)
                eng.autoreset(idx, sd, STRIDE, nply, done, reset=False)
                idx, p = idx.cpu().numpy(), p.cpu().numpy()
                assert np.array_equal(vis, wk["vis"]), what
                assert np.array_equal(idx, wk["idx"]), (what, idx, wk["idx"])
                assert np.array_equal(p.view(np.int64), wk["p"].view(np.int64)), what
                _check_state(eng, wk["state"], what)
                assert np.array_equal(eng.draws().cpu().numpy(), wk["draws"]), what
                assert np.array_equal(nply.cpu().numpy(), wk["plies"]), what
                assert np.array_equal(done.cpu().numpy(), wk["done"]) and not wk["done"].any()
            assert sd.tolist() == seeds
            eng.check()


def _pull(ev, games, S, B, bs, plies, reset, skip):
    """The pull-style run the fused launch must equal: per ply the position before, idx, p."""
    import rvz
    eng = rvz.Engine(G, S, B, board_size=bs, compact_leaves=True, memo=True)
    seeds = [SEED0 + i for i in range(G)]
    _set(eng, games, seeds)
    sd = torch.tensor(seeds, dtype=torch.int64, device="cuda")
    nply = torch.zeros(G, dtype=torch.int64, device="cuda")
    done = torch.zeros(G, dtype=torch.int64, device="cuda")
    hist, rb, rw, rs, rp = [], [], [], [], []
    for _ in range(plies):
        b, w, st = eng.get_state()
        rb.append(b.clone()); rw.append(w.clone()); rs.append(st[:, 0].clone())
        eng.search(ev, skip_last_eval=skip)
        idx, p = eng.act(1.0, apply=True)
        hist.append(idx.clone()); rp.append(p.clone())
        eng.autoreset(idx, sd, STRIDE, nply, done, reset=reset)
    eng.check()
    return {"hist": torch.stack(hist), "rb": torch.stack(rb), "rw": torch.stack(rw),
            "rs": torch.stack(rs), "rp": torch.stack(rp),
            "state": [t.clone() for t in eng.get_state()], "plies": nply, "done": done,
            "seeds": sd, "draws": eng.draws().clone()}


def _fused(ev, games, S, B, bs, plies, reset, skip, gpw, budget=None, eng=None):
    """One rvz_play launch from `games` on a new engine, or on `eng` with its counters zeroed."""
    import rvz
    n = len(games)
    if eng is None:
        eng = rvz.Engine(n, S, B, board_size=bs, memo=True)
    elif getattr(eng, "play_rows", None) is not None:
        eng.play_rows.zero_()
        eng.play_unread.zero_()
    seeds = [SEED0 + i for i in range(n)]
    _set(eng, games, seeds)
    sd = torch.tensor(seeds, dtype=torch.int64, device="cuda")
    nply = torch.zeros(n, dtype=torch.int64, device="cuda")
    done = torch.zeros(n, dtype=torch.int64, device="cuda")
    hist = torch.full((plies, n), -9, dtype=torch.int32, device="cuda")
    rb = torch.zeros(plies, n, dtype=torch.int64, device="cuda")
    rw = torch.zeros_like(rb)
    rs = torch.zeros(plies, n, dtype=torch.int32, device="cuda")
    rp = torch.zeros(plies, n, eng.npol, dtype=torch.float64, device="cuda")
    eng.play(ev, plies, 1.0, sd, STRIDE, nply, done, reset=reset, skip_last_eval=skip, hist=hist,
             games_per_workgroup=gpw, budget=budget, records=(rb, rw, rs, rp))
    eng.check()
    assert not ev.overflowed()
    return {"hist": hist, "rb": rb, "rw": rw, "rs": rs, "rp": rp,
            "state": [t.clone() for t in eng.get_state()], "plies": nply, "done": done,
            "seeds": sd, "draws": eng.draws().clone(), "rows": int(eng.play_rows.item()),
            "unread": int(eng.play_unread.item())}


@pytest.mark.parametrize("reset", [False, True], ids=["keep", "reset"])
@pytest.mark.parametrize("bs,S,B", [(8, 200, 64), (8, 48, 16), (6, 200, 64), (6, 48, 16)])
def test_fused_at_set_roots(oracle, evaluators, bs, S, B, reset):
    """rvz_play, two plies from the 32 roots, with games_per_workgroup 1 and -4 and
    skip_last_eval off and on: hist, records, state, counters, seeds and draws equal the
    pull-style run, which equals the oracle. Without reset a game that is over reports -2 in both
    plies and is left untouched; with reset it restarts with its slot's next seed."""
    O = oracle
    ev = evaluators("h2", bs)
    kinds, games = roots(O, bs)
    want = oracle_run(O, ev, games, S, B, 1.0, bs, 2, reset=reset)
    _check_pass_rows(kinds, want[0])
    over = [j for j, k in enumerate(kinds) if k == "over"]
    for skip in (False, True):
        pull = _pull(ev, games, S, B, bs, 2, reset, skip)
        # the pull-style run against the oracle
        for k, wk in enumerate(want):
            assert np.array_equal(pull["hist"][k].cpu().numpy(), wk["idx"]), (k, skip)
            assert np.array_equal(pull["rp"][k].cpu().numpy().view(np.int64),
                                  wk["p"].view(np.int64)), (k, skip)
            bb = pull["rb"][k].cpu().numpy().view(np.uint64)
            ww = pull["rw"][k].cpu().numpy().view(np.uint64)
            ss = pull["rs"][k].cpu().numpy()
            assert [(int(bb[j]), int(ww[j]), int(ss[j])) for j in range(G)] == \
                [t[:3] for t in wk["before"]], (k, skip)
        last = want[-1]
        b, w, st = (t.cpu().numpy() for t in pull["state"])
        assert [(int(b.view(np.uint64)[j]), int(w.view(np.uint64)[j]), *map(int, st[j]))
                for j in range(G)] == last["state"]
        assert np.array_equal(pull["plies"].cpu().numpy(), last["plies"])
        assert np.array_equal(pull["done"].cpu().numpy(), last["done"])
        assert pull["seeds"].tolist() == last["seeds"]
        assert np.array_equal(pull["draws"].cpu().numpy(), last["draws"])
        if reset:
            assert all(last["done"][j] == 1 and last["seeds"][j] == SEED0 + j + STRIDE
                       for j in over)
        else:
            assert not last["done"].any()
            for j in over:
                assert pull["hist"][:, j].tolist() == [-2, -2]
                assert last["state"][j] == games[j].astuple()
        for gpw in (1, -4):
            got = _fused(ev, games, S, B, bs, 2, reset, skip, gpw)
            for key in ("hist", "rb", "rw", "rs", "plies", "done", "seeds", "draws"):
                assert torch.equal(got[key], pull[key]), (key, skip, gpw)
            assert torch.equal(got["rp"].view(torch.int64), pull["rp"].view(torch.int64)), \
                (skip, gpw)
            for x, y in zip(got["state"], pull["state"]):
                assert torch.equal(x, y), (skip, gpw)


# ---------------------------------------------------------------- the unread-rows threshold
LS = (2, 3, 4, 5)


def threshold_roots(O, bs):
    """Four playout positions with exactly L legal moves for each L in LS (one per playout, at
    least 10 empties so that the root's children are ordinary leaves), grouped by L."""
    want = {L: [] for L in LS}
    seed = 0
    while any(len(v) < 4 for v in want.values()):
        rng = random.Random(seed)
        seed += 1
        g = O.new_game(bs)
        while not g.over:
            moves = list(R.squares(R.mover_mask(g, bs)))
            if len(moves) in want and len(want[len(moves)]) < 4 and R.empties(g, bs) >= 10 \
                    and rng.random() < 0.3:
                want[len(moves)].append(g.copy())
                break
            assert O.make_move(g, rng.choice(moves), bs)
    return [g for L in LS for g in want[L]]


def rows_by_rule(log, L, over, E, skip):
    """(rows, unread) per game from the oracle's leaf log (the copies waiting for the game's row
    in every batch), by the rule of test_gpu_unread_rows._row_bound: with skip_last_eval the last
    batch's row is never evaluated (E >= 2) and, where L >= E - 1, neither is any row after the
    root's; the rows between the first and the last batch are then the unread ones."""
    n = len(L)
    rows, unread = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for g in range(n):
        if over[g]:
            continue
        rule = skip and L[g] >= E - 1
        for k in range(E):
            if log[k][g] <= 0 or (skip and E > 1 and k == E - 1):
                continue
            if rule and k >= 1:
                unread[g] += 1
            else:
                rows[g] += 1
    return rows, unread


@pytest.mark.parametrize("bs", [8, 6])
def test_unread_rule_threshold(oracle, evaluators, bs):
    """Roots with L = 2, 3, 4, 5 legal moves (four each), one fused ply at batch 16 with S such
    that E - 1 is L - 1, L and L + 1 for every group, and the same with a remainder batch of 11
    (E = ceil(S / B), the last batch min(B, S - k B) traversals). Each group is launched on its
    own (a ply budget of 1 for its games, 0 for the others), so the counters are per group."""
    import rvz
    O = oracle
    ev = evaluators("h2", bs)
    games = threshold_roots(O, bs)
    n, B = len(games), 16
    L = np.array([bin(R.mover_mask(g, bs)).count("1") for g in games])
    assert L.tolist() == [x for x in LS for _ in range(4)]
    sims = sorted({16 * k for k in range(2, 8)} | {16 * (x + 1) - 5 for x in LS})
    fired = set()
    for S in sims:
        E = -(-S // B)
        want = oracle_run(O, ev, games, S, B, 1.0, bs, 1, reset=False)[0]
        assert len(want["log"]) == E
        eng = rvz.Engine(n, S, B, board_size=bs, memo=True)
        for gi, Lg in enumerate(LS):
            sel = np.arange(4 * gi, 4 * gi + 4)
            budget = torch.zeros(n, dtype=torch.int32, device="cuda")
            budget[sel.tolist()] = 1
            runs = {}
            for skip in (True, False):
                got = runs[skip] = _fused(ev, games, S, B, bs, 1, False, skip, -4, budget=budget,
                                          eng=eng)
                hist = got["hist"][0].cpu().numpy()
                assert np.array_equal(hist[sel], want["idx"][sel]), (S, Lg, skip)
                assert (np.delete(hist, sel) == -9).all()
                assert np.array_equal(got["rp"][0].cpu().numpy()[sel].view(np.int64),
                                      want["p"][sel].view(np.int64)), (S, Lg, skip)
                rows, unread = rows_by_rule([c[sel] for c in want["log"]], L[sel],
                                            [False] * 4, E, skip)
                print(f"{bs}x{bs} S {S} (E {E}) L {Lg} skip {skip}: rows {got['rows']} "
                      f"(rule {rows.sum()}), unread {got['unread']} (rule {unread.sum()})")
                assert got["rows"] == rows.sum(), (S, Lg, skip, got["rows"], rows)
                assert got["unread"] == unread.sum(), (S, Lg, skip, got["unread"], unread)
            for key in ("hist", "rb", "rw", "rs", "plies", "done", "seeds", "draws"):
                assert torch.equal(runs[True][key], runs[False][key]), (key, S, Lg)
            assert torch.equal(runs[True]["rp"].view(torch.int64),
                               runs[False]["rp"].view(torch.int64))
            for x, y in zip(runs[True]["state"], runs[False]["state"]):
                assert torch.equal(x, y)
            assert runs[False]["unread"] == 0
            fires = Lg >= E - 1 and E >= 3
            assert (runs[True]["unread"] > 0) == fires, (S, E, Lg, runs[True]["unread"])
            if fires:
                fired.add((Lg, E - 1 - Lg))
    # the rule fired with E - 1 == L for every group, and with E - 1 == L - 1 where E >= 3 allows
    for Lg in LS:
        assert {d for (x, d) in fired if x == Lg} >= ({0, -1} if Lg > 2 else {0}), (Lg, fired)
