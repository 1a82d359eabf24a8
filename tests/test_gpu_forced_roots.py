"""The forced searches of the fused self-play launch (rvz_play with skip_last_eval and
skip_forced_roots).

A search of E = ceil(S / B) >= 2 batches whose root is not over and has L >= E - 1 legal moves
sends every batch after the first whole to the next unvisited root child (§2.13,
test_gpu_unread_rows), so its visit counts are fixed by the move order alone: B on each of the
first E - 2 children, the remainder batch on child E - 2. With the switch on k_play writes that
tree in one step: no root row, no walk. The games must be those of the run with the switch off
(and of the literal oracle); only rows may differ, and they must add up:
rows(on) + roots_unread(on) == rows(off), rows_unread(on) == rows_unread(off)."""
import numpy as np
import pytest
import torch

from oracle_play import OracleGames

pytestmark = pytest.mark.gpu

# (board, blocks, filters, games, sims, plies, group): the shapes of test_gpu_unread_rows.PARENT_ROWS
SHAPES = [(8, 1, 64, 96, 800, 40, -6), (8, 1, 64, 64, 200, 3, -4), (6, 1, 64, 72, 400, 24, -6),
          (8, 2, 128, 32, 800, 30, -4)]


def _net(board, blocks, filters, seed=0):
    import rvz
    torch.manual_seed(seed)
    return rvz.AlphaZeroNetwork(board, blocks, filters).cuda().eval()


_EVS = {}


def _ev(board=8, blocks=1, filters=64):
    import rvz
    key = (board, blocks, filters)
    if key not in _EVS:
        _EVS[key] = rvz.LeafEvaluator(_net(*key))
    return _EVS[key]


def _play(ev, G, S, launches, forced, gpw, table=None, setup=None, seed_base=42, B=64,
          games=None, reset=True):
    """Fused launches with records on a new engine. launches: [(plies, budget or None)], played
    one after another. Returns every act's move, f64 policy and position, the final state, the
    counters, seeds, draws and the row counters."""
    import rvz
    eng = rvz.Engine(G, S, B, board_size=ev.board_size, memo=True)
    if table:
        eng.table(*table)
    if setup:
        setup(eng)
    seeds = torch.arange(G, dtype=torch.int64, device="cuda") + seed_base
    eng.reset(seeds)
    if games is not None:
        import solve_ref as R
        eng.set_state(*R.to_device(games))
    nply = torch.zeros(G, dtype=torch.int64, device="cuda")
    done = torch.zeros(G, dtype=torch.int64, device="cuda")
    out = {k: [] for k in ("moves", "p", "black", "white", "side")}
    for plies, budget in launches:
        hist = torch.full((plies, G), -9, dtype=torch.int32, device="cuda")
        rb = torch.zeros(plies, G, dtype=torch.int64, device="cuda")
        rw = torch.zeros_like(rb)
        rs = torch.zeros(plies, G, dtype=torch.int32, device="cuda")
        rp = torch.zeros(plies, G, eng.npol, dtype=torch.float64, device="cuda")
        eng.play(ev, plies, 1.0, seeds, G, nply, done, reset=reset, skip_last_eval=True,
                 hist=hist, games_per_workgroup=gpw, budget=budget, records=(rb, rw, rs, rp),
                 skip_forced_roots=forced)
        for k, t in zip(("moves", "p", "black", "white", "side"), (hist, rp, rb, rw, rs)):
            out[k].append(t)
    eng.check()
    assert not ev.overflowed()
    res = {k: torch.cat(v) for k, v in out.items()}
    res.update(state=[t.clone() for t in eng.get_state()], plies=nply, done=done, seeds=seeds,
               draws=eng.draws().clone(), rows=int(eng.play_rows.item()),
               unread=int(eng.play_unread.item()), roots=int(eng.play_roots_unread.item()),
               hits=int(eng.table_stats[0].item()))
    return res


def _same_games(a, b):
    for k in range(a["moves"].shape[0]):
        assert torch.equal(a["moves"][k], b["moves"][k]), f"ply {k}: moves differ"
        assert torch.equal(a["p"][k].view(torch.int64), b["p"][k].view(torch.int64)), \
            f"ply {k}: policy vectors differ"
    for x, y in zip(a["state"], b["state"]):     # boards, status
        assert torch.equal(x, y)
    for k in ("black", "white", "side", "plies", "done", "seeds", "draws"):
        assert torch.equal(a[k], b[k]), k


def _pair(ev, G, S, launches, gpw, **kw):
    on = _play(ev, G, S, launches, True, gpw, **kw)
    off = _play(ev, G, S, launches, False, gpw, **kw)
    _same_games(on, off)
    print(f"G {G} S {S}: rows {on['rows']} + {on['roots']} root rows left out == {off['rows']}; "
          f"child rows unread {on['unread']} / {off['unread']}")
    assert off["roots"] == 0
    assert on["unread"] == off["unread"]
    return on, off


# ------------------------------------------------------------ 1. equal games, exact accounting
@pytest.mark.parametrize("key", SHAPES, ids=[f"{k[0]}x{k[0]}_{k[1]}x{k[2]}_s{k[4]}" for k in SHAPES])
def test_same_games_and_exact_row_accounting(key):
    """The table is off and the memo on, so a root's row is left out exactly where the search
    is forced and its root carries no link: every such row is one row of the run without the
    switch."""
    board, blocks, filters, G, S, plies, gpw = key
    on, off = _pair(_ev(board, blocks, filters), G, S, [(plies, None)], gpw)
    assert on["roots"] > 0
    assert on["rows"] + on["roots"] == off["rows"], (on["rows"], on["roots"], off["rows"])


# ------------------------------------------------------------ 2. a window with no rows at all
def test_opening_window_evaluates_nothing(oracle):
    """64 games x 200 simulations (E = 4: forced from L >= 3), the first 3 plies: every root has
    at least 3 legal moves (test_gpu_unread_rows.test_rule_fires_in_every_search_of_the_opening),
    so every search is forced. A new game's first root carries no link, and a forced search from
    a root without one expands no child, so no later root of the window carries one either: all
    G * plies root rows are left out and no row is evaluated. 12 sampled games against the
    oracle, which evaluates its own leaves."""
    G, S, plies = 64, 200, 3
    ev = _ev()
    on, off = _pair(ev, G, S, [(plies, None)], -4)
    assert on["rows"] == 0
    assert on["roots"] == G * plies == off["rows"]
    sample = np.linspace(0, G - 1, 12).astype(int)
    orc = OracleGames(oracle, [42 + int(g) for g in sample], S)
    moves, p = on["moves"].cpu().numpy(), on["p"].cpu().numpy()
    for ply in range(plies):
        _, oi, op, _ = orc.ply(ev)
        assert np.array_equal(oi, moves[ply][sample]), ply
        assert np.array_equal(op.view(np.int64), p[ply][sample].view(np.int64)), ply


# ------------------------------------------------------------ 3. the threshold
@pytest.mark.parametrize("bs", [8, 6])
def test_threshold_and_visits(oracle, bs):
    """Roots with L = 2, 3, 4, 5 legal moves (four each, test_gpu_set_roots.threshold_roots), one
    ply at batch 16 with a remainder batch of 11 (S = 16 (E - 1) + 11, E - 1 = 1 .. 6) and
    without one (S = 64), each group launched on its own (ply budgets) so that the counters are
    per group: the four root rows are left out exactly where L >= E - 1, so for every L the
    groups with L = E - 2, E - 1 and E are all met. The visits (p * S at temperature 1) and the
    moves are the oracle's; the rows are those of the unread rule (rows_by_rule over the
    oracle's leaf log) less the roots'. A one-batch search (S = 16) evaluates its root."""
    from test_gpu_set_roots import LS, oracle_run, rows_by_rule, threshold_roots
    import solve_ref as R
    O, ev, B = oracle, _ev(bs), 16
    games = threshold_roots(O, bs)
    n = len(games)
    L = np.array([bin(R.mover_mask(g, bs)).count("1") for g in games])
    met = set()
    for S in (16, 27, 43, 59, 75, 91, 107, 64):
        E = -(-S // B)
        want = oracle_run(O, ev, games, S, B, 1.0, bs, 1, reset=False)[0]
        for gi, Lg in enumerate(LS):
            sel = np.arange(4 * gi, 4 * gi + 4)
            budget = torch.zeros(n, dtype=torch.int32, device="cuda")
            budget[sel.tolist()] = 1
            runs = {f: _play(ev, n, S, [(1, budget)], f, -4, B=B, games=games, reset=False,
                             seed_base=900) for f in (True, False)}
            _same_games(runs[True], runs[False])
            got = runs[True]
            assert np.array_equal(got["moves"][0].cpu().numpy()[sel], want["idx"][sel]), (S, Lg)
            p = got["p"][0].cpu().numpy()[sel]
            assert np.array_equal(p.view(np.int64), want["p"][sel].view(np.int64)), (S, Lg)
            # the children's visits add up to S less the first batch, which ends on the root
            tot = want["vis"][sel].sum(1, keepdims=True)
            assert (tot == (S - B if E >= 2 else 0)).all()
            assert np.array_equal(np.rint(p * tot).astype(np.int64), want["vis"][sel]), (S, Lg)
            if E >= 2 and Lg >= E - 1:   # the closed form: B per child in move order, then the rest
                for j in sel:
                    sq = list(R.squares(R.mover_mask(games[j], bs)))[:E - 1]
                    form = np.zeros(bs * bs + 1, np.int64)
                    form[sq] = [min(B, S - k * B) for k in range(1, E)]
                    assert np.array_equal(want["vis"][j], form), (S, Lg, j)
            rows, unread = rows_by_rule([c[sel] for c in want["log"]], L[sel], [False] * 4, E,
                                        True)
            fires = E >= 2 and Lg >= E - 1
            print(f"{bs}x{bs} S {S} (E {E}) L {Lg}: rows {got['rows']}, root rows left out "
                  f"{got['roots']}, unread {got['unread']} (rule: {rows.sum()}, {unread.sum()})")
            assert got["roots"] == (4 if fires else 0), (S, E, Lg, got["roots"])
            assert got["rows"] == rows.sum() - got["roots"], (S, Lg, got["rows"], rows)
            assert got["unread"] == unread.sum() == runs[False]["unread"], (S, Lg)
            assert runs[False]["rows"] == rows.sum() and runs[False]["roots"] == 0
            if E == 1:
                assert got["rows"] == 4
            else:
                met.add((Lg, E - 1 - Lg))
    for Lg in LS:    # E - 1 == L + 1 (off), L (on, at the threshold) and L - 1 (on)
        assert {d for (x, d) in met if x == Lg} >= {1, 0, -1}, (Lg, met)


@pytest.mark.parametrize("bs", [8, 6])
def test_roots_that_are_over_or_cannot_move(oracle, bs):
    """The 32 set roots of test_gpu_set_roots (one to six empties, roots whose mover has no legal
    square, full boards, finished games), two plies at S = 48, B = 16 (E = 3) with and without
    reset: a root that is over or has no legal square is never forced (L = 0 < E - 1) and the
    switch changes nothing but the rows."""
    from test_gpu_set_roots import roots
    _, games = roots(oracle, bs)
    for reset in (False, True):
        on, off = _pair(_ev(bs), len(games), 48, [(2, None)], -4, B=16, games=games, reset=reset,
                        seed_base=900)
        assert on["rows"] + on["roots"] == off["rows"]


# ------------------------------------------------------------ 4. options with the switch on
G4, S4, P4 = 48, 400, 16      # E = 7: forced from L >= 6, a mix of forced and walked searches


def _mixed(on, off):
    assert 0 < on["roots"] and on["rows"] > 0
    assert on["rows"] + on["roots"] == off["rows"]


def test_root_noise():
    """The noise goes into priors a forced search never reads; the walked searches mix it."""
    on, off = _pair(_ev(), G4, S4, [(P4, None)], -4, setup=lambda e: e.root_noise(0.3, 0.25, 7))
    _mixed(on, off)
    plain = _play(_ev(), G4, S4, [(P4, None)], True, -4)
    assert not torch.equal(plain["moves"], on["moves"])      # the noise is on


def test_temperature_schedule():
    on, off = _pair(_ev(), G4, S4, [(P4, None)], -4,
                    setup=lambda e: e.temperature_schedule(6, 0.0))
    _mixed(on, off)
    assert int(on["draws"].max()) <= 6                       # later moves draw nothing


def test_static_ownership():
    on, off = _pair(_ev(), G4, S4, [(P4, None)], 5)
    _mixed(on, off)
    _same_games(on, _play(_ev(), G4, S4, [(P4, None)], True, -4))


def test_ply_budgets_then_a_second_launch():
    """A stagger launch (game g commits g mod 7 plies of 6) and then 6 plies for every game."""
    bud = (torch.arange(G4, device="cuda") % 7).to(torch.int32).contiguous()
    on, off = _pair(_ev(), G4, S4, [(6, bud), (6, None)], -4)
    _mixed(on, off)
    assert torch.equal(on["plies"].cpu(), torch.minimum(bud.cpu(), torch.tensor(6)).long() + 6)


def _runner(forced, record, autoreset, G=G4, S=S4):
    import rvz
    eng = rvz.Engine(G, S, 64, memo=True)
    run = rvz.SelfPlayRunner(eng, _ev(), autoreset=autoreset, seed_base=42, skip_last_eval=True,
                             fused=True, record=record, skip_forced_roots=forced)
    run.play_group = -4
    run.start()
    return eng, run


def test_records_via_play_record():
    """Whole games through the fused recording runner (200 simulations: E = 4); the runner's
    default (None) is the switch on when fused with skip_last_eval."""
    recs = {}
    for forced in (None, False):
        eng, run = _runner(forced, True, False, G=24, S=200)
        assert run.skip_forced_roots == (forced is None)
        run.play_record(60)
        run.check()
        recs[forced] = (run, int(eng.play_rows.item()), int(eng.play_roots_unread.item()))
    (a, rows_a, roots_a), (b, rows_b, roots_b) = recs[None], recs[False]
    for k in ("rec_idx", "rec_black", "rec_white", "rec_side", "post_status"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.rec_p.view(torch.int64), b.rec_p.view(torch.int64))
    assert bool(a.post_status[:, 1].all())
    assert roots_b == 0 < roots_a and rows_a + roots_a == rows_b


def test_captured_graph_replayed_three_times():
    """Two plies per graph, three replays, against three eager launches of two plies and against
    the eager run with the switch off."""
    out = {}
    for mode in ("graph", "eager", "off"):
        eng, run = _runner(mode != "off", False, True)
        if mode == "graph":
            run.capture(plies=2)
        for _ in range(3):
            run.ply() if mode == "graph" else run._body(2)
        run.check()
        out[mode] = (int(eng.play_rows.item()), int(eng.play_roots_unread.item()),
                     int(eng.play_unread.item()), run._plies.clone(), run.seeds.clone(),
                     [t.clone() for t in eng.get_state()], eng.p_buf.clone(), eng.idx_buf.clone())
    for other in ("eager", "off"):
        for x, y in zip(out["graph"][3:5] + tuple(out["graph"][5]) + out["graph"][6:],
                        out[other][3:5] + tuple(out[other][5]) + out[other][6:]):
            assert torch.equal(x, y), other
    assert out["graph"][:3] == out["eager"][:3]
    assert out["graph"][1] > 0 and out["graph"][0] + out["graph"][1] == out["off"][0]


# ------------------------------------------------------------ 5. the table
def test_table_hits_account_for_every_row_not_evaluated():
    """With the cross-game table on (256 games x 800 simulations x 20 plies): a forced search
    takes no lookup, hit or insert, so every hit is still exactly one row not evaluated."""
    ev = _ev()
    G, S, plies = 256, 800, 20
    with_t = _play(ev, G, S, [(plies, None)], True, -6, table=(1 << 16, 14))
    plain = _play(ev, G, S, [(plies, None)], True, -6)
    _same_games(with_t, plain)
    assert with_t["hits"] > 0 and plain["roots"] > 0
    assert with_t["rows"] + with_t["hits"] == plain["rows"], \
        (with_t["rows"], with_t["hits"], plain["rows"])
    assert with_t["unread"] == plain["unread"] and with_t["roots"] == plain["roots"]
