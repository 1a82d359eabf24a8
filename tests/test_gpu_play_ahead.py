"""Ahead rows of the fused self-play kernel (k_play<64, 2, 2, 4, 8, 2>, rvz_play_ahead; DESIGN
§5.3): a trunk pass left with one live board evaluates, in its empty board slot, the row a game
of the group will ask for next (the next unvisited child of an expanded root with fewer legal
moves than the search has batches after the first), and the search takes that row from the game's
ahead slot when it queues a leaf with the same (P, O, V) key.

A row's outputs depend only on its position, so nothing a game computes may change: the launch
with the switch on (1: fill empty slots; 2: also instead of holding an odd row) is held against
the switch off and against the pull-style loop (search + act + autoreset, k_resnet_h2's passes),
array for array: every ply's move, f64 policy and recorded position, the final boards and status,
the ply and game counters, the seeds and the draws. The counters prove the path ran: rows taken
> 0 and rows evaluated ahead >= rows taken. 8x8, the 6x64 net and 800 simulations (13 batches), so
that the visits depend on the net; 6 games (one group of play_group -6) and 14 (two groups and a
short one)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

S, B, GROUP = 800, 64, -6
TABLE = (1 << 14, 14)
# the stagger: plies each of the 14 games has played when the compared launch starts, from the
# opening to the last moves of a game (so that games end and restart inside the launch)
BUDGET = [3, 11, 19, 27, 35, 43, 48, 51, 53, 55, 56, 57, 58, 59]

_EV = []


def _ev():
    import rvz
    if not _EV:
        torch.manual_seed(0)
        _EV.append(rvz.LeafEvaluator(rvz.AlphaZeroNetwork(8, 6, 64).cuda().eval()))
    return _EV[0]


def _engine(G, start, ahead=None, table=False):
    import rvz
    eng = rvz.Engine(G, S, B, memo=True)
    if table:
        eng.table(*TABLE)
    if ahead is not None:
        eng.ahead(ahead)
    seeds = torch.arange(G, dtype=torch.int64, device="cuda") + 42
    eng.reset(seeds)
    if start is not None:
        eng.set_state(*start)
    return eng, seeds


def _result(eng, seeds, nply, done, moves, p, black, white, side):
    eng.check()
    assert not _ev().overflowed()
    return dict(moves=moves, p=p, black=black, white=white, side=side, plies=nply, done=done,
                seeds=seeds, draws=eng.draws().clone(),
                state=[t.clone() for t in eng.get_state()])


def _fused(G, plies, ahead, start=None, table=False):
    """One fused launch of `plies` plies with records; the row and ahead counters ride along."""
    ev = _ev()
    eng, seeds = _engine(G, start, ahead, table)
    nply = torch.zeros(G, dtype=torch.int64, device="cuda")
    done = torch.zeros_like(nply)
    hist = torch.full((plies, G), -9, dtype=torch.int32, device="cuda")
    rb = torch.zeros(plies, G, dtype=torch.int64, device="cuda")
    rw = torch.zeros_like(rb)
    rs = torch.zeros(plies, G, dtype=torch.int32, device="cuda")
    rp = torch.zeros(plies, G, eng.npol, dtype=torch.float64, device="cuda")
    eng.play(ev, plies, 1.0, seeds, G, nply, done, reset=True, skip_last_eval=True, hist=hist,
             games_per_workgroup=GROUP, records=(rb, rw, rs, rp), skip_forced_roots=True)
    out = _result(eng, seeds, nply, done, hist, rp, rb, rw, rs)
    issued, taken = eng.play_ahead.tolist()
    out.update(rows=int(eng.play_rows.item()), issued=issued, taken=taken,
               forced=int(eng.play_roots_unread.item()), hits=int(eng.table_stats[0].item()))
    return out


def _pull(G, plies, start=None):
    """The pull-style loop: per ply the position, a search (one launch per batch, the h2
    evaluator's own kernels), the act and the autoreset bookkeeping."""
    ev = _ev()
    eng, seeds = _engine(G, start)
    nply = torch.zeros(G, dtype=torch.int64, device="cuda")
    done = torch.zeros_like(nply)
    moves, p, black, white, side = [], [], [], [], []
    for _ in range(plies):
        b, w, st = eng.get_state()
        black.append(b.clone())
        white.append(w.clone())
        side.append(st[:, 0].clone())
        eng.search(ev, fused_softmax=True, skip_last_eval=True)
        idx, _ = eng.act(1.0, apply=True)
        moves.append(idx.clone())
        p.append(eng.p_buf.clone())
        eng.autoreset(idx, seeds, G, nply, done, reset=True)
    return _result(eng, seeds, nply, done, *(torch.stack(t) for t in (moves, p, black, white,
                                                                    side)))


def _same(a, b):
    for k in range(a["moves"].shape[0]):
        assert torch.equal(a["moves"][k], b["moves"][k]), f"ply {k}: moves differ"
        assert torch.equal(a["p"][k].view(torch.int64), b["p"][k].view(torch.int64)), \
            f"ply {k}: policy vectors differ"
    for x, y in zip(a["state"], b["state"]):     # boards, status
        assert torch.equal(x, y)
    for k in ("black", "white", "side", "plies", "done", "seeds", "draws"):
        assert torch.equal(a[k], b[k]), k


def _ran(on, off):
    """The ahead path did something, and the accounting holds: rows taken > 0, every one of them
    evaluated ahead, and play_rows counts the ahead rows as the rows they are."""
    print(f"rows {off['rows']} -> {on['rows']}; ahead rows {on['issued']}, taken {on['taken']}")
    assert off["issued"] == 0 and off["taken"] == 0
    assert on["taken"] > 0 and on["issued"] >= on["taken"]
    assert on["rows"] + on["taken"] - on["issued"] == off["rows"]


@pytest.fixture(scope="module")
def mid_game():
    """Seeded mid-game positions for 14 games: game g after BUDGET[g] plies of its seed's game,
    played by the fused launch with the switch off. Read-only."""
    G = len(BUDGET)
    eng, seeds = _engine(G, None, 0)
    nply = torch.zeros(G, dtype=torch.int64, device="cuda")
    done = torch.zeros_like(nply)
    bud = torch.tensor(BUDGET, dtype=torch.int32, device="cuda")
    eng.play(_ev(), max(BUDGET), 1.0, seeds, G, nply, done, reset=True, skip_last_eval=True,
             games_per_workgroup=GROUP, budget=bud, skip_forced_roots=True)
    eng.check()
    assert torch.equal(nply.cpu(), bud.cpu().long())
    black, white, status = (t.clone() for t in eng.get_state())
    # the last game: a hand-made position with a pass in it whatever black plays. Black (to move)
    # holds squares 0 and 63, white 1 and 62; black takes square 2 or 61, white is left with one
    # disc and no move, black moves again and the game ends
    black[-1] = (1 << 0) | -(1 << 63)
    white[-1] = (1 << 1) | (1 << 62)
    status[-1] = torch.tensor([1, 0, -1, 0], dtype=torch.int32)
    return [black, white, status]


_REF = {}


def _refs(G, plies, start, key):
    """The pull-style loop's and the switched-off launch's arrays of a case, computed once."""
    if key not in _REF:
        _REF[key] = (_pull(G, plies, start), _fused(G, plies, 0, start))
        _same(_REF[key][1], _REF[key][0])
    return _REF[key]


@pytest.mark.parametrize("mode", [1, 2], ids=["fill", "fill_no_hold"])
@pytest.mark.parametrize("G", [6, 14, 5, 11])
def test_from_the_start_position(G, mode):
    """Four plies from the start position: every root has fewer than 12 legal moves, so every
    search after its root's row sends its next batches to fresh children, one by one.
    Groups of 6, 6 + 6 + 2, 5 and 6 + 5 games. Without the table the games of a group walk
    through those batches in lockstep, each queueing one row per cycle, so a group of 6 or 2 has
    an even row count in every such cycle and no board slot is ever empty while a fresh child is
    left: measured on MI355X, 6 and 14 games evaluate 0 ahead rows (206 rows either way), and no
    rule that uses empty board slots only can do otherwise. There the arrays and the row
    accounting are held, and the path is shown at work from the same position by the groups of 5
    (an odd row count from the first cycle on: the odd row is held back a cycle by mode 1,
    which so stays idle too, and takes a fresh child's row along in mode 2) and by
    test_with_the_cross_game_table[start] (14 games, mode 1; table hits break the lockstep)."""
    pull, off = _refs(G, 4, None, ("start", G))
    on = _fused(G, 4, mode)
    _same(on, off)
    _same(on, pull)
    if G % 6 == 5 and mode == 2:
        _ran(on, off)
    else:
        print(f"rows {off['rows']} -> {on['rows']}; ahead rows {on['issued']}, taken {on['taken']}")
        assert off["issued"] == 0 and on["issued"] >= on["taken"]
        assert on["rows"] + on["taken"] - on["issued"] == off["rows"]


@pytest.mark.parametrize("mode", [1, 2], ids=["fill", "fill_no_hold"])
def test_from_a_mid_game_stagger(mid_game, mode):
    """Six plies of 14 games between their 3rd and their 59th ply: forced searches (roots of 12
    legal moves or more), searches that take ahead rows, passes and games that end and restart
    share the groups."""
    G, plies = len(BUDGET), 6
    pull, off = _refs(G, plies, mid_game, ("mid", G))
    on = _fused(G, plies, mode, mid_game)
    _same(on, off)
    _same(on, pull)
    _ran(on, off)
    side, done = on["side"].cpu(), on["done"].cpu()
    discs = torch.tensor([[bin((int(b) | int(w)) & (2 ** 64 - 1)).count("1") for b, w in zip(rb, rw)]
                          for rb, rw in zip(on["black"].cpu(), on["white"].cpu())])
    # a pass: the same side moves twice in a row in one game (one disc more, no restart between)
    passes = int(((side[1:] == side[:-1]) & (discs[1:] == discs[:-1] + 1)).sum())
    print(f"forced searches {on['forced']}, games ended {int(done.sum())}, passes {passes}")
    assert on["forced"] > 0 and int(done.sum()) > 0 and passes > 0


@pytest.mark.parametrize("case", ["start", "mid"])
def test_with_the_cross_game_table(mid_game, case):
    """The same with rvz_play_table on: an ahead row of a table position is stored there like any
    evaluated row, a leaf takes its ahead row before it looks into the table, and the games stay
    the pull-style loop's."""
    G = len(BUDGET)
    plies, start = (4, None) if case == "start" else (6, mid_game)
    pull, _ = _refs(G, plies, start, (case, G))
    off = _fused(G, plies, 0, start, table=True)
    on = _fused(G, plies, 1, start, table=True)
    _same(on, off)
    _same(on, pull)
    print(f"rows {off['rows']} -> {on['rows']}; ahead rows {on['issued']}, taken {on['taken']}; "
          f"table hits {off['hits']} -> {on['hits']}")
    assert off["hits"] > 0 and on["hits"] > 0
    assert off["issued"] == 0 and on["taken"] > 0 and on["issued"] >= on["taken"]


def test_no_ahead_rows_without_the_one_board_pass(monkeypatch):
    """RVZ_PLAY_SINGLE_PASS=0 is the pair shape everywhere, the launch as it was before either
    change: the ahead switch does nothing there (no row evaluated ahead, the same arrays)."""
    monkeypatch.setenv("RVZ_PLAY_SINGLE_PASS", "0")
    G = 14
    pull, _ = _refs(G, 4, None, ("start", G))
    off = _fused(G, 4, 0)
    on = _fused(G, 4, 1)
    _same(on, off)
    _same(on, pull)
    assert on["issued"] == 0 and on["taken"] == 0 and on["rows"] == off["rows"]
