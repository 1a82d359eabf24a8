"""The ready schedule of the fused self-play launch (rvz_play's task queue).

A workgroup takes the least-advanced game group whose previous ply is published instead of the
next (group, ply) in a fixed order. Which workgroup plays which task, and when, must not show in
the result: every launch here is held against the static schedule (each workgroup owns its games
for all plies) on the same seeds. The shapes are the ones where the schedule's paths differ:
more groups than resident workgroups with tasks of very different length (ply budgets 0..4),
fewer groups than workgroups (a workgroup that finds nothing ready waits and rescans), a single
group, a short last group, graph replays (the group words are reset by the launch's fill), and
forced searches."""
import pytest
import torch

from test_gpu_forced_roots import _ev, _play, _same_games

pytestmark = pytest.mark.gpu

S, B = 192, 64


def _budgets(G, top):
    return (torch.arange(G, device="cuda") % (top + 1)).to(torch.int32).contiguous()


# (board, filters, games, group): 600 groups of one game for the 512 resident workgroups; packed
# 6x6 boards in groups of 24; the 128-filter form (one board per pass, the pass gate at its
# default) in groups of 16 with a short last group
UNEVEN = [(8, 64, 600, -1), (6, 64, 600, -24), (8, 128, 600, -16)]


@pytest.mark.parametrize("key", UNEVEN, ids=[f"{k[0]}x{k[0]}_f{k[1]}_group{-k[3]}" for k in UNEVEN])
def test_same_games_with_uneven_tasks(key):
    """Four plies with per-game budgets cycling through 0..4: some tasks are empty, some full.
    hist is written exactly below each game's budget, the ply counters equal the budgets, and
    moves, policies, positions, final boards, status, seeds and draws equal the static
    schedule's."""
    board, filters, G, gpw = key
    ev = _ev(board, 1, filters)
    plies = 4
    bud = _budgets(G, plies)
    queue = _play(ev, G, S, [(plies, bud)], False, gpw)
    static = _play(ev, G, S, [(plies, bud)], False, 8)
    _same_games(queue, static)
    assert torch.equal(queue["plies"].cpu(), bud.cpu().long())
    hist = queue["moves"].cpu()
    below = torch.arange(plies).view(plies, 1) < bud.cpu().view(1, G)
    assert (hist[below] >= 0).all()
    assert (hist[~below] == -9).all()


@pytest.mark.parametrize("G,gpw", [(40, -6), (5, -6)], ids=["7_groups_last_short", "one_group"])
def test_fewer_groups_than_workgroups(G, gpw):
    """Seven groups (the last of four games) and a single group, five plies: as many workgroups
    as groups, so a workgroup whose group is taken waits, rescans and picks again."""
    ev = _ev()
    queue = _play(ev, G, S, [(5, None)], False, gpw)
    static = _play(ev, G, S, [(5, None)], False, 8)
    _same_games(queue, static)
    assert (queue["moves"] >= 0).all()
    assert torch.equal(queue["plies"].cpu(), torch.full((G,), 5, dtype=torch.int64))


def _runner(G, sims, group, forced=None):
    import rvz
    eng = rvz.Engine(G, sims, B, memo=True)
    run = rvz.SelfPlayRunner(eng, _ev(), autoreset=True, seed_base=42, skip_last_eval=True,
                             fused=True, skip_forced_roots=forced)
    run.play_group = group
    run.start()
    return eng, run


def test_graph_replays_reset_the_group_words():
    """A captured 3-ply launch (96 games in groups of 6) replayed three times: every replay
    commits 3 plies of every game, so both halves of every group word are inside the launch's
    fill (the small twin of test_fused_graph_replays_keep_playing)."""
    G = 96
    eng, run = _runner(G, S, -6)
    run._body(3)
    run.capture(plies=3)
    for _ in range(3):
        before = run._plies.clone()
        run.ply()
        torch.cuda.synchronize()
        assert torch.equal(run._plies - before, torch.full_like(before, 3))
        run.check()


def test_forced_searches_on():
    """The fused runner with forced searches (its default), 192 games x 256 simulations, six
    plies: the queue's games and row counters equal the static schedule's, and against the queue
    with the switch off rows + roots_unread add up as in test_gpu_forced_roots."""
    out = {}
    for name, group, forced in (("queue", 0, None), ("static", 4, None), ("off", 0, False)):
        eng, run = _runner(192, 256, group, forced)
        run._body(6)
        run.check()
        out[name] = (int(eng.play_rows.item()), int(eng.play_roots_unread.item()),
                     int(eng.play_unread.item()),
                     [run._plies.clone(), run._done.clone(), run.seeds.clone(), eng.p_buf.clone(),
                      eng.idx_buf.clone(), eng.draws().clone()] +
                     [t.clone() for t in eng.get_state()])
    for other in ("static", "off"):
        for x, y in zip(out["queue"][3], out[other][3]):
            assert torch.equal(x, y), other
    assert out["queue"][:3] == out["static"][:3]
    rows, roots, unread = out["queue"][:3]
    assert roots > 0 and out["off"][1] == 0
    assert rows + roots == out["off"][0], (rows, roots, out["off"][0])
    assert unread == out["off"][2]
