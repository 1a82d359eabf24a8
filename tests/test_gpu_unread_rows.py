"""The unread rows of the fused self-play launch (rvz_play with skip_last_eval).

A child of the root with N == 0 scores inf (mcts.py:96-97), and a batch's 64 traversals all end
on one leaf, so every batch after a search's first goes whole to the next unvisited root child
for as long as one exists. With E = ceil(S / 64) batches and L legal moves at the root, L >= E - 1
means no selection of that search ever compares two visited children: the visit counts (64 per
child in move order, the remainder on the last) do not depend on any child's NN row, and the tree
is dropped after the act. k_play then evaluates the root's row only. The games must be the games
of the run that evaluates every row (skip_last_eval=False) and of the literal oracle, which
evaluates its own leaves; only the number of evaluated rows may differ.

PARENT_ROWS: play_rows of the commit before the rule, measured with that commit's library for the
same arguments with skip_last_eval=False, where the rule must change nothing."""
import numpy as np
import pytest
import torch

from oracle_play import OracleGames

pytestmark = pytest.mark.gpu

# (board, blocks, filters, games, sims, plies, group): play_rows with skip_last_eval=False
PARENT_ROWS = {
    (8, 1, 64, 96, 800, 40, -6): 42412,
    (8, 1, 64, 64, 200, 3, -4): 640,
    (6, 1, 64, 72, 400, 24, -6): 9993,
    (8, 2, 128, 32, 800, 30, -4): 10330,
}


def _net(board, blocks, filters, seed=0):
    import rvz
    torch.manual_seed(seed)
    return rvz.AlphaZeroNetwork(board, blocks, filters).cuda().eval()


def _play(ev, G, S, plies, skip, gpw, table=None, seed_base=42):
    """One fused launch of `plies` plies with records: every act's move, f64 policy vector and
    the position before it, the final state, the counters, the rows."""
    import rvz
    eng = rvz.Engine(G, S, 64, board_size=ev.board_size, memo=True)
    if table:
        eng.table(*table)
    run = rvz.SelfPlayRunner(eng, ev, autoreset=True, seed_base=seed_base, skip_last_eval=skip,
                             fused=True)
    run.start()
    hist = torch.full((plies, G), -9, dtype=torch.int32, device="cuda")
    rb = torch.zeros(plies, G, dtype=torch.int64, device="cuda")
    rw = torch.zeros_like(rb)
    rs = torch.zeros(plies, G, dtype=torch.int32, device="cuda")
    rp = torch.zeros(plies, G, eng.npol, dtype=torch.float64, device="cuda")
    eng.play(ev, plies, 1.0, run.seeds, run.seed_stride, run._plies, run._done, reset=True,
             skip_last_eval=skip, hist=hist, games_per_workgroup=gpw, records=(rb, rw, rs, rp))
    eng.check()
    assert not ev.overflowed()
    return {"moves": hist, "p": rp, "black": rb, "white": rw, "side": rs,
            "state": eng.get_state(), "plies": run._plies, "done": run._done, "seeds": run.seeds,
            "rows": int(eng.play_rows.item()), "unread": int(eng.play_unread.item()),
            "hits": int(eng.table_stats[0].item())}


def _same_games(a, b):
    for k in range(a["moves"].shape[0]):
        assert torch.equal(a["moves"][k], b["moves"][k]), f"ply {k}: moves differ"
        assert torch.equal(a["p"][k].view(torch.int64), b["p"][k].view(torch.int64)), \
            f"ply {k}: policy vectors differ"
    for x, y in zip(a["state"], b["state"]):     # boards, status
        assert torch.equal(x, y)
    for k in ("black", "white", "side", "plies", "done", "seeds"):
        assert torch.equal(a[k], b[k]), k


def _root_moves(oracle, r, board):
    """Legal moves of every recorded root, [plies, G] (the oracle's move generator)."""
    b = r["black"].cpu().numpy().view(np.uint64)
    w = r["white"].cpu().numpy().view(np.uint64)
    s = r["side"].cpu().numpy()
    out = np.zeros(b.shape, np.int64)
    for i in np.ndindex(*b.shape):
        P, Q = (b[i], w[i]) if s[i] == 1 else (w[i], b[i])
        out[i] = bin(oracle.legal(int(P), int(Q), board)).count("1")
    return out


def _row_bound(L, S):
    """At most one row per batch and none for the deferred last one: E - 1 rows per search, and
    the root's row alone where the rule holds (L >= E - 1)."""
    E = -(-S // 64)
    return int(np.where(L >= E - 1, 1, E - 1).sum())


def _pair(oracle, key, table=None):
    """The run with the rule and the run that evaluates every row, at PARENT_ROWS' key: the same
    games, fewer rows with the rule, the parent's rows without it."""
    board, blocks, filters, G, S, plies, gpw = key
    import rvz
    ev = rvz.LeafEvaluator(_net(board, blocks, filters))
    lazy = _play(ev, G, S, plies, True, gpw, table=table)
    full = _play(ev, G, S, plies, False, gpw, table=table)
    _same_games(lazy, full)
    L = _root_moves(oracle, lazy, board)
    print(f"{key}: rows {lazy['rows']} with the rule ({lazy['unread']} left unread), "
          f"{full['rows']} without; roots with L >= E - 1: {int((L >= -(-S // 64) - 1).sum())} "
          f"of {L.size}")
    assert full["unread"] == 0
    assert full["rows"] == PARENT_ROWS[key], (full["rows"], PARENT_ROWS[key])
    assert lazy["rows"] < full["rows"]
    assert 0 < lazy["rows"] <= _row_bound(L, S)
    return ev, lazy, full, L


def test_c2_shape_same_games_fewer_rows_and_the_oracle(oracle):
    """96 8x8 games x 800 simulations (E = 13), a 1x64 net, memo on, groups of 6, 40 plies: the
    window in which roots with 12 or more legal moves occur. With and without the rule: every
    ply's moves and f64 policy vectors bitwise equal, final boards, status, counters and seeds
    equal, fewer rows with it. 12 sampled games against the oracle in every ply; the oracle's own
    roots include some with >= 12 legal moves."""
    key = (8, 1, 64, 96, 800, 40, -6)
    ev, lazy, _, _ = _pair(oracle, key)
    G, S, plies = key[3], key[4], key[5]
    sample = np.linspace(0, G - 1, 12).astype(int)
    orc = OracleGames(oracle, [42 + int(g) for g in sample], S)
    moves, p = lazy["moves"].cpu().numpy(), lazy["p"].cpu().numpy()
    compared = wide = 0
    for ply in range(plies):
        live = np.array([not g.over for g in orc.games])   # an ended game restarted (autoreset)
        nmoves = np.array([bin(oracle.legal(*((g.black, g.white) if g.side == 1
                                              else (g.white, g.black)), 8)).count("1")
                           for g in orc.games])
        _, oi, op, _ = orc.ply(ev)
        s = sample[live]
        assert np.array_equal(oi[live], moves[ply][s]), (ply, oi[live], moves[ply][s])
        assert np.array_equal(op[live].view(np.int64), p[ply][s].view(np.int64)), ply
        compared += int(live.sum())
        wide += int((nmoves[live] >= 12).sum())
    print(f"oracle: {compared} plies compared, {wide} with >= 12 legal moves at the root")
    assert compared >= 12 * plies * 0.9
    assert wide >= 1


def test_rule_fires_in_every_search_of_the_opening(oracle):
    """64 games x 200 simulations (E = 4: the rule needs L >= 3), the first 3 plies: every root
    there has at least 3 legal moves (4, 3, then >= 4; the fourth ply has roots with 2, so the
    window ends before it), so every search evaluates its root's row at most."""
    key = (8, 1, 64, 64, 200, 3, -4)
    _, lazy, _, L = _pair(oracle, key)
    assert L.min() >= 3, L.min(0)
    assert lazy["rows"] <= key[3] * key[5]
    assert lazy["unread"] > 0


def test_6x6_three_boards_per_pass(oracle):
    """6x6 at 400 simulations (E = 7: L >= 6), 72 games, three packed boards per trunk pass."""
    _pair(oracle, (6, 1, 64, 72, 400, 24, -6))


def test_8x8_two_blocks_of_128_one_board_per_pass(oracle):
    """8x8 with a 2x128 net, 32 games, one board per pass, the pass gate at its default."""
    _pair(oracle, (8, 2, 128, 32, 800, 30, -4))


def test_table_hits_still_account_for_every_row_not_evaluated(oracle):
    """With the cross-game table on (256 games x 800 simulations x 20 plies): an unread row takes
    no lookup, hit or insert, so every hit is still exactly one row not evaluated."""
    import rvz
    ev = rvz.LeafEvaluator(_net(8, 1, 64))
    G, S, plies = 256, 800, 20
    with_t = _play(ev, G, S, plies, True, -6, table=(1 << 16, 14))
    plain = _play(ev, G, S, plies, True, -6)
    _same_games(with_t, plain)
    assert with_t["hits"] > 0
    assert with_t["rows"] + with_t["hits"] == plain["rows"], \
        (with_t["rows"], with_t["hits"], plain["rows"])
    assert with_t["unread"] == plain["unread"]
