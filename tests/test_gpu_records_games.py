"""rvz_records_games on the device against the Python restatement (tests/records_games_ref.py),
every comparison exact: synthetic windows at the sizes that cross the wave, workgroup and scan
boundaries, the edge cases of the walk, the carry equivalence, determinism and graph replay, the
entry point's refusals; then the engine's own autoreset records through
SelfPlayRunner(carry_plies=...) and one SelfPlayTrainer(continuous_plies=...) iteration pair."""
import math

import numpy as np
import pytest
import torch

import records_games_ref as RG
from test_records_games import carried_rows, carry_case, check_entry_point_refusals

pytestmark = pytest.mark.gpu

ROW_KEYS = ("mover", "opponent", "policy", "value", "src")


def _call(bs, win, emit_from=0):
    import rvz
    out = rvz.records_games(*RG.tensors(*win, device="cuda"), bs, emit_from=emit_from, state=True)
    torch.cuda.synchronize()
    return out


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(out, ref, what=""):
    """m, the rows [0, m) of every output, state and stats equal the reference's."""
    m = int(out["m"])
    assert m == ref["m"], (what, m, ref["m"])
    assert out["stats"].tolist() == ref["stats"].tolist(), what
    assert np.array_equal(out["state"].cpu().numpy(), ref["state"]), what
    for k in ROW_KEYS:
        got = out[k][:m].cpu().numpy()
        want = ref[k].view(np.int64) if ref[k].dtype == np.uint64 else ref[k]
        assert got.dtype == want.dtype and got.shape == want.shape, (what, k)
        assert got.tobytes() == want.tobytes(), (what, k)
    return m


@pytest.mark.parametrize("bs,P,G", [(6, 40, 1), (6, 40, 63), (6, 40, 64), (6, 40, 65),
                                    (6, 40, 130), (8, 70, 65), (6, 40, 1025), (6, 40, 2049)])
def test_synthetic_windows(oracle, bs, P, G):
    """Games restarting right after they end, slots opening inside a game, gaps, pass-index
    records: emit_from at 0, in the middle and at P (nothing emitted)."""
    win = RG.edge_window(oracle, bs, P, G, 100 * bs + G)
    for emit_from in (0, P // 2 + 3, P):
        ref = RG.games(oracle, bs, *win, emit_from)
        m = _same(_call(bs, win, emit_from), ref, f"emit_from={emit_from}")
        assert (m == 0) == (emit_from == P) and ref["stats"][2] > 0
    assert ref["stats"][6] > 0 and not ref["stats"][0] and not ref["stats"][1]


@pytest.mark.parametrize("bs", [6, 8])
def test_game_ending_at_the_emit_boundary(oracle, bs):
    """A game whose last record is at ply e: emitted with emit_from = e, state 2 with e + 1."""
    P = bs * bs + 6
    win = RG.window(oracle, bs, P, 5, 3)
    black = win[0]
    # slot 2's second game opens with the start position again: its first game ends a ply before
    end = next(p for p in range(1, P) if black[p, 2] == black[0, 2]) - 1
    assert 8 <= end < bs * bs - 4
    for emit_from, state in ((end, 1), (end + 1, 2)):
        ref = RG.games(oracle, bs, *win, emit_from)
        assert (ref["state"][:end + 1, 2] == state).all()
        _same(_call(bs, win, emit_from), ref, f"emit_from={emit_from}")


def _malformed_window(oracle, bs):
    """One mutation per slot, each at a ply inside the slot's first game."""
    nsq = bs * bs
    black, white, side, idx, p = RG.window(oracle, bs, nsq, 8, 11)
    start = oracle.new_game(bs)
    b = int(black[9, 0])
    white[9, 0] = np.uint64(int(white[9, 0]) | (b & -b))           # a disc of both colours
    if bs == 6:
        black[9, 1] |= np.uint64(1 << 40)                          # a bit off the board
    else:
        side[9, 1] = 0
    side[9, 2] = 3
    idx[9, 3] = nsq + 1
    occupied = int(black[9, 4] | white[9, 4])
    idx[9, 4] = next(s for s in range(nsq) if occupied >> s & 1)   # an occupied square
    # a broken chain: slot 5's record 9 becomes the start position with its first move
    black[9, 5], white[9, 5], side[9, 5], idx[9, 5] = black[0, 5], white[0, 5], 1, idx[0, 5]
    assert (int(black[0, 5]), int(white[0, 5])) == (int(start.black), int(start.white))
    idx[9, 6] = nsq                                                # a pass with moves to play
    return black, white, side, idx, p


@pytest.mark.parametrize("bs", [6, 8])
def test_malformed_records_and_broken_chains(oracle, bs):
    win = _malformed_window(oracle, bs)
    ref = RG.games(oracle, bs, *win, 0)
    st = ref["state"]
    for g in (0, 1, 2, 3, 4, 6):
        assert st[9, g] == -5 and (st[:9, g] == 3).all(), g       # the segment is abandoned
        assert st[10, g] in (0, 1)                                 # a headless one follows
    assert (st[:9, 5] == 3).all() and st[9, 5] == 3 and st[10, 5] in (0, 1)
    assert (st[:, 7] != 3).all() and ref["stats"][4] == 6 and ref["stats"][3] == 6 * 9 + 10
    assert ref["stats"][5] >= 1
    _same(_call(bs, win), ref)


def test_window_without_a_finished_game_writes_no_row(oracle):
    """m = 0: the row outputs keep their bytes; with rows, those at and above m keep theirs."""
    import rvz
    lib = rvz.load()
    for P, want_rows in ((12, False), (40, True)):
        win = RG.window(oracle, 6, P, 70, 2)
        ref = RG.games(oracle, 6, *win, 0)
        assert (ref["m"] > 0) == want_rows
        b, w, s, i, p = RG.tensors(*win, device="cuda")
        n = P * 70
        outs = [torch.full((n,), -7, dtype=torch.int64, device="cuda") for _ in range(2)] + \
            [torch.full((n, 37), -7.0, device="cuda"), torch.full((n,), -7.0, device="cuda"),
             torch.full((n,), -7, dtype=torch.int32, device="cuda")]
        m = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        stats = torch.full((8,), -7, dtype=torch.int64, device="cuda")
        scratch = torch.empty(lib.rvz_records_scratch_size(P, 70), dtype=torch.uint8,
                              device="cuda").fill_(0xA5)               # no preparation needed
        rc = lib.rvz_records_games(6, P, 70, b.data_ptr(), w.data_ptr(), s.data_ptr(),
                                   i.data_ptr(), p.data_ptr(), 0, scratch.data_ptr(),
                                   m.data_ptr(), *(t.data_ptr() for t in outs), None,
                                   stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0 and int(m) == ref["m"] and stats.tolist() == ref["stats"].tolist()
        for t, k in zip(outs, ROW_KEYS):
            assert bool((t[ref["m"]:] == -7).all()), k
            want = ref[k].view(np.int64) if ref[k].dtype == np.uint64 else ref[k]
            assert t[:ref["m"]].cpu().numpy().tobytes() == want.tobytes(), k


def test_carry_equivalence(oracle):
    win, C, K, first, second, whole = carry_case(oracle)
    G = win[3].shape[1]
    cut = lambda lo, hi: tuple(a[lo:hi] for a in win)
    a, b, c = _call(6, cut(0, C + K), C), _call(6, cut(K, C + 2 * K), C), _call(6, win, C)
    _same(a, first), _same(b, second), _same(c, whole)
    ma, mb, mc = int(a["m"]), int(b["m"]), int(c["m"])
    src_a, src_b = a["src"][:ma].tolist(), b["src"][:mb].tolist()
    got = carried_rows({"src": src_a}, {"src": src_b}, K, G)
    assert got == [divmod(int(s), G) for s in c["src"][:mc].tolist()] and ma + mb == mc > 0
    # and the rows themselves: the two windows' rows, put slot-major, are the whole window's
    rows = [divmod(s, G) for s in src_a] + [(s // G + K, s % G) for s in src_b]
    perm = sorted(range(mc), key=lambda j: (rows[j][1], rows[j][0]))
    for k in ("mover", "opponent", "policy", "value"):
        both = torch.cat([a[k][:ma], b[k][:mb]])
        assert torch.equal(_bits(both[perm]), _bits(c[k][:mc])), k


def test_determinism_and_graph_replay(oracle):
    import rvz
    win = RG.edge_window(oracle, 6, 40, 130, 9)
    args = RG.tensors(*win, device="cuda")
    one = rvz.records_games(*args, 6, emit_from=4, state=True)
    two = rvz.records_games(*args, 6, emit_from=4, state=True)
    torch.cuda.synchronize()
    m = int(one["m"])
    assert m > 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = rvz.records_games(*args, 6, emit_from=4, state=True)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for other in (two, held):
            assert int(other["m"]) == m
            assert torch.equal(other["stats"], one["stats"])
            assert torch.equal(other["state"], one["state"])
            for k in ROW_KEYS:
                assert torch.equal(_bits(other[k][:m]), _bits(one[k][:m])), k


def test_entry_point_refusals_and_scratch_size():
    import rvz
    check_entry_point_refusals(rvz.load())


# ---------------------------------------------------------------- the engine's own records
# 64 simulations in batches of 16: a search of one batch (64 at batch 64) visits no child of its
# root, its act has no move to play and the game stands still (records_games calls that malformed)
G6, S6, B6 = 16, 64, 16


def _net():
    import rvz
    torch.manual_seed(0)
    return rvz.AlphaZeroNetwork(6, 1, 64).cuda().eval()


def _runner_window(run):
    return tuple(t.cpu().numpy() for t in (run.rec_black.view(torch.int64), run.rec_white,
                                           run.rec_side, run.rec_idx, run.rec_p))


def test_runner_with_carry_against_the_reference(oracle):
    """6x6, 16 games, 64 simulations: two launches of 24 plies with autoreset behind a carry of
    32, roll() between them; records_games on the runner's tensors equals the reference, nothing
    is abandoned, malformed or headless, and the emitted games are the growth of games_done."""
    import rvz
    C, K = 32, 24
    eng = rvz.Engine(G6, S6, B6, board_size=6, compact_leaves=True, memo=True)
    run = rvz.SelfPlayRunner(eng, rvz.LeafEvaluator(_net()), record=True, max_plies=K, fused=True,
                             autoreset=True, carry_plies=C, skip_last_eval=True)
    run.start()
    assert run.ply_index == C and run.rec_idx.shape == (C + K, G6)
    assert bool((run.rec_idx == -2).all())
    emitted, rows = 0, 0
    for launch in range(2):
        run.play_record(K)
        run.check()
        assert run.ply_index == C + K
        out = rvz.records_games(run.rec_black, run.rec_white, run.rec_side, run.rec_idx,
                                run.rec_p, 6, emit_from=C, state=True)
        b, w, s, i, p = _runner_window(run)
        ref = RG.games(oracle, 6, b.view(np.uint64), w.view(np.uint64), s, i, p, C)
        rows += _same(out, ref, f"launch {launch}")
        stats = out["stats"].tolist()
        assert stats[3] == stats[4] == stats[5] == 0, stats
        assert stats[2] > 0                                        # games go on into the next
        emitted += stats[1]
        before = [t.clone() for t in (run.rec_black, run.rec_white, run.rec_side, run.rec_idx,
                                      run.rec_p)]
        run.roll()
        assert run.ply_index == C and bool((run.rec_idx[C:] == -2).all())
        for t, old in zip((run.rec_black, run.rec_white, run.rec_side, run.rec_idx, run.rec_p),
                          before):
            assert torch.equal(t[:C], old[K:])
    assert emitted == int(run.games_done.item()) > 0 and rows > 0


def test_trainer_continuous_iterations():
    """Two iterations of 24 plies: the buffer grows by the emitted games' rows, the counters
    agree with each other, the loss is finite."""
    import rvz
    from rvz.pipeline import SelfPlayTrainer
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(6, 1, 64).cuda()
    spt = SelfPlayTrainer(net, G6, num_simulations=S6, batch_size=B6, seed=5, train_steps=2,
                          train_batch=32, continuous_plies=24, replay_iterations=2, policy_target="full")
    held, games, steps = 0, 0, 0
    for it in range(2):
        out = spt.run_iteration()
        assert out["records_abandoned"] == 0 and out["records_headless_games"] == 0
        assert out["board_steps"] == 24 * G6                        # no slot idles
        assert out["replay_rows"] == held + out["samples"]
        held, games = out["replay_rows"], games + out["games_emitted"]
        assert (out["samples"] > 0) == (out["games_emitted"] > 0)
        # every committed ply is emitted or still open
        steps += out["board_steps"]
        assert held + out["records_open"] == steps
        assert math.isfinite(out["train/loss"])
    assert games == int(spt.runner.games_done.item()) > 0 and out["steps"] == 2
    assert out["train/loss"] > 0
