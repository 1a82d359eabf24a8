"""rvz_alphabeta (csrc/rvz_alphabeta.hip), the depth-limited heuristic search, on the GPU against
the host reference of tests/alphabeta_ref.py: the unpruned negamax over the CPU oracle's legal /
make_move, i.e. the definition in include/rvz.h with the reference's rule quirks. Every score is
an integer and every comparison is exact."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import alphabeta_ref as A
import solve_ref as R

pytestmark = pytest.mark.gpu

BIG = 2 ** 40        # a node limit no row of these tests reaches
GARBAGE = 77


def gpu_ab(games, bs, depth, wt, node_limit=BIG, arrays=None):
    import rvz
    b, w, st = arrays if arrays is not None else R.to_device(games)
    s, m, k = rvz.alphabeta(b, w, st, bs, depth, list(wt), node_limit)
    assert s.dtype == torch.int32 and m.dtype == torch.int32 and k.dtype == torch.int64
    assert s.is_cuda and m.is_cuda and k.is_cuda
    return s.cpu().numpy(), m.cpu().numpy(), k.cpu().numpy()


def check_rows(tag, games, got, host):
    """host: per row (score, move in the kernel's encoding, negamax's node count or None)."""
    score, move, nodes = got
    for i, (g, (hs, hm, hk)) in enumerate(zip(games, host)):
        assert (score[i], move[i]) == (hs, hm), (tag, i, g.astuple(), score[i], move[i], hs, hm)
        if hk is None:
            assert nodes[i] >= 1, (tag, i)
        elif hm == -5:
            assert nodes[i] == 0, (tag, i)
        else:
            assert 1 <= nodes[i] <= hk, (tag, i, g.astuple(), nodes[i], hk)


@pytest.mark.parametrize("bs", [8, 6])
@pytest.mark.parametrize("table", ["default", "asymmetric"])
def test_depths_1_to_3_against_negamax(bs, table):
    """64 opening and midgame playouts and the late positions; the pruned search visits no more
    positions than the unpruned definition."""
    games = A.playouts(bs) + A.late(bs)
    wt = A.TABLES[table](bs)
    arrays = R.to_device(games)
    for depth in (1, 2, 3):
        check_rows((bs, table, depth), games, gpu_ab(games, bs, depth, wt, arrays=arrays),
                   A.host_negamax(bs, table, depth))
    # depth 1 prunes nothing: every root child is a frontier node
    assert np.array_equal(gpu_ab(games, bs, 1, wt, arrays=arrays)[2],
                          [h[2] for h in A.host_negamax(bs, table, 1)])


# the host's alpha-beta takes about 0.3 s per 8x8 midgame position at depth 5: 16 rows a case
@pytest.mark.parametrize("bs,part,parts", [(8, 0, 4), (8, 1, 4), (8, 2, 4), (8, 3, 4), (6, 0, 1)])
@pytest.mark.parametrize("table", ["default", "asymmetric"])
def test_depth_5_against_host_alphabeta(bs, part, parts, table):
    games = A.playouts(bs)[part::parts] + (A.late(bs) if part == 0 else [])
    wt = A.TABLES[table](bs)
    host = []
    for g in games:
        hs, hm = A.alphabeta(g, 5, wt, bs)
        host.append((hs, A.expected_move(g, hm, bs), None))
    check_rows((bs, table, 5), games, gpu_ab(games, bs, 5, wt), host)


@pytest.mark.parametrize("bs", [8, 6])
@pytest.mark.parametrize("table", ["default", "asymmetric"])
def test_max_depth_reaches_the_end_of_the_game(bs, table):
    """RVZ_AB_MAX_DEPTH on positions with at most 9 empties: every line ends in T."""
    games = A.late(bs)
    assert all(R.empties(g, bs) <= 9 for g in games)
    wt = A.TABLES[table](bs)
    host = []
    for g in games:
        hs, hm = A.alphabeta(g, A.MAX_DEPTH, wt, bs)
        assert hs == 0 or abs(hs) > A.WIN
        host.append((hs, A.expected_move(g, hm, bs), None))
    check_rows((bs, table, A.MAX_DEPTH), games, gpu_ab(games, bs, A.MAX_DEPTH, wt), host)


def _expect(g, depth, wt, bs):
    """What the kernel reports for any row, malformed ones included."""
    nsq = bs * bs
    if (g.black & g.white) or (g.black | g.white) >> nsq or g.side not in (1, 2):
        return 0, -5, 0
    hs, hm, hk = A.negamax(g, depth, wt, bs)
    return hs, A.expected_move(g, hm, bs), hk


@pytest.mark.parametrize("bs,seeds", [(8, (12, 25)), (6, (9, 15))])
def test_root_cases_and_synthetic_rows(bs, seeds):
    """Positions no playout reaches: pass roots with passed 0 and 1 (explicit passes, passes that
    end the game), finished games (-2), malformed rows (-5), one-colour, empty and full boards,
    and every synthetic row, both sides to move. A pass costs no depth; there is no -3."""
    nsq = bs * bs
    full = (1 << nsq) - 1
    cases = R.RootCases(bs, seeds)
    extra = [R.O.Game(0, 0, 1, 0, -1, 0), R.O.Game(0, 0, 2, 0, -1, 1),
             R.O.Game(full, 0, 1, 0, -1, 0), R.O.Game(0, full, 1, 0, -1, 0),
             R.O.Game(full & 0x5555555555555555, full & 0xAAAAAAAAAAAAAAAA, 2, 0, -1, 0),
             R.O.Game(full ^ 1, 0, 2, 0, -1, 0), R.O.Game(1, 0, 1, 0, -1, 0)]
    games = cases.mixed + extra + R.synthetic_rows(bs)
    R.check_synthetic_kinds(bs)
    wt = A.asymmetric_table(bs)
    for depth in (1, 2):
        got = gpu_ab(games, bs, depth, wt)
        host = [_expect(g, depth, wt, bs) for g in games]
        check_rows((bs, depth), games, got, host)
        codes = {int(m) for m in got[1] if m < 0}
        assert codes == {-2, -5}, codes
        for i, j in cases.where.items():
            want = cases.expect[j][1]
            if want in (-2, -5, nsq):                  # the solver's -3 row is an ordinary row
                assert got[1][i] == want, (i, j)
            if want == -2:
                assert got[2][i] == 1 and got[0][i] == A.terminal(games[i])
            if want == -5:
                assert got[2][i] == 0 and got[0][i] == 0
        # a pass root's count: the root, the position after the pass, and that one's search
        assert sum(1 for m in got[1] if m == nsq) >= 10
    # at a depth that reaches the end the synthetic rows' values are the solver's, pushed by WIN
    syn = R.synthetic_rows(bs)
    score, move, _ = gpu_ab(syn, bs, R.SYNTHETIC_MAX_EMPTIES, wt)
    for i, (g, (hs, hm, _)) in enumerate(zip(syn, R.synthetic_solved(bs))):
        want = 0 if hs == 0 else (A.WIN + hs if hs > 0 else hs - A.WIN)
        assert (score[i], move[i]) == (want, R.expected_move(g, hm, bs)), (bs, i, g.astuple())


def _auto_pass_pairs(seed, bs):
    """(parent, child) for every auto-pass of a seeded playout: the child is the position right
    after the move that left the other side without a reply."""
    rng = random.Random(seed)
    g = R.O.new_game(bs)
    out = []
    while not g.over:
        parent, mover = g.copy(), g.side
        sq = rng.choice(list(R.squares(R.mover_mask(g, bs))))
        assert R.O.make_move(g, sq, bs)
        if not g.over and g.side == mover:
            out.append((parent, g.copy()))
    return out


@pytest.mark.parametrize("bs", [8, 6])
def test_auto_pass_costs_no_depth(bs):
    """Positions right after an auto-pass and their parents at depth 2: below the parent the
    passing side's move is skipped at no depth, so the mover's second move is still searched."""
    games = []
    for seed in range(120):
        last = R.last_auto_pass(seed, 0, bs)
        pairs = _auto_pass_pairs(seed, bs)
        assert (last is None) == (not pairs)
        if pairs:
            assert pairs[-1][1].astuple() == last.astuple()
            games += [g for pair in pairs for g in pair]
    assert len(games) >= 20
    wt = A.default_table(bs)
    host = [_expect(g, 2, wt, bs) for g in games]
    # the test has teeth: charging the pass a ply changes at least one of these values
    changed = 0
    for g, (hs, _, _) in zip(games[0::2], host[0::2]):
        best = -A.INF
        for sq in R.squares(R.mover_mask(g, bs)):
            c = g.copy()
            R.O.make_move(c, sq, bs)
            d = 0 if (c.side == g.side and not c.over) else 1
            v = A.negamax(c, d, wt, bs)[0]
            best = max(best, v if c.side == g.side else -v)
        changed += best != hs
    assert changed >= 1
    check_rows((bs, "auto-pass"), games, gpu_ab(games, bs, 2, wt), host)


def test_batch_shape_independence():
    """A row's three outputs do not depend on the batch it is in: 40 rows at n = 1, 63, 64, 65
    and 129, repeated and permuted; and a batch larger than the launch's lane count equals its
    64-row period."""
    games = A.playouts(8)[:28] + A.late(8)
    assert len(games) == 40
    wt = A.default_table(8)
    base = gpu_ab(games, 8, 3, wt)
    rng = np.random.RandomState(5)
    for n in (1, 63, 64, 65, 129):
        idx = np.concatenate([rng.permutation(40) for _ in range(-(-n // 40))])[:n]
        got = gpu_ab([games[i] for i in idx], 8, 3, wt)
        for a, b in zip(got, base):
            assert np.array_equal(a, b[idx]), n
    # the launch: min(ceil(n / 128), 4 workgroups per CU) workgroups of 128 lanes
    period = A.playouts(8)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lanes = cus * 4 * 128
    reps = lanes // 64 + 3
    arrays = tuple(torch.from_numpy(np.tile(a, (reps,) + (1,) * (a.ndim - 1))).cuda()
                   for a in R.to_arrays(period))
    assert arrays[0].numel() == 64 * reps > lanes
    one = gpu_ab(period, 8, 2, wt)
    big = gpu_ab(None, 8, 2, wt, arrays=arrays)
    for a, b in zip(big, one):
        assert np.array_equal(a.reshape(reps, 64), np.broadcast_to(b, (reps, 64)))


def test_node_limit():
    games = A.playouts(8)[:32] + [R.position(3, 0, 8)[0]]
    wt = A.default_table(8)
    score, move, nodes = gpu_ab(games, 8, 3, wt)
    again = gpu_ab(games, 8, 3, wt, node_limit=int(nodes.max()))
    for a, b in zip(again, (score, move, nodes)):
        assert np.array_equal(a, b)
    # a limit equal to a row's own count solves it, one less abandons it; neighbours keep theirs
    i = int(np.argsort(nodes)[len(nodes) // 2])
    limit = int(nodes[i])
    assert limit > 2
    s1, m1, k1 = gpu_ab(games, 8, 3, wt, node_limit=limit)
    assert (s1[i], m1[i], k1[i]) == (score[i], move[i], nodes[i])
    s2, m2, k2 = gpu_ab(games, 8, 3, wt, node_limit=limit - 1)
    assert (s2[i], m2[i], k2[i]) == (0, -4, limit - 1)
    for got, lim in (((s1, m1, k1), limit), ((s2, m2, k2), limit - 1)):
        for j in range(len(games)):
            if nodes[j] <= lim:
                assert (got[0][j], got[1][j], got[2][j]) == (score[j], move[j], nodes[j]), j
            else:
                assert (got[0][j], got[1][j], got[2][j]) == (0, -4, lim), j
    assert (m2 == -4).sum() >= 2 and (m2 >= 0).sum() >= 2
    # one position per row: only a root that is over has an answer
    s3, m3, k3 = gpu_ab(games, 8, 3, wt, node_limit=1)
    assert list(m3[:32]) == [-4] * 32 and not s3[:32].any() and list(k3[:32]) == [1] * 32
    assert (s3[32], m3[32], k3[32]) == (score[32], -2, 1) and move[32] == -2


def _raw(lib, arrays, bs, depth, wt_host, out, stream):
    b, w, st = arrays
    rc = lib.rvz_alphabeta(bs, b.numel(), b.data_ptr(), w.data_ptr(), st.data_ptr(), depth,
                           C.cast(wt_host, C.c_void_p), BIG, out[0].data_ptr(),
                           out[1].data_ptr(), out[2].data_ptr() if out[2] is not None else None,
                           stream)
    assert rc == 0, rc


def test_graph_capture_keeps_its_weights():
    """One captured call replayed twice gives the eager outputs; the host table is read at the
    call, so overwriting it after the capture changes nothing."""
    import rvz
    lib = rvz.load()
    games = A.playouts(8)
    arrays = R.to_device(games)
    wt, other = A.asymmetric_table(8), A.default_table(8)
    eager = [t.clone() for t in rvz.alphabeta(*arrays, 8, 3, list(wt), BIG)]      # warm
    torch.cuda.synchronize()
    out = tuple(torch.empty_like(t) for t in eager)
    host = (C.c_int32 * 65)(*wt)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _raw(lib, arrays, 8, 3, host, out, torch.cuda.current_stream().cuda_stream)
    host[:] = list(other)
    for _ in range(2):
        for t in out:
            t.fill_(GARBAGE)
        graph.replay()
        torch.cuda.synchronize()
        for a, e in zip(out, eager):
            assert torch.equal(a, e)
    # out_nodes is nullable
    for t in out:
        t.fill_(GARBAGE)
    _raw(lib, arrays, 8, 3, host, (out[0], out[1], None), None)
    torch.cuda.synchronize()
    want = rvz.alphabeta(*arrays, 8, 3, list(other), BIG)
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
    assert bool((out[2] == GARBAGE).all())
    assert not torch.equal(want[0], eager[0])


def test_solver_and_alphabeta_in_flight_together():
    """rvz.solve, rvz.solve_moves and rvz.alphabeta issued back to back on three streams with
    nothing between them give, node counts included, what each gives alone: both translation
    units take their row counters from csrc/rvz_negamax.hip.h, each a copy of its own. More than
    128 rows: lanes take further rows and more than one workgroup runs. 32 rounds, all queued
    before anything is waited for: a round takes two of the solver's 32 counter slots and one of
    alpha-beta's, so the difference of the two units' slot indices passes through every residue
    and, were the array one, some round's calls would hold the same counter while the streams'
    queues keep the three kernels running side by side."""
    import rvz
    games = [R.position(s, 8, 8)[0] for s in range(300)] + R.RootCases(8, (12, 25)).mixed
    arrays = R.to_device(games)
    wt = list(A.default_table(8))
    calls = [lambda: rvz.solve(*arrays, 8, 8, BIG),
             lambda: rvz.solve_moves(*arrays, 8, 8, BIG),
             lambda: rvz.alphabeta(*arrays, 8, 3, wt, BIG)]
    alone = []
    for call in calls:
        alone.append(call())
        torch.cuda.synchronize()
    assert int((alone[0][2] > 1).sum()) > 256 and int((alone[2][2] > 1).sum()) > 256
    streams = [torch.cuda.Stream() for _ in calls]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    rounds = []
    for _ in range(32):
        together = []
        for s, call in zip(streams, calls):
            with torch.cuda.stream(s):
                together.append(call())
        rounds.append(together)
    for s in streams:
        s.synchronize()
    for i, together in enumerate(rounds):
        for name, got, want in zip(("solve", "solve_moves", "alphabeta"), together, alone):
            for a, b in zip(got, want):
                assert torch.equal(a, b), (i, name)


def test_two_streams_two_tables_and_the_engine():
    import rvz
    games = A.playouts(8)
    arrays = R.to_device(games)
    tables = [A.default_table(8), A.asymmetric_table(8)]
    want = [rvz.alphabeta(*arrays, 8, 4, list(t), BIG) for t in tables]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for s, t in zip(streams, tables):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got.append(rvz.alphabeta(*arrays, 8, 4, list(t), BIG))
    for s in streams:
        s.synchronize()
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert torch.equal(a, b)
    assert not torch.equal(want[0][0], want[1][0])
    # the engine's own games
    eng = rvz.Engine(64, num_simulations=16, batch_size=16, device="cuda:0")
    eng.set_state(*arrays)
    before = [t.clone() for t in eng.get_state()]
    for a, b in zip(eng.alphabeta(4, node_limit=BIG), want[0]):
        assert torch.equal(a, b)
    for a, b in zip(eng.alphabeta(4, list(tables[1]), BIG), want[1]):
        assert torch.equal(a, b)
    for a, b in zip(before, eng.get_state()):
        assert torch.equal(a, b)
    eng.check()
