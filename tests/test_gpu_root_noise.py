"""Dirichlet noise at the search roots (rvz_search_root_noise / Engine.root_noise): the pull-style
search and the fused launch against the literal oracle fed rows mixed in NumPy (noise_oracle.py),
fused against pull-style over every setting that must not matter, resets, off-is-off, the
SelfPlay opt-in and graph replay.

Priors only influence visits once every root child has been visited (tests/test_gpu_dropin.py
explains why S <= 200 at B = 64 sees none), so the searches here use num_simulations = 64 at
batch_size = 8: the root's batch, at most four batches for the opening's four children, then
three that UCB decides. Every search test first asserts that this configuration sees the priors:
without noise the 64 identical start positions give one ply-0 visit vector, with noise at least
two."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S, B = 64, 8
ALPHA, EPS = 0.3, 0.25


@functools.lru_cache(maxsize=None)
def _net(board=8, blocks=2, filters=64, seed=0):
    import rvz
    torch.manual_seed(seed)
    return rvz.AlphaZeroNetwork(board, blocks, filters).cuda().eval()


@functools.lru_cache(maxsize=None)
def _ply0_distinct(board, blocks, filters):
    """(distinct ply-0 visit vectors of 64 games without noise, with noise)."""
    import rvz
    net = _net(board, blocks, filters)
    out = []
    for noise in (False, True):
        eng = rvz.Engine(64, S, B, board_size=board)
        if noise:
            eng.root_noise(ALPHA, EPS)
        eng.reset(range(100, 164))
        eng.search(rvz.LeafEvaluator(net))
        out.append(len({tuple(r) for r in eng.visits().cpu().numpy().tolist()}))
        eng.check()
    return tuple(out)


def _assert_sees_priors(board=8, blocks=2, filters=64):
    clean, noisy = _ply0_distinct(board, blocks, filters)
    assert clean == 1, f"{clean} distinct ply-0 visit vectors without noise"
    assert noisy >= 2, "the noise does not reach the visits at these sizes: raise S"


# ---------------------------------------------------------------- against the oracle
def _oracle(oracle, net, seeds, plies, softmax=None):
    import rvz
    from noise_oracle import NoisyOracleGames
    orc = NoisyOracleGames(oracle, seeds, S, B, ALPHA, EPS, bs=net.board_size, softmax=softmax)
    ev = rvz.LeafEvaluator(net)
    return [orc.ply(ev) for _ in range(plies)]


@functools.lru_cache(maxsize=None)
def _oracle_games():
    from oracle import oracle as O
    O.lib()
    return _oracle(O, _net(), tuple(range(1000, 1064)), 6)


def _check_ply(k, want, vis, idx, p):
    wv, wi, wp = want
    assert np.array_equal(vis, wv), f"ply {k}: visits differ from the oracle"
    assert np.array_equal(idx, wi), f"ply {k}: moves differ from the oracle"
    assert np.array_equal(p.view(np.int64), wp.view(np.int64)), f"ply {k}: p differs"


@pytest.mark.parametrize("logits", [True, False], ids=["logits", "probs"])
@pytest.mark.parametrize("compact", [False, True], ids=["dense", "compact"])
@pytest.mark.parametrize("memo", [False, True], ids=["nomemo", "memo"])
def test_pull_style_against_oracle(memo, compact, logits):
    """64 games, 6 plies: every ply's visits, f64 p (bitwise) and move equal the oracle's."""
    import rvz
    _assert_sees_priors()
    net = _net()
    want = _oracle_games()
    eng = rvz.Engine(64, S, B, compact_leaves=compact, memo=memo)
    eng.root_noise(ALPHA, EPS)
    eng.reset(range(1000, 1064))
    ev = rvz.LeafEvaluator(net)
    for k in range(6):
        if logits:
            eng.search(ev)
        else:                       # the rows softmaxed outside, submitted as probabilities
            eng.search_begin()
            while eng.search_step():
                if compact:
                    lg, val = ev(eng.leaf_x, n_live=eng.live_count())
                else:
                    lg, val = ev(eng.leaf_x)
                eng.search_submit(rvz.policy_softmax(lg), val.float().contiguous(), False)
        vis = eng.visits().cpu().numpy().copy()
        idx, p = eng.act(1.0, apply=True)
        _check_ply(k, want[k], vis, idx.cpu().numpy(), p.cpu().numpy())
    assert len({tuple(w[1]) for w in want}) > 1
    eng.check()


@pytest.mark.parametrize("memo", [False, True], ids=["nomemo", "memo"])
def test_fused_against_oracle(memo):
    """The same through Engine.play, one launch per ply, the cross-game table on (a root expanded
    from a table hit is mixed after the softmax of the stored, clean logits)."""
    import rvz
    _assert_sees_priors()
    net = _net()
    want = _oracle_games()
    G = 64
    eng = rvz.Engine(G, S, B, memo=memo)
    eng.table(1 << 12, 14)
    eng.root_noise(ALPHA, EPS)
    seeds = torch.arange(1000, 1000 + G, dtype=torch.int64, device="cuda")
    eng.reset(seeds)
    ev = rvz.LeafEvaluator(net)
    nply = torch.zeros(G, dtype=torch.int64, device="cuda")
    ndone = torch.zeros(G, dtype=torch.int64, device="cuda")
    for k in range(6):
        hist = torch.full((1, G), -9, dtype=torch.int32, device="cuda")
        eng.play(ev, 1, 1.0, seeds, G, nply, ndone, reset=False, skip_last_eval=memo, hist=hist,
                 games_per_workgroup=-2)
        wv, wi, wp = want[k]
        assert np.array_equal(hist[0].cpu().numpy(), wi), f"ply {k}: moves differ"
        assert np.array_equal(eng.p_buf.cpu().numpy().view(np.int64), wp.view(np.int64)), \
            f"ply {k}: p differs from the oracle"
    assert int(eng.table_stats[0].item()) > 0          # table hits happened (the shared opening)
    eng.check()


# ---------------------------------------------------------------- fused equals pull-style
def _pull(net, G, plies, memo, skip, seed_base=42, noise=(ALPHA, EPS), keep_p=False):
    import rvz
    eng = rvz.Engine(G, S, B, board_size=net.board_size, compact_leaves=True, memo=memo)
    if noise:
        eng.root_noise(*noise)
    run = rvz.SelfPlayRunner(eng, rvz.LeafEvaluator(net), autoreset=True, seed_base=seed_base,
                             skip_last_eval=skip)
    run.start()
    moves, ps, done = [], [], []
    for _ in range(plies):
        run.ply()
        moves.append(eng.idx_buf.clone())
        if keep_p:
            ps.append(eng.p_buf.clone())
            done.append(run._done.clone())
    return run, torch.stack(moves), ps, done


@functools.lru_cache(maxsize=None)
def _pull_cached(key, G, plies, memo):
    return _pull(_net(*key), G, plies, memo, memo)


def _fused(net, G, plies, memo, skip, gpw, table=False, gate=None, seed_base=42,
           noise=(ALPHA, EPS)):
    import rvz
    eng = rvz.Engine(G, S, B, board_size=net.board_size, memo=memo)
    if table:
        eng.table(1 << 12, 14)
    if gate is not None:
        eng.play_gate(*gate)
    if noise:
        eng.root_noise(*noise)
    run = rvz.SelfPlayRunner(eng, rvz.LeafEvaluator(net), autoreset=True, seed_base=seed_base,
                             skip_last_eval=skip, fused=True)
    run.start()
    hist = torch.full((plies, G), -9, dtype=torch.int32, device="cuda")
    eng.play(run.evaluator, plies, 1.0, run.seeds, run.seed_stride, run._plies, run._done,
             reset=True, skip_last_eval=skip, hist=hist, games_per_workgroup=gpw)
    return run, hist


def _same(a, b):
    (ra, ma), (rb, mb) = a[:2], b[:2]
    assert ma.shape == mb.shape
    for k in range(ma.shape[0]):
        assert torch.equal(ma[k], mb[k]), f"ply {k}: {int((ma[k] != mb[k]).sum())} games differ"
    for x, y in zip(ra.eng.get_state(), rb.eng.get_state()):
        assert torch.equal(x, y)
    assert torch.equal(ra._plies, rb._plies) and torch.equal(ra._done, rb._done)
    assert torch.equal(ra.seeds, rb.seeds)
    assert torch.equal(ra.eng.p_buf, rb.eng.p_buf)
    ra.eng.check()
    rb.eng.check()


@pytest.mark.parametrize("table", [False, True], ids=["notable", "table"])
@pytest.mark.parametrize("memo", [False, True], ids=["nomemo", "memo"])
@pytest.mark.parametrize("gpw", [-6, 5])
def test_fused_equals_pull_style(gpw, memo, table):
    """203 games, 9 plies in one launch: hist, boards, statuses, seeds and counters equal."""
    _assert_sees_priors()
    key = (8, 2, 64, 0)
    ref = _pull_cached(key, 203, 9, memo)
    a = _fused(_net(*key), 203, 9, memo, memo, gpw, table=table)
    assert len({tuple(c) for c in a[1].t().tolist()}) > 1          # distinct games
    _same(a, ref)


@pytest.mark.parametrize("gate", [None, (0.0, 0.0, 0.0)], ids=["gate", "nogate"])
def test_fused_equals_pull_style_pass_gate(gate):
    """The 128-wide form (the pass gate applies to it only), gate default and off."""
    key = (8, 2, 128, 0)
    _assert_sees_priors(*key[:3])
    ref = _pull_cached(key, 203, 9, True)
    _same(_fused(_net(*key), 203, 9, True, True, -6, table=True, gate=gate), ref)


def test_resets_follow_the_new_seed():
    """Board 6, 34 plies with autoreset (a 6x6 game has at most 32): every game restarts; fused
    equals pull-style throughout; and a restarted game's first search does not repeat its
    previous life's, because the noise is keyed by the new seed. Identical noise would give
    identical first plies for every game (same position, same net), so one differing game shows
    the key moved; two lives may still share a visit vector by chance, so not every game must."""
    key = (6, 2, 64, 0)
    _assert_sees_priors(*key[:3])
    net = _net(*key)
    G, plies = 64, 34
    run, moves, ps, done = _pull(net, G, plies, True, True, keep_p=True)
    _same(_fused(net, G, plies, True, True, -6), (run, moves))
    assert bool((run._done >= 1).all())
    differ = 0
    for g in range(G):
        t = next(k for k in range(plies) if int(done[k][g]) >= 1)     # the ply that ended life 1
        assert t + 1 < plies
        differ += not torch.equal(ps[0][g], ps[t + 1][g])
    assert differ >= 1, "every restarted game repeated its first life's first search"


# ---------------------------------------------------------------- off is off, eps = 1
def test_epsilon_zero_is_off():
    import rvz
    net = _net()
    G = 64
    fresh = _pull(net, G, 4, True, True, noise=None)
    eng_off = _pull(net, G, 4, True, True, noise=(ALPHA, 0.0))
    _same(eng_off, fresh)
    # set, then cleared: bitwise a fresh engine's games, pull-style and fused
    eng = rvz.Engine(G, S, B, compact_leaves=True, memo=True)
    eng.root_noise(ALPHA, EPS, salt=5)
    eng.root_noise(ALPHA, 0.0)
    run = rvz.SelfPlayRunner(eng, rvz.LeafEvaluator(net), autoreset=True, seed_base=42,
                             skip_last_eval=True)
    run.start()
    moves = []
    for _ in range(4):
        run.ply()
        moves.append(eng.idx_buf.clone())
    _same((run, torch.stack(moves)), fresh)
    f_off = _fused(net, G, 4, True, True, -6, noise=(ALPHA, 0.0))
    _same(f_off, fresh)
    assert len({tuple(r) for r in fresh[1].t().tolist()}) >= 1


def test_epsilon_one_priors_are_eta():
    """eps = 1: the root's children carry exactly eta (0 * P + 1 * eta), read back through
    rvz_tree_export; roots expanded from an evaluated row and (second ply, memo) from the memo."""
    import rvz
    from oracle import oracle as O
    from noise_oracle import root_eta
    _assert_sees_priors()
    net = _net()
    G = 64
    eng = rvz.Engine(G, S, B, memo=True)
    eng.root_noise(ALPHA, 1.0, salt=9)
    seeds = list(range(300, 300 + G))
    eng.reset(seeds)
    ev = rvz.LeafEvaluator(net)
    games = [O.new_game() for _ in range(G)]
    for ply in range(2):
        eng.search(ev)
        nodes, meta = eng.tree()
        nodes, meta = nodes.cpu().numpy(), meta.cpu().numpy().view(np.uint32)
        eta, legal = root_eta(O, games, seeds, 9, ALPHA)
        for g in range(G):
            m0 = int(meta[g, 0])
            nch, blk = (m0 >> 11) & 127, m0 >> 18
            sq = [s for s in range(64) if int(legal[g]) >> s & 1]
            assert nch == len(sq) > 0
            got = nodes[g, 1 + blk * 64: 1 + blk * 64 + nch, 2]
            assert np.array_equal(got, eta[g, sq].view(np.int32)), (ply, g)
        idx, _ = eng.act(1.0, apply=True)
        for g, a in enumerate(idx.cpu().numpy()):
            assert O.make_move(games[g], -1 if a == 64 else int(a))
    eng.check()


# ---------------------------------------------------------------- SelfPlay, graph
def _selfplay_records(tmp_path, extra, fused, seed=7):
    import rvz
    net = _net(6, 2, 64, 0)
    args = {"num_simulations": S, "batch_size": B, "save_dir": str(tmp_path), "fused": fused}
    if seed is not None:
        args["seed"] = seed
    args.update(extra)
    sp = rvz.SelfPlay(net, args)
    sp.generate_games(4)
    return [t.clone() for t in sp._last_records]


def _records_equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_selfplay_opt_in(tmp_path):
    """root_noise = True turns the noise on (fused and pull-style give equal records, which differ
    from the games without it); dirichlet_* alone, as the reference's pipeline always passes
    them, changes nothing. Both randomness modes."""
    _assert_sees_priors(6, 2, 64)
    on = {"root_noise": True, "dirichlet_alpha": 0.3}
    a = _selfplay_records(tmp_path, on, True)
    b = _selfplay_records(tmp_path, on, False)
    assert _records_equal(a, b)
    plain = _selfplay_records(tmp_path, {}, True)
    assert not _records_equal(a, plain)
    inert = _selfplay_records(tmp_path, {"dirichlet_alpha": 0.3, "dirichlet_epsilon": 0.25}, True)
    assert _records_equal(inert, plain)
    # the global-stream order: the caller's np.random stream, left where the reference leaves it
    outs = []
    for fused in (True, False):
        np.random.seed(3)
        outs.append((_selfplay_records(tmp_path, on, fused, seed=None), np.random.random_sample()))
    assert _records_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
    np.random.seed(3)
    assert not _records_equal(outs[0][0], _selfplay_records(tmp_path, {}, True, seed=None))


def test_graph_replay_keeps_the_noise():
    """A captured fused launch replays with the noise of its capture: the replayed games equal
    the eager ones."""
    import rvz
    _assert_sees_priors()
    net = _net()
    G, plies = 64, 5

    def runner():
        eng = rvz.Engine(G, S, B, memo=True)
        eng.root_noise(ALPHA, EPS)
        run = rvz.SelfPlayRunner(eng, rvz.LeafEvaluator(net), autoreset=True, seed_base=42,
                                 skip_last_eval=True, fused=True)
        run.start()
        return run

    eager, moves_e = runner(), []
    for _ in range(plies):
        eager.ply()
        moves_e.append(eager.eng.idx_buf.clone())
    graphed, moves_g = runner(), []
    graphed.ply()
    moves_g.append(graphed.eng.idx_buf.clone())
    graphed.capture()
    for _ in range(plies - 1):
        graphed.ply()
        moves_g.append(graphed.eng.idx_buf.clone())
    _same((graphed, torch.stack(moves_g)), (eager, torch.stack(moves_e)))
    ref = _pull(net, G, plies, True, True)
    _same((eager, torch.stack(moves_e)), ref[:2])
