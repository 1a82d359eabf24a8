"""policy_softmax<NSQ> (csrc/rvz_search.hip.h), the one device function every prior of every
search tree comes from, against the float64 reference of tests/softmax_ref.py at every output,
under the bound derived in tests/test_softmax_ref_cpu.py:

    |p - ref| <= max((d + 8) * 2^-23 * ref, 2^-148),   |sum(p) - 1| <= 16 * 2^-24.

The oracle helpers (tests/oracle_play.py, tests/noise_oracle.py, the smoke) feed the CPU oracle
with rvz.policy_softmax, so their bitwise comparisons cannot see an error in it; this file is
what licenses that.

The stateless call (rvz_policy_softmax through the C-ABI, outputs pre-filled with NaN, a guard of
64 floats behind both buffers), boards 8 and 6, n in {1, 3, 4, 5, 257} rows (the kernel runs 4
rows per workgroup: 3 and 5 straddle one, 257 leaves a one-row tail). The 257 rows of
softmax_ref.pool, by family:
  random_1/3/10/30   N(0, scale^2) logits; outlier: N(0, 3^2) with one entry raised by 60
  (a) a_max_pass     the maximum at the pass index, by 0.5, 5 and 50
  (b) b_max_sq0/last the maximum at square 0 and at square S*S-1
  (c) c_equal        all entries 0, -1e30, 3e38: one float32 everywhere, no inf or NaN
  (d) d_one_hot      one entry (a square, the pass) 1e4 above the rest: exactly 1.0, the others 0
  (e) e_ladder       d = 0, 10, .., 100 across the row and d = 80 .. 112 in fine steps: float32
                     denormal results, non-zero wherever ref >= 2^-148 (the library is built with
                     -fno-gpu-flush-denormals-to-zero; an exact 0 prior changes UCB ties)
  (f) f_neg_inf      -inf at a square, at the pass, at every other square: exactly 0 there
  (g) g_alternate    consecutive rows at offsets 0 and +1e4 in turn: on 6x6 the floats behind a
                     row's 37 entries are far larger than the row, so a lane >= 36 that leaked
                     into the maximum or the sum gives a wrong row
  (h) h_shifted      whole rows at offsets -87, -200, -1e4, +200: lanes >= 36 hold the logit 0.0
                     on 6x6, which only a row far below 0 tells from a masked lane
Besides the bound and the row sum: monotonicity within a row, a row alone (n = 1) has the bits it
has inside the 257-row batch, two calls return equal bytes. NaN and all -inf rows are not given
to this call: ERR_NN covers them in the engine (tests/test_gpu_selfplay_parity.py).

The pull-style expand (search_submit(is_logits=True)) at roots with many legal moves: the
children are the legal squares in row-major order and each prior is bit for bit
rvz.policy_softmax's, hence within the bound. The fused k_play exports no priors; its games equal
the pull-style ones (tests/test_gpu_set_roots.py, tests/test_gpu_play_oracle.py).

Largest fraction of the bound measured on the MI355X (printed by the tests; the same for every
n), 8x8 / 6x6: random_1 0.28 / 0.28, random_3 0.32 / 0.35, random_10 0.42 / 0.41, random_30
0.52 / 0.66, outlier 0.43 / 0.44, a 0.31 / 0.34, b 0.42 / 0.28, c 0.00 / 0.03, d 0.00 / 0.00,
e 0.40 / 0.24, f 0.31 / 0.29, g 0.24 / 0.18, h 0.11 / 0.10; at the expand's children at most
0.52 / 0.50."""
import random

import numpy as np
import pytest
import torch

import softmax_ref as S

pytestmark = pytest.mark.gpu

BOARDS = (8, 6)
COUNTS = (1, 3, 4, 5, 257)
GUARD = 64
BIG = 3.0e38


def _call(bs, rows):
    """rvz_policy_softmax on `rows` (host float32 [n, npol]): a fresh input buffer with GUARD
    floats of 3e38 behind the rows, a NaN-filled output with a NaN guard that must stay NaN."""
    from rvz import _lib
    lib = _lib.load()
    n, npol = rows.shape
    host = np.full(n * npol + GUARD, BIG, np.float32)
    host[:n * npol] = rows.reshape(-1)
    x = torch.from_numpy(host).cuda()
    out = torch.full((n * npol + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    rc = lib.rvz_policy_softmax(bs, n, _lib.ptr(x), _lib.ptr(out), _lib.stream_handle(x.device))
    assert rc == 0, rc
    res = out.cpu().numpy()
    assert np.isnan(res[n * npol:]).all(), "wrote behind the last row"
    return res[:n * npol].reshape(n, npol).copy()


@pytest.fixture(scope="module")
def batch():
    """The whole pool in one call, per board (computed once)."""
    cache = {}

    def get(bs):
        if bs not in cache:
            cache[bs] = _call(bs, S.pool(bs)[0])
            cache[bs].setflags(write=False)
        return cache[bs]
    return get


def _report(bs, what, worst):
    print(f"{bs}x{bs} {what}: largest fraction of the bound: "
          + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("bs", BOARDS)
def test_stateless_call(batch, bs, n):
    """The pool in calls of n rows each (chunks from the front; the last chunk is the last n
    rows): every output under the bound, the row sums, monotonicity, the exact expectations, and
    every row's bits those it has in the 257-row call."""
    z, fam = S.pool(bs)
    got = np.full(z.shape, np.nan, np.float32)
    starts = sorted(set(list(range(0, len(z) - n + 1, n)) + [len(z) - n]))
    for s in starts:
        p = _call(bs, z[s:s + n])
        assert not np.isnan(p).any(), (bs, n, s, "an output is NaN or was not written")
        seen = ~np.isnan(got[s:s + n]).any(1)
        assert np.array_equal(p[seen].view(np.int32), got[s:s + n][seen].view(np.int32))
        got[s:s + n] = p
    worst = S.check_rows(z, fam, got, (bs, n), S.pool_ref(bs))
    _report(bs, f"n = {n}", worst)
    assert np.array_equal(got.view(np.int32), batch(bs).view(np.int32)), \
        (bs, n, "rows differ from the 257-row call",
         np.flatnonzero((got.view(np.int32) != batch(bs).view(np.int32)).any(1))[:8].tolist())


@pytest.mark.parametrize("bs", BOARDS)
def test_two_calls_equal_bytes(batch, bs):
    assert _call(bs, S.pool(bs)[0]).tobytes() == batch(bs).tobytes()


@pytest.mark.parametrize("bs", BOARDS)
def test_python_wrapper_is_the_call(batch, bs):
    """rvz.policy_softmax (what the oracle helpers call) returns the C-ABI call's bits."""
    import rvz
    z = torch.from_numpy(S.pool(bs)[0].copy()).cuda()
    p = rvz.policy_softmax(z, bs).cpu().numpy()
    assert np.array_equal(p.view(np.int32), batch(bs).view(np.int32))


# ------------------------------------------------------------------ the pull-style expand
G = 64
CORNER_GAMES = 16
MIN_LEGAL = {8: 10, 6: 8}


def expand_roots(O, R, bs):
    """64 positions of seeded random playouts (random.Random(seed), at most two per seed), each
    with at least MIN_LEGAL legal moves: first 16 where square 0 and square S*S-1 are both legal,
    then 48 others."""
    nsq = bs * bs
    corner, plain = [], []
    seed = 0
    while len(corner) < CORNER_GAMES or len(plain) < G - CORNER_GAMES:
        rng = random.Random(seed)
        seed += 1
        g = O.new_game(bs)
        took = [False, False]
        while not g.over:
            lm = R.mover_mask(g, bs)
            if bin(lm).count("1") >= MIN_LEGAL[bs]:
                both = bool(lm & 1 and lm >> (nsq - 1) & 1)
                want = corner if both else plain
                cap = CORNER_GAMES if both else G - CORNER_GAMES
                if not took[both] and len(want) < cap and rng.random() < 0.5:
                    want.append(g.copy())
                    took[both] = True
            assert O.make_move(g, rng.choice(list(R.squares(lm))), bs)
        assert seed < 2000
    return corner + plain


def expand_rows(bs):
    """64 pool rows for the 64 games: every structured row whose pass logit is finite (a
    non-finite pass logit is an NN error to the engine, ERR_NN), 3 outlier rows and the random
    scales in equal parts. Returns the pool indices."""
    z, fam = S.pool(bs)
    structured = [i for i in range(len(z))
                  if not fam[i].startswith(("random", "outlier")) and np.isfinite(z[i, -1])]
    idx = structured + list(np.flatnonzero(fam == "outlier")[:3])
    per = (G - len(idx)) // len(S.SCALES)
    for s in S.SCALES:
        idx += list(np.flatnonzero(fam == f"random_{s}")[:per])
    idx += list(np.flatnonzero(fam == "random_30")[per:per + G - len(idx)])
    assert len(idx) == G == len(set(idx))
    return np.array(idx)


@pytest.mark.parametrize("bs", BOARDS)
def test_expand_priors_are_the_stateless_call(oracle, batch, bs):
    """One search batch (64 games, num_simulations = batch_size = 64) at roots with 10+ (6x6: 8+)
    legal moves, 16 of them with both far corners legal; search_submit(rows, 0, is_logits=True),
    then the tree. Four rounds with the rows rotated by 16 games, so every row meets a corner
    root once. The root's children are its legal squares in row-major order, none the pass; each
    prior is bit for bit rvz.policy_softmax(rows)[g, square], and within the bound of the float64
    reference; eng.check() is clean."""
    import rvz
    import solve_ref as R
    O = oracle
    nsq = bs * bs
    games = expand_roots(O, R, bs)
    legal = [R.mover_mask(g, bs) for g in games]
    squares = [list(R.squares(lm)) for lm in legal]
    assert all(len(s) >= MIN_LEGAL[bs] for s in squares) and max(map(len, squares)) >= 12
    assert all(s[0] == 0 and s[-1] == nsq - 1 for s in squares[:CORNER_GAMES])
    z, fam = S.pool(bs)
    ref, d = S.pool_ref(bs)
    pick = expand_rows(bs)
    eng = rvz.Engine(G, num_simulations=64, batch_size=64, board_size=bs)
    value = torch.zeros(G, device="cuda")
    worst, met = {}, set()
    for rnd in range(G // CORNER_GAMES):
        rows = np.roll(pick, CORNER_GAMES * rnd)
        logits = torch.from_numpy(z[rows]).cuda()
        eng.reset(range(G))
        eng.set_state(*R.to_device(games))
        eng.search_begin()
        assert eng.search_step()
        eng.search_submit(logits, value, is_logits=True)
        nodes, meta = eng.tree()
        want = rvz.policy_softmax(logits, bs).cpu().numpy()
        torch.cuda.synchronize()
        eng.check()
        assert np.array_equal(want.view(np.int32), batch(bs)[rows].view(np.int32))
        nodes, meta = nodes.cpu().numpy(), meta.cpu().numpy().view(np.uint32)
        for g in range(G):
            L = len(squares[g])
            rm = int(meta[g, 0])
            assert (rm >> 11) & 127 == L, (bs, rnd, g, hex(rm))      # the root's child count
            c0 = 1 + (rm >> 18) * nsq                                # and its children's block
            sq = (meta[g, c0:c0 + L] & 63).tolist()
            assert sq == squares[g] and all(s < nsq for s in sq), (bs, rnd, g, sq, squares[g])
            pri = nodes[g, c0:c0 + L, 2].copy().view(np.float32)
            assert np.array_equal(pri.view(np.int32), want[g, sq].view(np.int32)), \
                (bs, rnd, g, fam[rows[g]], pri, want[g, sq])
            f = S.fraction(pri, ref[rows[g], sq], d[rows[g], sq])
            assert (f <= 1.0).all(), (bs, rnd, g, fam[rows[g]], f.max())
            k = str(fam[rows[g]])
            worst[k] = max(worst.get(k, 0.0), float(f.max()))
            if g < CORNER_GAMES:
                met.add(k)
    assert {"b_max_sq0", "b_max_last", "a_max_pass", "e_ladder", "f_neg_inf"} <= met
    _report(bs, "expand", dict(sorted(worst.items())))
