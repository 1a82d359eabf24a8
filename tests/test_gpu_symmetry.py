"""Board-symmetry augmentation on the GPU: rvz_board_symmetry and rvz_training_rows against the
NumPy reference (tests/symmetry_ref.py, from the definition T_k = fliplr^f(rot90^r), legal masks
by the CPU oracle), the group laws on the device, agreement with rvz_board_canonical, the quirk
flag, argument and row checks, graph capture, and SelfPlayTrainer(symmetries=...) end to end.
Outputs are pre-filled with NaN / a sentinel before every raw call, so a comparison also shows
that every element was written."""
import numpy as np
import pytest
import torch

import symmetry_ref as S

pytestmark = pytest.mark.gpu

EINVAL = -22
SIZES = (1, 63, 64, 65, 257)           # across wave and block edges
SENTINEL = -77


def _i64(a):
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).cuda()


def _inputs(bs, rows):
    """Device (black, white, status, policy) of rows `rows` of the shared set."""
    b, w, s = S.positions(bs)
    rows = np.asarray(rows, dtype=np.int64)
    status = np.zeros((len(rows), 4), np.int32)
    status[:, 0], status[:, 2] = s[rows], -1
    return (_i64(b[rows]), _i64(w[rows]), torch.from_numpy(status).cuda(),
            torch.from_numpy(S.policies(bs)[rows]).cuda())


def _raw_rows(bs, black, white, status, policy, sym, fan, quirk=True, stream=None, out=None):
    """rvz_training_rows through the C-ABI on pre-filled outputs."""
    import rvz
    from rvz._lib import ptr
    n, m = black.numel(), black.numel() * fan
    if out is None:
        out = (torch.full((m, 3, bs, bs), float("nan"), device="cuda"),
               torch.full((m, bs * bs + 1), float("nan"), device="cuda"),
               torch.full((m,), SENTINEL, dtype=torch.int32, device="cuda"))
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    rc = rvz.load().rvz_training_rows(bs, n, ptr(black), ptr(white), ptr(status), ptr(policy),
                                      None if sym is None else ptr(sym), fan, ptr(out[0]),
                                      ptr(out[1]), ptr(out[2]) if quirk else None, stream)
    assert rc == 0, rc
    return out


def _raw_board(bs, black, white, sym, out_black, out_white):
    import rvz
    from rvz._lib import ptr
    rc = rvz.load().rvz_board_symmetry(bs, black.numel(), ptr(black), ptr(white), ptr(sym),
                                       ptr(out_black), ptr(out_white),
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


def _expect(bs, rows, sym=None):
    """The reference's (states, policy, quirk) on the device: fan = 8 for sym None."""
    if sym is None:
        at = (8 * np.asarray(rows)[:, None] + np.arange(8)[None, :]).reshape(-1)
        out = tuple(a[at] for a in S.reference(bs))
    else:
        out = S.reference_rows(bs, rows, sym)
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in out)


# ---------------------------------------------------------------- rvz_board_symmetry
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bs", [8, 6])
def test_board_symmetry_against_reference(bs, n):
    import rvz
    b, w, _ = S.positions(bs)
    b, w = b[:n], w[:n]
    junk = np.uint64(0)
    if bs == 6:                       # input bits at or above 36 are ignored, outputs stay clean
        junk = np.random.default_rng(n).integers(0, 1 << 28, size=n, dtype=np.uint64) << np.uint64(36)
    db, dw = _i64(b | junk), _i64(w | junk)
    mixed = np.random.default_rng(7 + n).integers(0, 8, size=n).astype(np.int32)
    for sym in [np.full(n, k, np.int32) for k in range(8)] + [mixed]:
        want_b = np.zeros(n, np.uint64)
        want_w = np.zeros(n, np.uint64)
        for k in range(8):
            m = sym == k
            want_b[m], want_w[m] = S.image_bits(b[m], k, bs), S.image_bits(w[m], k, bs)
        ds = torch.from_numpy(sym).cuda()
        ob, ow = rvz.board_symmetry(db, dw, ds, bs)                  # out of place
        assert torch.equal(ob, _i64(want_b)) and torch.equal(ow, _i64(want_w))
        ib, iw = db.clone(), dw.clone()
        _raw_board(bs, ib, iw, ds, ib, iw)                           # in place
        assert torch.equal(ib, ob) and torch.equal(iw, ow)
        if bs == 6:
            assert int((ob >> 36).abs().max()) == 0 and int((ow >> 36).abs().max()) == 0


@pytest.mark.parametrize("bs", [8, 6])
def test_board_symmetry_beyond_one_grid(bs):
    """More boards than the capped grid holds lanes: the grid-stride loop."""
    import rvz
    n = 2048 * 256 + 300
    b, w, _ = S.positions(bs)
    at = np.arange(n) % len(b)
    sym = (np.arange(n) // len(b) + np.arange(n)).astype(np.int32) % 8
    want_b, want_w = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for k in range(8):
        m = sym == k
        want_b[m], want_w[m] = S.image_bits(b[at][m], k, bs), S.image_bits(w[at][m], k, bs)
    ob, ow = rvz.board_symmetry(_i64(b[at]), _i64(w[at]), torch.from_numpy(sym).cuda(), bs)
    assert torch.equal(ob, _i64(want_b)) and torch.equal(ow, _i64(want_w))


@pytest.mark.parametrize("bs", [8, 6])
def test_group_laws_on_the_device(bs):
    import rvz
    b, w, _ = S.positions(bs)
    n = 257
    db, dw = _i64(b[:n]), _i64(w[:n])
    const = [torch.full((n,), k, dtype=torch.int32, device="cuda") for k in range(8)]
    img = [rvz.board_symmetry(db, dw, const[k], bs) for k in range(8)]
    assert torch.equal(img[0][0], db) and torch.equal(img[0][1], dw)
    assert len({t[0].cpu().numpy().tobytes() for t in img}) == 8
    for a in range(8):
        for k in range(8):
            c = rvz.symmetry_compose(a, k)
            assert c == S.COMPOSE[a][k]
            ab, aw = rvz.board_symmetry(*img[k], const[a], bs)       # T_a(T_k(x))
            assert torch.equal(ab, img[c][0]) and torch.equal(aw, img[c][1]), (a, k)
        inv = rvz.symmetry_inverse(a)
        back = rvz.board_symmetry(*img[a], const[inv], bs)
        assert torch.equal(back[0], db) and torch.equal(back[1], dw)


def test_board_symmetry_invalid_sym_and_errors():
    import rvz
    b, w, _ = S.positions(8)
    db, dw = _i64(b[:6]), _i64(w[:6])
    sym = torch.tensor([3, -1, 5, 8, 0, 1 << 20], dtype=torch.int32, device="cuda")
    ob, ow = rvz.board_symmetry(db, dw, sym, 8)
    for i, k in enumerate(sym.tolist()):
        if 0 <= k < 8:
            assert int(ob[i]) == int(S.image_bits(b[i:i + 1], k, 8).view(np.int64)[0])
            assert int(ow[i]) == int(S.image_bits(w[i:i + 1], k, 8).view(np.int64)[0])
        else:
            assert int(ob[i]) == 0 and int(ow[i]) == 0
    e = torch.empty(0, dtype=torch.int64, device="cuda")
    assert rvz.board_symmetry(e, e, e.to(torch.int32), 6)[0].numel() == 0
    with pytest.raises(rvz.RvzError):
        rvz.board_symmetry(db, dw, sym, 7)
    with pytest.raises(rvz.RvzError):
        rvz.board_symmetry(db, dw[:3], sym, 8)
    with pytest.raises(rvz.RvzError):
        rvz.board_symmetry(db, dw, sym.float(), 8)
    with pytest.raises(rvz.RvzError):
        rvz.board_symmetry(db.to(torch.int32), dw, sym, 8)


# ---------------------------------------------------------------- rvz_training_rows
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fan", [1, 8])
@pytest.mark.parametrize("bs", [8, 6])
def test_training_rows_against_reference(bs, fan, n):
    rows = np.arange(n)
    sym = None
    if fan == 1:
        sym = np.random.default_rng(100 * bs + n).integers(0, 8, size=n).astype(np.int32)
    dsym = None if sym is None else torch.from_numpy(sym).cuda()
    got = _raw_rows(bs, *_inputs(bs, rows), dsym, fan)
    want = _expect(bs, rows, sym)
    for g, x, name in zip(got, want, ("states", "policy", "quirk")):
        assert g.dtype == x.dtype and torch.equal(g, x), name
    # out_quirk is nullable: the same states and policy, the quirk array untouched
    no = _raw_rows(bs, *_inputs(bs, rows), dsym, fan, quirk=False)
    assert torch.equal(no[0], got[0]) and torch.equal(no[1], got[1])
    assert bool((no[2] == SENTINEL).all())


@pytest.mark.parametrize("bs", [8, 6])
def test_training_rows_whole_set(bs):
    """Every row of the shared set (both quirk classes are in it), repeated until the batch
    exceeds what the capped grid takes in one step: the grid-stride loop, through rvz.training_rows."""
    import rvz
    total = len(S.positions(bs)[0])
    rows = np.arange(3 * total) % total
    assert len(rows) > 2048 * 4
    black, white, status, policy = _inputs(bs, rows)
    states, pol, quirk = rvz.training_rows(black, white, status, policy, board_size=bs,
                                           all_images=True, quirk=True)
    want = _expect(bs, rows)
    assert torch.equal(states, want[0]) and torch.equal(pol, want[1])
    assert torch.equal(quirk, want[2])
    q8 = quirk.reshape(-1, 8)
    assert int((q8 == 1).sum()) > 0 and int((q8[:, 1:] == 0).sum()) > 0
    assert not bool(q8[:, 0].any())
    two = rvz.training_rows(black, white, status, policy, board_size=bs, all_images=True)
    assert len(two) == 2 and torch.equal(two[0], states) and torch.equal(two[1], pol)
    sym = torch.from_numpy((np.arange(len(rows)) * 5 // 3 % 8).astype(np.int32)).cuda()
    one = rvz.training_rows(black, white, status, policy, sym, bs, quirk=True)
    want1 = _expect(bs, rows, sym.cpu().numpy())
    for g, x in zip(one, want1):
        assert torch.equal(g, x)


@pytest.mark.parametrize("bs", [8, 6])
def test_training_rows_n_zero(bs):
    import rvz
    e64 = torch.empty(0, dtype=torch.int64, device="cuda")
    st = torch.empty(0, 4, dtype=torch.int32, device="cuda")
    pol = torch.empty(0, bs * bs + 1, device="cuda")
    for every in (False, True):
        out = rvz.training_rows(e64, e64, st, pol, e64.to(torch.int32), bs, every, quirk=True)
        assert out[0].shape == (0, 3, bs, bs) and out[1].shape == (0, bs * bs + 1)
        assert out[2].shape == (0,)
    lib = rvz.load()
    for fan in (1, 8):
        assert lib.rvz_training_rows(bs, 0, None, None, None, None, None, fan, None, None, None,
                                     torch.cuda.current_stream().cuda_stream) == 0


@pytest.mark.parametrize("bs", [8, 6])
def test_identity_and_agreement_between_calls(bs):
    import rvz
    n = 257
    black, white, status, policy = _inputs(bs, np.arange(n))
    st8, pol8, q8 = rvz.training_rows(black, white, status, policy, board_size=bs,
                                      all_images=True, quirk=True)
    assert torch.equal(st8[::8], rvz.board_canonical(black, white, status, bs))
    assert torch.equal(pol8[::8], policy)
    for k in range(8):
        sym = torch.full((n,), k, dtype=torch.int32, device="cuda")
        st1, pol1, q1 = rvz.training_rows(black, white, status, policy, sym, bs, quirk=True)
        assert torch.equal(st1, st8[k::8]) and torch.equal(pol1, pol8[k::8])
        assert torch.equal(q1, q8[k::8])
    # permutation and pass: the values are moved, never recomputed
    nsq = bs * bs
    assert torch.equal(pol8[:, nsq].reshape(n, 8), policy[:, nsq:].expand(n, 8))
    moved = pol8[:, :nsq].contiguous().view(torch.int32).sort(dim=1).values.reshape(n, 8, nsq)
    assert torch.equal(moved, policy[:, :nsq].contiguous().view(torch.int32).sort(dim=1).values
                       .unsqueeze(1).expand(n, 8, nsq))
    assert len({pol8[8 * 0 + k].cpu().numpy().tobytes() for k in range(8)}) == 8   # a dense row


@pytest.mark.parametrize("bs", [8, 6])
def test_quirk_is_the_engines_own_mask_differing(bs):
    """quirk == 0: plane 3 equals board_canonical's plane 3 of the board_symmetry image position;
    quirk == 1: they differ. Planes 1 and 2 always equal the image position's."""
    import rvz
    n = 1024
    black, white, status, policy = _inputs(bs, np.arange(n))
    st8, _, q8 = rvz.training_rows(black, white, status, policy, board_size=bs, all_images=True,
                                   quirk=True)
    sym = torch.arange(8, dtype=torch.int32, device="cuda").repeat(n)
    ib, iw = rvz.board_symmetry(black.repeat_interleave(8), white.repeat_interleave(8), sym, bs)
    own = rvz.board_canonical(ib, iw, status.repeat_interleave(8, dim=0).contiguous(), bs)
    assert torch.equal(own[:, :2], st8[:, :2])
    differs = (own[:, 2] != st8[:, 2]).flatten(1).any(dim=1)
    assert torch.equal(differs, q8 == 1) and bool(((q8 == 0) | (q8 == 1)).all())
    assert int(differs.sum()) > 0 and int((~differs).reshape(n, 8)[:, 1:].sum()) > 0


@pytest.mark.parametrize("bs", [8, 6])
def test_invalid_sym_rows(bs):
    n = 65
    rows = np.arange(n)
    sym = np.random.default_rng(3).integers(0, 8, size=n).astype(np.int32)
    sym[[0, 7, 31, 32, 64]] = [-1, 8, -2 ** 31, 2 ** 31 - 1, 9]
    got = _raw_rows(bs, *_inputs(bs, rows), torch.from_numpy(sym).cuda(), 1)
    want = _expect(bs, rows, sym)
    for g, x in zip(got, want):
        assert torch.equal(g, x)                    # the neighbouring rows are untouched
    bad = torch.tensor([0, 7, 31, 32, 64], device="cuda")
    assert bool((got[2][bad] == -1).all()) and int((got[2] == -1).sum()) == 5
    assert not bool(got[0][bad].any()) and not bool(got[1][bad].any())


@pytest.mark.parametrize("bs", [8, 6])
def test_row_independence(bs):
    """A row's outputs at index 0 of a 1-row call and in the middle of a 257-row call."""
    mid = 130
    for fan in (1, 8):
        sym = None if fan == 8 else torch.full((257,), 5, dtype=torch.int32, device="cuda")
        big = _raw_rows(bs, *_inputs(bs, np.arange(257)), sym, fan)
        one = _raw_rows(bs, *_inputs(bs, [mid]), None if sym is None else sym[:1].clone(), fan)
        for a, b in zip(big, one):
            assert torch.equal(a[mid * fan:(mid + 1) * fan], b)


def test_einval_through_the_c_abi():
    import rvz
    from rvz._lib import ptr
    lib = rvz.load()
    black, white, status, policy = _inputs(8, np.arange(4))
    sym = torch.zeros(4, dtype=torch.int32, device="cuda")
    st = torch.full((32, 3, 8, 8), float("nan"), device="cuda")
    pol = torch.full((32, 65), float("nan"), device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    good = [8, 4, ptr(black), ptr(white), ptr(status), ptr(policy), ptr(sym), 1, ptr(st),
            ptr(pol), None, stream]
    assert lib.rvz_training_rows(*good) == 0
    for k, v in ((0, 7), (0, 4), (1, -1), (7, 0), (7, 2), (7, 16), (8, ptr(st) + 4),
                 (1, 2 ** 31 // 65 + 1)):
        args = list(good)
        args[k] = v
        assert lib.rvz_training_rows(*args) == EINVAL, (k, v)
    for k in (2, 3, 4, 5, 6, 8, 9):
        args = list(good)
        args[k] = None
        assert lib.rvz_training_rows(*args) == EINVAL, k
    args = list(good)
    args[6], args[7] = None, 8                       # sym may be null with fan = 8
    assert lib.rvz_training_rows(*args) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(st).any()) and not bool(torch.isnan(pol).any())
    ob = torch.empty(4, dtype=torch.int64, device="cuda")
    goodb = [8, 4, ptr(black), ptr(white), ptr(sym), ptr(ob), ptr(ob.clone()), stream]
    assert lib.rvz_board_symmetry(*goodb) == 0
    for k, v in ((0, 5), (1, -3), (2, None), (3, None), (4, None), (5, None), (6, None)):
        args = list(goodb)
        args[k] = v
        assert lib.rvz_board_symmetry(*args) == EINVAL, (k, v)
    # the Python surface refuses malformed arrays before the library sees them
    for call in (lambda: rvz.training_rows(black, white, status, policy[:, :64], sym),
                 lambda: rvz.training_rows(black, white, status, policy.double(), sym),
                 lambda: rvz.training_rows(black, white, status[:, :3], policy, sym),
                 lambda: rvz.training_rows(black, white, status, policy),          # no sym
                 lambda: rvz.training_rows(black, white, status, policy, sym[:2]),
                 lambda: rvz.training_rows(black, white, status, policy, sym, 7)):
        with pytest.raises(rvz.RvzError):
            call()


def test_graph_capture():
    """One rvz_training_rows call captured and replayed after the inputs change."""
    bs, n = 8, 257
    a = _inputs(bs, np.arange(n))
    b = _inputs(bs, np.arange(n, 2 * n))
    sym_a = np.random.default_rng(1).integers(0, 8, size=n).astype(np.int32)
    sym_b = np.random.default_rng(2).integers(0, 8, size=n).astype(np.int32)
    for fan in (1, 8):
        ins = [t.clone() for t in a]
        sym = torch.from_numpy(sym_a).cuda()
        eager = [t.clone() for t in _raw_rows(bs, *ins, sym, fan)]               # warm
        torch.cuda.synchronize()
        out = tuple(torch.empty_like(t) for t in eager)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _raw_rows(bs, *ins, sym, fan, stream=torch.cuda.current_stream().cuda_stream, out=out)
        for src, s in ((b, sym_b), (a, sym_a)):
            for t, x in zip(ins, src):
                t.copy_(x)
            sym.copy_(torch.from_numpy(s))
            out[0].fill_(float("nan"))
            out[1].fill_(float("nan"))
            out[2].fill_(SENTINEL)
            graph.replay()
            rows = np.arange(n, 2 * n) if src is b else np.arange(n)
            want = _expect(bs, rows, s if fan == 1 else None)
            for g, x in zip(out, want):
                assert torch.equal(g, x)
        assert torch.equal(out[0], eager[0]) and torch.equal(out[2], eager[2])


# ---------------------------------------------------------------- end to end
def test_selfplay_trainer_with_symmetries():
    import copy

    import rvz
    from rvz.pipeline import SelfPlayTrainer
    from rvz.trainer import records_to_training
    torch.manual_seed(0)
    G, sims = 8, 200      # four leaf batches: distinct games (test_gpu_pipeline.py's count)
    net = rvz.AlphaZeroNetwork(8, 2, 64).cuda()
    kw = dict(num_simulations=sims, seed=7, train_steps=1, train_batch=64)
    base = SelfPlayTrainer(copy.deepcopy(net), G, **kw).generate()
    spt = SelfPlayTrainer(net, G, symmetries="all", **kw)
    data = spt.generate()
    n = base["states"].shape[0]
    assert n >= 9 * G and set(data) == set(base) | {"symmetry_rows", "symmetry_quirk_rows"}
    for k in ("states", "policy_targets", "value_targets"):
        assert data[k].shape[0] == 8 * n and data[k].dtype == base[k].dtype
        assert torch.equal(data[k][::8], base[k]), k
    assert torch.equal(data["value_targets"].reshape(n, 8), base["value_targets"].expand(n, 8))
    assert int(data["symmetry_rows"]) == 8 * n
    assert 0 <= int(data["symmetry_quirk_rows"]) <= 7 * n
    # every row's policy mass lies where its plane 3 is 1, or on the pass
    off_mask = (data["policy_targets"][:, :64].reshape(-1, 8, 8) > 0) & (data["states"][:, 2] == 0)
    assert not bool(off_mask.any())
    assert bool((data["policy_targets"].sum(dim=1) - 1).abs().max() < 1e-5)
    # "random": reproducible for a fixed seed, rows taken from the eight images by its draws
    spt.symmetries, spt.symmetry_seed = "random", 5
    r1 = spt.generate()
    run = spt.runner                    # the same records once more: generate()'s own tail
    r2 = records_to_training(run.rec_black, run.rec_white, run.rec_side, run.rec_idx, run.rec_p,
                             run.post_status, 8, symmetries="random", symmetry_seed=5)
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k
    sym = torch.randint(0, 8, (n,), generator=torch.Generator().manual_seed(5))
    at = 8 * torch.arange(n, device="cuda") + sym.cuda()
    assert torch.equal(r1["states"], data["states"][at])
    assert torch.equal(r1["policy_targets"], data["policy_targets"][at])
    assert torch.equal(r1["value_targets"], base["value_targets"])
    assert int(r1["symmetry_rows"]) == n
    # default seed: seed + iteration (world 1), another draw than seed 5
    spt.symmetry_seed = None
    assert spt._symmetry_args() == {"symmetries": "random", "symmetry_seed": 7}
    spt.symmetries = "all"
    losses = spt.train(data)
    assert losses["steps"] == 1 and np.isfinite(losses["train/loss"])
    assert np.isfinite(losses["train/policy_loss"]) and np.isfinite(losses["train/value_loss"])
