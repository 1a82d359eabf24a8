"""Board-symmetry augmentation on the CPU (no GPU): the host reference's own group laws
(tests/symmetry_ref.py), rvz.symmetry_compose / symmetry_inverse against its tables,
records_to_training(symmetries=...) with the NumPy `augment` and the oracle's `canonical`
injected, and the argument checks of the two entry points at the C-ABI (they run before any HIP
call)."""
import numpy as np
import pytest
import torch

import symmetry_ref as S
from test_pipeline_cpu import synthetic_records
from test_solve_cpu import _train

EINVAL = -22


# ---------------------------------------------------------------- the reference itself
def test_reference_group_laws():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 1 << 30, size=(8, 8))                # an asymmetric board
    imgs = [S.image(x, k) for k in range(8)]
    assert np.array_equal(imgs[0], x)                         # T_0 is the identity
    assert len({a.tobytes() for a in imgs}) == 8              # eight distinct images
    for a in range(8):
        for b in range(8):
            c = S.COMPOSE[a][b]
            assert 0 <= c < 8                                 # closure
            assert np.array_equal(S.image(S.image(x, b), a), imgs[c])
        assert np.array_equal(S.image(imgs[a], S.INVERSE[a]), x)
        assert S.COMPOSE[S.INVERSE[a]][a] == 0 == S.COMPOSE[a][S.INVERSE[a]]
    assert sorted(S.COMPOSE[3]) == list(range(8))
    # the numbering in words: 4 mirrors the columns, 6 the rows, 7 is the transpose
    assert np.array_equal(imgs[4], x[:, ::-1]) and np.array_equal(imgs[6], x[::-1])
    assert np.array_equal(imgs[7], x.T) and np.array_equal(imgs[2], x[::-1, ::-1])


@pytest.mark.parametrize("bs", [8, 6])
def test_reference_bitboards_and_policies(bs):
    nsq = bs * bs
    rng = np.random.default_rng(bs)
    bits = rng.integers(0, 1 << 63, size=50, dtype=np.uint64) & np.uint64((1 << nsq) - 1)
    assert np.array_equal(S.pack(S.unpack(bits, bs)), bits)
    for k in range(8):
        img = S.image_bits(bits, k, bs)
        assert np.array_equal(S.image_bits(img, S.INVERSE[k], bs), bits)
        assert all(bin(int(a)).count("1") == bin(int(b)).count("1") for a, b in zip(img, bits))
        # square s of the image is square src of the original; the policy moves the same way
        pol = rng.random((50, nsq + 1)).astype(np.float32)
        out = S.image_policy(pol, k, bs)
        assert np.array_equal(out[:, nsq], pol[:, nsq])
        src = S.image(np.arange(nsq).reshape(bs, bs), k).reshape(-1)
        assert np.array_equal(out[:, :nsq], pol[:, src])
        assert np.array_equal((img[:, None] >> np.arange(nsq, dtype=np.uint64)) & np.uint64(1),
                              (bits[:, None] >> src.astype(np.uint64)) & np.uint64(1))
    # bits at or above S*S are dropped
    if bs == 6:
        assert np.array_equal(S.image_bits(bits | np.uint64(1 << 63) | np.uint64(1 << 36), 0, bs),
                              bits)


@pytest.mark.parametrize("bs", [8, 6])
def test_shared_set_holds_both_quirk_classes(bs):
    """The set the GPU tests compare on: the wrap-around quirk fires for some (row, k) and not for
    some non-identity (row, k); the identity never has it; every policy row's mass lies on the
    image of the legal mask or on the pass, except the dense rows."""
    st, pol, q = S.reference(bs)
    n = len(S.positions(bs)[0])
    assert st.shape == (8 * n, 3, bs, bs) and pol.shape == (8 * n, bs * bs + 1) and n > 3000
    q8 = q.reshape(n, 8)
    fires, quiet = int((q8 == 1).sum()), int((q8[:, 1:] == 0).sum())
    print(f"{bs}x{bs}: {n} rows, quirk 1 at {fires} (row, k), 0 at {quiet} non-identity (row, k)")
    assert fires > 0 and quiet > 0 and not q8[:, 0].any()
    for m in (63, 257):                                       # and within the small prefixes
        assert (q8[:m] == 1).any() and (q8[:m, 1:] == 0).any()
    sparse = np.ones(8 * n, bool)
    sparse.reshape(n, 8)[::16] = False
    off_mask = (pol[:, :-1].reshape(8 * n, bs, bs) > 0) & (st[:, 2] == 0)
    assert not off_mask[sparse].any() and off_mask[~sparse].any()
    assert np.array_equal(st[::8], S.canonical(*S.positions(bs), bs))


def test_python_group_table_is_the_references():
    import rvz
    for a in range(8):
        assert rvz.symmetry_inverse(a) == S.INVERSE[a]
        for b in range(8):
            assert rvz.symmetry_compose(a, b) == S.COMPOSE[a][b]


def test_argument_errors():
    import rvz
    for bad in (-1, 8, 1.0, True, None, "1"):
        with pytest.raises(rvz.RvzError):
            rvz.symmetry_inverse(bad)
        with pytest.raises(rvz.RvzError):
            rvz.symmetry_compose(bad, 0)
        with pytest.raises(rvz.RvzError):
            rvz.symmetry_compose(0, bad)
    rec, _ = synthetic_records(G=2)
    for bad in ("ALL", "some", 8, True):
        with pytest.raises(ValueError):
            _train(rec, 8, symmetries=bad, augment=S.augment)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """RVZ_EINVAL before any HIP call (the pointers are never dereferenced)."""
    import rvz
    lib = rvz.load()
    p = 0x10000
    assert lib.rvz_board_symmetry(8, 0, None, None, None, None, None, None) == 0
    assert lib.rvz_board_symmetry(7, 4, p, p, p, p, p, None) == EINVAL
    assert lib.rvz_board_symmetry(8, -1, p, p, p, p, p, None) == EINVAL
    for k in range(2, 7):
        args = [8, 4, p, p, p, p, p, None]
        args[k] = None
        assert lib.rvz_board_symmetry(*args) == EINVAL, k
    good = [8, 4, p, p, p, p, p, 1, p, p, None, None]
    assert lib.rvz_training_rows(8, 0, None, None, None, None, None, 8, None, None, None,
                                 None) == 0
    assert lib.rvz_training_rows(6, 0, None, None, None, None, None, 1, None, None, None,
                                 None) == 0
    for k, v in ((0, 7), (0, 4), (1, -1), (7, 0), (7, 2), (7, 4), (7, -8), (8, p + 4), (8, p + 8)):
        args = list(good)
        args[k] = v
        assert lib.rvz_training_rows(*args) == EINVAL, (k, v)
    for k in (2, 3, 4, 5, 6, 8, 9):                           # sym (6) is required with fan = 1
        args = list(good)
        args[k] = None
        assert lib.rvz_training_rows(*args) == EINVAL, k
    # n * fan * (S*S + 1) must fit int32, also with n = 0 rows of work refused first by the size
    assert lib.rvz_training_rows(8, 2 ** 31 // 65 + 1, p, p, p, p, p, 1, p, p, None,
                                 None) == EINVAL
    assert lib.rvz_training_rows(8, 2 ** 31 // (8 * 65) + 1, p, p, p, p, None, 8, p, p, None,
                                 None) == EINVAL
    assert lib.rvz_training_rows(6, 2 ** 31 // (8 * 37) + 1, p, p, p, p, None, 8, p, p, None,
                                 None) == EINVAL


# ---------------------------------------------------------------- records_to_training
def test_symmetries_none_is_byte_identical():
    rec, _ = synthetic_records(G=6, seed=3)
    calls = []

    def augment(*a):
        calls.append(a)
        return S.augment(*a)

    base = _train(rec, 8)
    off = _train(rec, 8, symmetries=None, symmetry_seed=5, augment=augment)
    assert not calls and list(off) == list(base) == ["states", "policy_targets", "value_targets"]
    for k in base:
        assert off[k].dtype == base[k].dtype and off[k].shape == base[k].shape
        assert off[k].numpy().tobytes() == base[k].numpy().tobytes(), k


def test_symmetries_all():
    rec, _ = synthetic_records(G=6, seed=3)
    base = _train(rec, 8)
    out = _train(rec, 8, symmetries="all", augment=S.augment)
    n = base["states"].shape[0]
    assert set(out) == set(base) | {"symmetry_rows", "symmetry_quirk_rows"}
    assert out["states"].shape == (8 * n, 3, 8, 8) and out["states"].dtype == torch.float32
    assert out["policy_targets"].shape == (8 * n, 65)
    assert out["policy_targets"].dtype == torch.float32
    assert out["value_targets"].shape == (8 * n, 1)
    for k in ("states", "policy_targets", "value_targets"):
        assert out[k][::8].numpy().tobytes() == base[k].numpy().tobytes(), k
    assert torch.equal(out["value_targets"].reshape(n, 8),
                       base["value_targets"].expand(n, 8))
    for k in range(8):
        st = out["states"][k::8].numpy()
        assert np.array_equal(st, np.stack([[S.image(p, k) for p in row]
                                            for row in base["states"].numpy()]))
        assert np.array_equal(out["policy_targets"][k::8].numpy(),
                              S.image_policy(base["policy_targets"].numpy(), k, 8))
    for k in ("symmetry_rows", "symmetry_quirk_rows"):
        assert out[k].dim() == 0 and out[k].dtype == torch.int64
    assert int(out["symmetry_rows"]) == 8 * n
    live = (rec["rec_idx"] >= 0).t().reshape(-1).numpy()
    b = rec["rec_black"].t().reshape(-1).numpy()[live].view(np.uint64)
    w = rec["rec_white"].t().reshape(-1).numpy()[live].view(np.uint64)
    s = rec["rec_side"].t().reshape(-1).numpy()[live]
    want = sum(int(S.quirk_flags(b, w, s, k, 8).sum()) for k in range(8))
    assert int(out["symmetry_quirk_rows"]) == want


def test_symmetries_random_is_a_function_of_the_seed():
    rec, _ = synthetic_records(G=6, seed=3)
    base = _train(rec, 8)
    every = _train(rec, 8, symmetries="all", augment=S.augment)
    n = base["states"].shape[0]
    a = _train(rec, 8, symmetries="random", symmetry_seed=11, augment=S.augment)
    b = _train(rec, 8, symmetries="random", symmetry_seed=11, augment=S.augment)
    c = _train(rec, 8, symmetries="random", symmetry_seed=12, augment=S.augment)
    assert set(a) == set(every)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["states"], c["states"])
    assert not torch.equal(a["policy_targets"], c["policy_targets"])
    # the draws are torch.randint's from a CPU generator seeded with symmetry_seed
    sym = torch.randint(0, 8, (n,), generator=torch.Generator().manual_seed(11))
    assert len(set(sym.tolist())) == 8
    at = 8 * torch.arange(n) + sym
    assert torch.equal(a["states"], every["states"][at])
    assert torch.equal(a["policy_targets"], every["policy_targets"][at])
    assert torch.equal(a["value_targets"], base["value_targets"])
    assert int(a["symmetry_rows"]) == n


def test_augmentation_runs_after_the_exact_replacements():
    """exact_policy and exact_endgame, with their injected host solvers, replace targets first;
    the symmetry acts on the replaced policy and repeats the replaced value."""
    import solve_moves_ref as V
    import solve_ref as R
    from test_solve_moves_cpu import synthetic_records as exact_records
    bs, N = 8, 5
    _, rec = exact_records(bs, N)
    kw = dict(exact_policy=N, moves_solver=V.host_moves_solver, exact_endgame=N,
              solver=R.host_solver)
    plain = _train(rec, bs)
    exact = _train(rec, bs, **kw)
    assert not torch.equal(exact["policy_targets"], plain["policy_targets"])
    assert not torch.equal(exact["value_targets"], plain["value_targets"])
    out = _train(rec, bs, symmetries="all", augment=S.augment, **kw)
    n = exact["states"].shape[0]
    for k in ("exact_rows", "exact_unsolved", "exact_policy_rows", "exact_policy_unsolved"):
        assert int(out[k]) == int(exact[k])                   # counts of records, not of images
    for k in range(8):
        assert np.array_equal(out["policy_targets"][k::8].numpy(),
                              S.image_policy(exact["policy_targets"].numpy(), k, bs))
        assert torch.equal(out["value_targets"][k::8], exact["value_targets"])
    assert int(out["symmetry_rows"]) == 8 * n
    # every image of a replaced row (uniform over proven-optimal moves; the other rows keep this
    # fixture's dense random targets) has its mass where its third plane is 1, or on the pass
    replaced = (exact["policy_targets"] != plain["policy_targets"]).any(dim=1)
    assert int(replaced.sum()) == int(exact["exact_policy_rows"]) > 0
    off_mask = (out["policy_targets"][:, :-1].reshape(-1, bs, bs) > 0) & (out["states"][:, 2] == 0)
    assert not bool(off_mask[replaced.repeat_interleave(8)].any())
