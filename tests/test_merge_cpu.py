"""Merging duplicate positions on the CPU (no GPU): the host reference's own self-checks
(tests/merge_ref.py), the argument checks of rvz_merge_positions / rvz_merge_scratch_size at the
C-ABI (they run before any HIP call), and records_to_training(merge_positions=True) with the NumPy
`merger` and the oracle's `canonical` injected."""
import numpy as np
import pytest
import torch

import merge_ref as M
from test_pipeline_cpu import synthetic_records
from test_solve_cpu import _train, played_records

EINVAL = -22


# ---------------------------------------------------------------- the reference itself
def test_reference_groups_by_hand():
    """Six rows: A, B, A as its colour-swapped twin, C, B, A. Groups in first-occurrence order."""
    A, B, C = (0x0F, 0xF0), (0x100, 0x200), (0x0F, 0xF000)     # (mover, opponent)
    black = np.array([A[0], B[0], A[1], C[1], B[0], A[0]], np.uint64)
    white = np.array([A[1], B[1], A[0], C[0], B[1], A[1]], np.uint64)
    side = np.array([1, 1, 2, 2, 1, 1], np.int32)
    pol = np.zeros((6, 65), np.float32)
    pol[np.arange(6), [0, 1, 2, 3, 4, 0]] = 1.0
    val = np.array([1, -1, 1, 0, 1, -1], np.float32)
    out = M.merge(black, white, side, pol, val)
    assert out["m"] == 3
    assert out["first"].tolist() == [0, 1, 3] and out["count"].tolist() == [3, 2, 1]
    assert out["group"].tolist() == [0, 1, 0, 2, 1, 0]
    want = np.zeros((3, 65), np.float32)
    want[0, 0], want[0, 2] = np.float32(2 / 3), np.float32(1 / 3)
    want[1, 1] = want[1, 4] = 0.5
    want[2, 3] = 1.0
    assert np.array_equal(out["policy"], want)
    assert np.array_equal(out["value"], np.array([1 / 3, 0, 0], np.float32))
    for k in ("first", "count", "group"):
        assert out[k].dtype == np.int32
    assert out["policy"].dtype == out["value"].dtype == np.float32


@pytest.mark.parametrize("bs", [8, 6])
def test_reference_is_the_identity_on_distinct_rows(bs):
    b, w, s, pol, val = M.distinct_rows(bs, 300)
    pol = pol.copy()
    pol[5, 7] = np.float32(1e-30)                  # q rounds to 0: a copy keeps it, a mean would not
    out = M.merge(b, w, s, pol, val, bs)
    assert out["m"] == 300 and np.array_equal(out["first"], np.arange(300))
    assert np.array_equal(out["group"], np.arange(300)) and (out["count"] == 1).all()
    assert out["policy"].tobytes() == pol.tobytes() and out["value"].tobytes() == val.tobytes()


def test_reference_means_of_outcomes():
    b = np.full(4, 0x1, np.uint64)
    w = np.full(4, 0x2, np.uint64)
    pol = np.full((4, 65), 1 / 65, np.float32)
    out = M.merge(b, w, np.ones(4, np.int32), pol, np.array([1, 1, -1, 1], np.float32))
    assert out["m"] == 1 and out["count"].tolist() == [4] and out["value"].tolist() == [0.5]
    assert np.array_equal(out["policy"][0], pol[0])         # the mean of equal entries is the entry
    out = M.merge(b[:3], w[:3], np.ones(3, np.int32), pol[:3], np.array([1, 0, 0], np.float32))
    assert out["value"][0] == np.float32(1 / 3)


def test_reference_malformed_rows():
    b, w, s, pol, val = M.distinct_rows(6, 8)
    b, w, s, pol, val = b.copy(), w.copy(), s.copy(), pol.copy(), val.copy()
    b[0] |= w[0] | np.uint64(1)
    w[0] |= np.uint64(1)                            # overlap
    b[1] |= np.uint64(1 << 36)                      # off the 6x6 board
    s[2] = 0
    pol[3, 4] = 1.5
    pol[4, 36] = np.nan
    val[5] = -2.0
    out = M.merge(b, w, s, pol, val, 6)
    assert out["group"].tolist() == [-1] * 6 + [0, 1] and out["m"] == 2
    assert out["first"].tolist() == [6, 7] and out["count"].tolist() == [1, 1]


@pytest.mark.parametrize("bs", [8, 6])
def test_mixed_rows_hold_duplicates_and_twins(bs):
    b, w, s, pol, val = M.mixed_rows(bs, 1023)
    out = M.merge(b, w, s, pol, val, bs)
    assert 100 < out["m"] < 1023 and out["count"].max() > 20 and (out["count"] == 1).any()
    both = {}
    for g, side in zip(out["group"], s):
        both.setdefault(int(g), set()).add(int(side))
    assert any(len(v) == 2 for v in both.values())           # a twin merged with its original
    assert (np.diff(out["first"]) > 0).all() and out["count"].sum() == 1023
    assert np.array_equal(out["group"][out["first"]], np.arange(out["m"]))


# ---------------------------------------------------------------- the C-ABI without a GPU
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """RVZ_EINVAL before any HIP call (the pointers are never dereferenced)."""
    import rvz
    lib = rvz.load()
    p = 0x10000
    good = [8, 100, p, p, p, p, p, 0, p, p, p, p, p, p, p, None]
    assert lib.rvz_merge_positions(8, 0, *[None] * 5, 0, *[None] * 8) == 0
    assert lib.rvz_merge_positions(6, 0, *[None] * 5, 0, *[None] * 8) == 0
    bad = [(0, 7), (0, 4), (1, -1), (1, 2 ** 31 // 65 + 1), (7, -1), (7, 6), (7, 31),
           (8, p + 8), (8, p + 4)]
    for k, v in bad:
        args = list(good)
        args[k] = v
        assert lib.rvz_merge_positions(*args) == EINVAL, (k, v)
    args = list(good)
    args[0], args[1] = 6, 2 ** 31 // 37 + 1
    assert lib.rvz_merge_positions(*args) == EINVAL
    for k in (2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14):
        args = list(good)
        args[k] = None
        assert lib.rvz_merge_positions(*args) == EINVAL, k
    # table_log2 must give more than n slots: 2^7 = 128 > 100 is the smallest that does
    assert lib.rvz_merge_scratch_size(8, 100, 6) < 0 and lib.rvz_merge_scratch_size(8, 100, 7) > 0
    assert lib.rvz_merge_scratch_size(8, 128, 7) < 0


def test_scratch_size():
    import rvz
    lib = rvz.load()
    for bs in (8, 6):
        np_ = bs * bs + 1
        sizes = [lib.rvz_merge_scratch_size(bs, n, 0) for n in
                 (0, 1, 2, 63, 64, 65, 1000, 4097, 70001, 2 ** 21, 2 ** 31 // np_ - 1)]
        assert all(s >= 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[1]
        for n in (1000, 70001, 2 ** 21):
            slots = 1 << (2 * n - 1).bit_length()
            size = lib.rvz_merge_scratch_size(bs, n, 0)
            assert size % 16 == 0 and size <= n * (8 * (np_ + 1) + 32) + 4 * slots + 4096
            assert lib.rvz_merge_scratch_size(bs, n, slots.bit_length()) > size   # twice the table
    for args in ((7, 10, 0), (8, -1, 0), (8, 10, -1), (8, 10, 3), (8, 10, 31),
                 (8, 2 ** 31 // 65 + 1, 0), (6, 2 ** 31 // 37 + 1, 0)):
        assert lib.rvz_merge_scratch_size(*args) < 0, args


def test_python_argument_errors():
    import rvz
    b = torch.zeros(4, dtype=torch.int64)
    st = torch.ones(4, 4, dtype=torch.int32)
    pol, val = torch.zeros(4, 65), torch.zeros(4)
    for call in (lambda: rvz.merge_positions(b, b, st, pol, val, 7),
                 lambda: rvz.merge_positions(b, b[:2], st, pol, val),
                 lambda: rvz.merge_positions(b.int(), b, st, pol, val),
                 lambda: rvz.merge_positions(b, b, st[:, :3], pol, val),
                 lambda: rvz.merge_positions(b, b, st, pol[:, :64], val),
                 lambda: rvz.merge_positions(b, b, st, pol.double(), val),
                 lambda: rvz.merge_positions(b, b, st, pol, val[:3]),
                 lambda: rvz.merge_positions(b, b, st, pol, val.double()),
                 lambda: rvz.merge_positions(b, b, st, pol, val, table_log2=2),
                 lambda: rvz.merge_positions(b, b, st, pol, val, table_log2=1.0),
                 lambda: rvz.merge_positions(b, b, st, pol, val)):        # host tensors
        with pytest.raises(rvz.RvzError):
            call()


# ---------------------------------------------------------------- records_to_training
def _keys(rec):
    """(mover, opponent) of the kept rows in records_to_training's order."""
    live = (rec["rec_idx"] >= 0).t().reshape(-1).numpy()
    b = rec["rec_black"].t().reshape(-1).numpy()[live].view(np.uint64)
    w = rec["rec_white"].t().reshape(-1).numpy()[live].view(np.uint64)
    s = rec["rec_side"].t().reshape(-1).numpy()[live]
    return [(int(x), int(y)) if z == 1 else (int(y), int(x)) for x, y, z in zip(b, w, s)]


def _with_copy_of_game(rec, g, rng):
    """rec with game g's column appended once more, under fresh policies and the opposite result:
    every kept row of that column is a planted duplicate."""
    out = {k: torch.cat([v, v[:, g:g + 1]], dim=1) for k, v in rec.items() if k != "final_status"}
    p = rng.random(out["rec_p"][:, -1].shape)
    out["rec_p"][:, -1] = torch.from_numpy(p / p.sum(axis=1, keepdims=True))
    final = rec["final_status"][g:g + 1].clone()
    final[0, 2] = 3 - final[0, 2] if int(final[0, 2]) in (1, 2) else 1
    out["final_status"] = torch.cat([rec["final_status"], final])
    return out


def test_merge_off_is_byte_identical():
    rec, _ = synthetic_records(G=6, seed=3)
    calls = []

    def merger(*a):
        calls.append(a)
        return M.host_merger(*a)

    base = _train(rec, 8)
    off = _train(rec, 8, merge_positions=False, merger=merger)
    assert not calls and list(off) == list(base) == ["states", "policy_targets", "value_targets"]
    for k in base:
        assert off[k].dtype == base[k].dtype and off[k].shape == base[k].shape
        assert off[k].numpy().tobytes() == base[k].numpy().tobytes(), k


def test_merge_collapses_groups_in_first_occurrence_order():
    rec, _ = synthetic_records(G=6, seed=3)
    g = next(g for g in range(6) if int(rec["final_status"][g, 2]) in (1, 2))   # a decided game
    planted = int((rec["rec_idx"][:, g] >= 0).sum())
    rec2 = _with_copy_of_game(rec, g, np.random.default_rng(0))
    base = _train(rec2, 8)
    canon_rows = []

    def canonical(b, w, st, bs):
        from test_solve_cpu import _oracle_canonical
        canon_rows.append(b.numel())
        return _oracle_canonical(b, w, st, bs)

    from rvz.trainer import records_to_training
    out = records_to_training(rec2["rec_black"], rec2["rec_white"], rec2["rec_side"],
                              rec2["rec_idx"], rec2["rec_p"], rec2["final_status"], 8,
                              canonical=canonical, merge_positions=True, merger=M.host_merger)
    keys = _keys(rec2)
    n = len(keys)
    order = list(dict.fromkeys(keys))                         # distinct, first occurrence first
    m = len(order)
    assert list(out) == ["states", "policy_targets", "value_targets", "position_counts",
                         "merge_rows", "merge_input_rows"]
    assert canon_rows == [m]                                  # the merged rows only
    for k in ("merge_rows", "merge_input_rows"):
        assert out[k].dim() == 0 and out[k].dtype == torch.int64
    assert int(out["merge_input_rows"]) == n == base["states"].shape[0]
    assert int(out["merge_rows"]) == m == out["states"].shape[0]
    # the duplicates: the start position of every game, early transpositions, and the planted
    # copy, each of whose rows repeats a row of game g
    natural = _keys(rec)
    assert n - m == (len(natural) - len(set(natural))) + planted and planted > 30
    first = [keys.index(k) for k in order]
    assert torch.equal(out["states"], base["states"][first])
    assert out["states"].dtype == torch.float32 and out["policy_targets"].dtype == torch.float32
    assert out["value_targets"].shape == (m, 1) and out["value_targets"].dtype == torch.float32
    counts = [keys.count(k) for k in order]
    assert out["position_counts"].dtype == torch.int32
    assert out["position_counts"].tolist() == counts and counts[0] == 7   # the start position
    for j in (0, 1, m - 1):
        rows = [i for i, k in enumerate(keys) if k == order[j]]
        q = np.rint(base["policy_targets"][rows].numpy().astype(np.float64) * 2.0 ** 36)
        want = (q.sum(axis=0) / (len(rows) * 2.0 ** 36)).astype(np.float32)
        if len(rows) == 1:
            want = base["policy_targets"][rows[0]].numpy()
        assert np.array_equal(out["policy_targets"][j].numpy(), want)
    # game g and its copy end with opposite winners: their shared last row averages to 0
    late = sum(int((rec["rec_idx"][:, k] >= 0).sum()) for k in range(g + 1)) - 1
    assert keys.count(keys[late]) == 2
    assert float(out["value_targets"][order.index(keys[late])]) == 0.0
    assert abs(float(base["value_targets"][late])) == 1.0


def test_exact_value_targets_survive_merging():
    import solve_ref as R
    bs, N = 8, 5
    rec = _with_copy_of_game(played_records(range(4), bs), 1, np.random.default_rng(1))
    kw = dict(exact_endgame=N, solver=R.host_solver)
    exact = _train(rec, bs, **kw)
    out = _train(rec, bs, merge_positions=True, merger=M.host_merger, **kw)
    assert int(out["exact_rows"]) == int(exact["exact_rows"]) > 0   # counted before merging
    keys = _keys(rec)
    order = list(dict.fromkeys(keys))
    empties = 64 - exact["states"][:, :2].sum(dim=(1, 2, 3))
    checked = merged_late = 0
    for i, k in enumerate(keys):
        if empties[i] <= N:
            j = order.index(k)
            assert out["value_targets"][j, 0] == exact["value_targets"][i, 0]
            checked += 1
            merged_late += int(out["position_counts"][j]) > 1
    assert checked == int(exact["exact_rows"]) and merged_late >= 2


def test_merging_runs_before_symmetries():
    import symmetry_ref as S
    rec, _ = synthetic_records(G=5, seed=4)
    merged = _train(rec, 8, merge_positions=True, merger=M.host_merger)
    out = _train(rec, 8, merge_positions=True, merger=M.host_merger, symmetries="all",
                 augment=S.augment)
    m = merged["states"].shape[0]
    assert set(out) == set(merged) | {"symmetry_rows", "symmetry_quirk_rows"}
    for k in ("states", "policy_targets", "value_targets", "position_counts"):
        assert out[k].shape[0] == 8 * m
        assert out[k][::8].numpy().tobytes() == merged[k].numpy().tobytes(), k
    assert torch.equal(out["position_counts"].reshape(m, 8),
                       merged["position_counts"].unsqueeze(1).expand(m, 8))
    assert int(out["symmetry_rows"]) == 8 * m and int(out["merge_rows"]) == m
    for k in range(8):
        assert np.array_equal(out["policy_targets"][k::8].numpy(),
                              S.image_policy(merged["policy_targets"].numpy(), k, 8))
    rnd = _train(rec, 8, merge_positions=True, merger=M.host_merger, symmetries="random",
                 symmetry_seed=3, augment=S.augment)
    assert rnd["states"].shape[0] == m and torch.equal(rnd["position_counts"],
                                                       merged["position_counts"])
