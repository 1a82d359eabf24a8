"""Continuous self-play records without a GPU: the Python restatement of rvz_records_games
(tests/records_games_ref.py) checked against records_to_training on whole lockstep games, the
properties the GPU tests lean on (the carry equivalence, the edge cases' presence), and the
wrappers: games_to_training through the injected solvers and merger, the argument rules of
rvz.records_games, SelfPlayRunner(carry_plies=...) and SelfPlayTrainer(continuous_plies=...), and
the C entry point's refusals, which come before any HIP call."""
import numpy as np
import pytest
import torch

import merge_ref as M
import records_games_ref as RG
import solve_moves_ref as V
import solve_ref as R
from test_solve_cpu import _oracle_canonical, _train, played_records

EINVAL = -22


def _rows_dict(ref, pad=3):
    """The reference's rows as rvz.records_games returns them: tensors at a length above m, the
    rows from m on holding bytes nobody may read."""
    m = ref["m"]
    def grow(a, fill):
        tail = np.full((pad,) + a.shape[1:], fill, a.dtype)
        return torch.from_numpy(np.concatenate([a, tail]))
    return {"m": torch.tensor(m, dtype=torch.int32),
            "mover": grow(ref["mover"].view(np.int64), -1),
            "opponent": grow(ref["opponent"].view(np.int64), -1),
            "policy": grow(ref["policy"], np.nan), "value": grow(ref["value"], np.nan),
            "src": grow(ref["src"], -1), "stats": torch.from_numpy(ref["stats"])}


# ---------------------------------------------------------------- the reference itself
def test_reference_equals_records_to_training_on_lockstep_games(oracle):
    """Whole games from the start, no reset, emit_from = 0: the reference's rows are
    records_to_training(compact=True)'s, bit for bit."""
    rec = played_records(range(20, 31), 6)
    ref = RG.games(oracle, 6, rec["rec_black"].numpy().view(np.uint64),
                   rec["rec_white"].numpy().view(np.uint64), rec["rec_side"].numpy(),
                   rec["rec_idx"].numpy(), rec["rec_p"].numpy(), 0)
    want = _train(rec, 6, compact=True)
    n = want["mover"].numel()
    assert ref["m"] == n > 11 * 20
    assert np.array_equal(ref["mover"].view(np.int64), want["mover"].numpy())
    assert np.array_equal(ref["opponent"].view(np.int64), want["opponent"].numpy())
    assert ref["policy"].tobytes() == want["policy_targets"].numpy().tobytes()
    assert ref["value"].tobytes() == want["value_targets"].numpy().reshape(-1).tobytes()
    idx = rec["rec_idx"].numpy()
    assert np.array_equal(ref["state"], np.where(idx >= 0, 1, -1))
    assert ref["stats"].tolist() == [n, 11, 0, 0, 0, 0, 0, 0]
    assert set(ref["value"].tolist()) >= {1.0, -1.0}


def carry_case(O, bs=6, G=9, K=14, seed=5):
    """The carry equivalence's inputs: one long window [0, C + 2K) and what the two short
    windows and the whole one emit, per slot, as lists of (absolute ply, slot). The slots open
    at different move numbers, as in steady play, so games end all over the window."""
    C = bs * bs - 4
    win = RG.window(O, bs, C + 2 * K, G, seed, offsets={g: 7 * g % 30 for g in range(G)})
    cut = lambda lo, hi: tuple(a[lo:hi] for a in win)
    first = RG.games(O, bs, *cut(0, C + K), C)
    second = RG.games(O, bs, *cut(K, C + 2 * K), C)
    whole = RG.games(O, bs, *win, C)
    return win, C, K, first, second, whole


def carried_rows(first, second, K, G):
    """Both short windows' rows as (absolute ply, slot), slot-major."""
    both = [divmod(int(s), G) for s in first["src"]] + \
           [(q + K, g) for q, g in (divmod(int(s), G) for s in second["src"])]
    return sorted(both, key=lambda r: (r[1], r[0]))


def test_reference_carry_equivalence(oracle):
    """Two windows of K new plies behind a carry of C = S*S - 4 emit together exactly what the
    whole window emits from ply C on: no game twice, none lost."""
    win, C, K, first, second, whole = carry_case(oracle)
    G = win[3].shape[1]
    want = [divmod(int(s), G) for s in whole["src"]]
    got = carried_rows(first, second, K, G)
    assert len(got) == len(set(got)) and got == want and len(want) > 4 * G
    assert first["stats"][1] + second["stats"][1] == whole["stats"][1]
    # the second window meets the first's games again and does not emit them
    assert second["stats"][6] > 0 and first["m"] > 0 and second["m"] > 0


def test_reference_edge_cases(oracle):
    """The cases of the GPU tests exist in the windows they use."""
    win = RG.edge_window(oracle, 6, 40, 65, 7)
    ref = RG.games(oracle, 6, *win, 0)
    state, side, idx = ref["state"], win[2], win[3]
    assert ref["stats"][5] >= 2 and (state[:5, 3] == 1).all()        # headless games emitted
    assert (state[[6, 7, 20], 4] == -1).all() and state[5, 4] == state[8, 4] == 1
    assert state[39, 11] == -1
    passes = np.argwhere(idx == 36)                                  # the pass-index records
    assert len(passes) >= 2 and ref["stats"][4] == 0                 # the rules accept them
    for p, g in passes:                                              # each opens a headless segment
        assert state[p, g] in (0, 1) and state[p - 1, g] == 3 and side[p, g] != side[p - 1, g]
    assert (state[passes[:, 0], passes[:, 1]] == 1).any()            # and one such game is emitted
    same = (side[1:] == side[:-1]) & (state[1:] == 1) & (state[:-1] == 1)
    assert same.any()                                                # an auto-pass inside a game
    assert (ref["value"] == 0).any()                                 # a drawn game
    assert ref["stats"][2] > 0                                       # and games still open


# ---------------------------------------------------------------- games_to_training
def test_games_to_training_is_the_tail_of_records_to_training():
    """The rows of whole games through games_to_training equal records_to_training's outputs
    under every option of the tail, key for key."""
    from rvz.trainer import games_to_training
    from test_solve_moves_cpu import synthetic_records as exact_records
    _, rec = exact_records(8, 5)
    base = _train(rec, 8, compact=True)
    n = base["mover"].numel()
    rows = _rows_dict({"m": n, "mover": base["mover"].numpy().view(np.uint64),
                       "opponent": base["opponent"].numpy().view(np.uint64),
                       "policy": base["policy_targets"].numpy(),
                       "value": base["value_targets"].numpy().reshape(-1),
                       "src": np.arange(n, dtype=np.int32), "stats": np.zeros(8, np.int64)})
    exact = dict(exact_policy=5, moves_solver=V.host_moves_solver, exact_endgame=5,
                 solver=R.host_solver)
    merge = dict(merge_positions=True, merger=M.host_merger)
    for kw in ({}, exact, merge, {**exact, **merge}):
        want = _train(rec, 8, compact=True, **kw)
        got = games_to_training(rows, 8, **kw)
        assert list(got) == list(want), kw
        for k in want:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (k, kw)
        full = _train(rec, 8, **kw)
        planes = games_to_training(rows, 8, canonical=_oracle_canonical, compact=False, **kw)
        assert list(planes) == list(full), kw
        for k in full:
            assert torch.equal(planes[k], full[k]), (k, kw)
    changed = games_to_training(rows, 8, **exact)
    assert not torch.equal(changed["policy_targets"], base["policy_targets"])
    assert int(changed["exact_rows"]) > 0
    # m = 0: no rows, the same keys
    none = games_to_training(dict(rows, m=0), 8, **merge)
    assert none["mover"].shape == (0,) and none["policy_targets"].shape == (0, 65)
    assert none["value_targets"].shape == (0, 1) and int(none["merge_rows"]) == 0
    for bad in ("all", "random"):
        with pytest.raises(ValueError):
            games_to_training(rows, 8, symmetries=bad)
    with pytest.raises(ValueError):
        games_to_training(rows, 8, symmetries="some", compact=False)


# ---------------------------------------------------------------- the argument rules
def _window_tensors(oracle, bs=6, P=8, G=3):
    return RG.tensors(*RG.window(oracle, bs, P, G, 1))


def test_records_games_refuses_bad_arguments(oracle):
    """Every rule raises RvzError, its message naming the function, before any device call: a
    good call on these CPU tensors gets as far as the device check."""
    import rvz
    b, w, s, i, p = _window_tensors(oracle)
    with pytest.raises(rvz.RvzError) as err:
        rvz.records_games(b, w, s, i, p, 6)
    assert "device tensors" in str(err.value)
    bad = [dict(board_size=7), dict(emit_from=9), dict(emit_from=-1), dict(emit_from=True),
           dict(emit_from=1.0), dict(rec_black=b.to(torch.int32)), dict(rec_white=w[:, :2]),
           dict(rec_side=s.double()), dict(rec_idx=i.reshape(-1)), dict(rec_idx=i != 0),
           dict(rec_p=p.float()), dict(rec_p=p[:, :, :36]), dict(rec_p=p[:7]),
           dict(rec_black=None)]
    for mut in bad:
        kw = dict(rec_black=b, rec_white=w, rec_side=s, rec_idx=i, rec_p=p, board_size=6,
                  emit_from=0)
        kw.update(mut)
        with pytest.raises(rvz.RvzError) as err:
            rvz.records_games(**kw)
        assert str(err.value).startswith("records_games:"), (mut.keys(), str(err.value))
    # a window without records: no launch, no rows
    out = rvz.records_games(b[:0], w[:0], s[:0], i[:0], p[:0], 6, state=True)
    assert int(out["m"]) == 0 and out["state"].shape == (0, 3) and out["policy"].shape == (0, 37)
    assert out["stats"].tolist() == [0] * 8 and "state" not in rvz.records_games(
        b[:0], w[:0], s[:0], i[:0], p[:0], 6)


def check_entry_point_refusals(lib):
    """RVZ_EINVAL before any HIP call (the pointers are never dereferenced), and the scratch
    size's rules."""
    q = 0x10000
    #       bs  P  G  black white side idx p  emit scratch m  mover opp pol val src state stats
    good = [8, 70, 65, q, q, q, q, q, 60, q, q, q, q, q, q, q, None, q, None]
    for k, v in ((0, 7), (0, 4), (1, 0), (1, -1), (2, 0), (2, -5), (8, -1), (8, 71),
                 (1, 2 ** 31 // (65 * 65) + 1), (2, 2 ** 31 // (65 * 70) + 1),
                 (9, q + 4), (9, q + 8)):
        args = list(good)
        args[k] = v
        assert lib.rvz_records_games(*args) == EINVAL, (k, v)
    args = list(good)
    args[0], args[1], args[2] = 6, 2 ** 16, 2 ** 31 // (37 * 2 ** 16) + 1
    assert lib.rvz_records_games(*args) == EINVAL                 # 6x6: * 37 reaches 2^31
    for k in (3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 17):      # out_state (16) may be null
        bad = list(good)
        bad[k] = None
        assert lib.rvz_records_games(*bad) == EINVAL, k
    size = lib.rvz_records_scratch_size
    for bad in ((0, 4), (4, 0), (-1, 4), (4, -1), (2 ** 16, 2 ** 31 // (37 * 2 ** 16) + 1)):
        assert size(*bad) < 0, bad
    assert size(1, 1) > 0 and size(1, 1) % 16 == 0
    for P in (1, 2, 39, 40, 120):
        for G in (1, 2, 63, 64, 65, 4096):
            assert 8 * P * G <= size(P, G) <= size(P + 1, G) and size(P, G) <= size(P, G + 1)


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    import rvz
    check_entry_point_refusals(rvz.load())


def test_runner_carry_plies_rules():
    """carry_plies is checked before the runner touches its engine."""
    from rvz.selfplay import SelfPlayRunner
    for kw, says in ((dict(carry_plies=-1), "carry_plies"), (dict(carry_plies=True), "carry_plies"),
                     (dict(carry_plies=2.0), "carry_plies"),
                     (dict(carry_plies=32, fused=False, record=True), "fused"),
                     (dict(carry_plies=32, fused=True, record=False), "record"),
                     # the default keeps today's refusal
                     (dict(fused=True, record=True, autoreset=True), "no autoreset"),
                     (dict(carry_plies=0, fused=True, record=True, autoreset=True),
                      "no autoreset")):
        with pytest.raises(ValueError) as err:
            SelfPlayRunner(None, None, **kw)
        assert says in str(err.value), (kw, str(err.value))
    # with a carry the same runner passes every rule and only then reaches for its engine
    with pytest.raises(AttributeError):
        SelfPlayRunner(None, None, fused=True, record=True, autoreset=True, carry_plies=32)


def test_trainer_continuous_plies_rules():
    from rvz.network import AlphaZeroNetwork
    from rvz.pipeline import SelfPlayTrainer
    net = AlphaZeroNetwork(6, 1, 16)
    for kw, says in ((dict(continuous_plies=24), "replay_iterations"),
                     (dict(continuous_plies=0, replay_iterations=2), "continuous_plies"),
                     (dict(continuous_plies=True, replay_iterations=2), "continuous_plies"),
                     (dict(continuous_plies=24.0, replay_iterations=2), "continuous_plies"),
                     (dict(continuous_plies=24, replay_iterations=2, fused=False), "fused"),
                     (dict(continuous_plies=24, replay_iterations=2, adjudicate_empties=4),
                      "adjudicate_empties"),
                     (dict(continuous_plies=24, replay_iterations=2, symmetries="random"),
                      "symmetries")):
        with pytest.raises(ValueError) as err:
            SelfPlayTrainer(net, games=4, **kw)
        assert says in str(err.value), (kw, str(err.value))
