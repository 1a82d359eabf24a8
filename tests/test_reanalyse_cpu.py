"""Replay reanalysis without a GPU: the argument checks of rvz_replay_stale / rvz_replay_roots /
rvz_replay_refresh (RVZ_EINVAL before any HIP call), their scratch sizes, the NumPy restatement
(tests/reanalyse_ref.py) against a brute-force selection, the Python wrappers' refusals, and
ReplayBuffer's stamps."""
import numpy as np
import pytest
import torch

import reanalyse_ref as R

EINVAL = -22
P = 0x10000                      # a pointer that is never dereferenced


def test_stale_refuses_bad_arguments_without_a_gpu():
    import rvz
    lib = rvz.load()
    size = lib.rvz_replay_stale_scratch_size(7, 2)
    #       cap stamp start live n lo below scratch bytes out_slot out_count stream
    good = [7, P, 5, 3, 4, 0, 2, P, size, P, P, None]
    bad = [(0, 0), (0, -1), (2, -1), (2, 7), (3, 0), (3, 8), (3, -1), (4, -1), (5, -1), (6, 0),
           (5, 2), (5, 3), (6, 65537), (1, None), (7, None), (7, P + 8), (7, P + 4),
           (8, size - 1), (8, 0), (9, None), (10, None)]
    for k, v in bad:
        args = list(good)
        args[k] = v
        assert lib.rvz_replay_stale(*args) == EINVAL, (k, v)
    args = list(good)
    args[5], args[6], args[8] = 10, 10 + 65537, 2 ** 40
    assert lib.rvz_replay_stale(*args) == EINVAL
    args[6] = 2 ** 31 - 1                        # lo = 10: more than 65536 classes
    assert lib.rvz_replay_stale(*args) == EINVAL
    # n = 0: nothing to do, whatever the pointers; the geometry and the request still count
    zero = [7, None, 5, 3, 0, 0, 2, None, 0, None, None, None]
    assert lib.rvz_replay_stale(*zero) == 0
    for k, v in ((0, 0), (2, 7), (3, 0), (3, 8), (5, -1), (6, 0)):
        args = list(zero)
        args[k] = v
        assert lib.rvz_replay_stale(*args) == EINVAL, (k, v)


def test_roots_refuses_bad_arguments_without_a_gpu():
    import rvz
    lib = rvz.load()
    #       bs cap mover opponent n slot black white status bad stream
    good = [8, 7, P, P, 3, P, P, P, P, P, None]
    for k, v in ((0, 7), (0, 4), (1, 0), (1, -1), (4, -1), (4, 2 ** 30 + 1), (8, P + 8), (8, P + 4)):
        args = list(good)
        args[k] = v
        assert lib.rvz_replay_roots(*args) == EINVAL, (k, v)
    for k in (2, 3, 5, 6, 7, 8, 9):
        args = list(good)
        args[k] = None
        assert lib.rvz_replay_roots(*args) == EINVAL, k
    for bs in (8, 6):
        assert lib.rvz_replay_roots(bs, 7, None, None, 0, None, None, None, None, None, None) == 0
    assert lib.rvz_replay_roots(7, 7, None, None, 0, None, None, None, None, None, None) == EINVAL
    assert lib.rvz_replay_roots(8, 0, None, None, 0, None, None, None, None, None, None) == EINVAL


def test_refresh_refuses_bad_arguments_without_a_gpu():
    import rvz
    lib = rvz.load()
    size = lib.rvz_replay_refresh_scratch_size(5)
    #       bs cap policy stamp n slot p idx new_stamp scratch bytes counts stream
    good = [8, 7, P, P, 5, P, P, P, 3, P, size, P, None]
    for k, v in ((0, 7), (0, 4), (1, 0), (1, -1), (4, -1), (4, 2 ** 30 + 1), (8, -1),
                 (9, P + 8), (9, P + 4), (10, size - 1), (10, 0)):
        args = list(good)
        args[k] = v
        assert lib.rvz_replay_refresh(*args) == EINVAL, (k, v)
    for k in (2, 3, 5, 6, 7, 9, 11):
        args = list(good)
        args[k] = None
        assert lib.rvz_replay_refresh(*args) == EINVAL, k
    zero = [6, 7, None, None, 0, None, None, None, 0, None, 0, None, None]
    assert lib.rvz_replay_refresh(*zero) == 0
    for k, v in ((0, 5), (1, 0), (8, -1)):
        args = list(zero)
        args[k] = v
        assert lib.rvz_replay_refresh(*args) == EINVAL, (k, v)


def test_scratch_sizes_are_monotone():
    import rvz
    lib = rvz.load()
    caps = (1, 2, 1023, 1024, 1025, 3072, 3073, 2 ** 21, 2 ** 31 - 1)
    classes = (1, 2, 3, 4, 5, 64, 65, 4096, 65535, 65536)
    grid = [[lib.rvz_replay_stale_scratch_size(c, k) for k in classes] for c in caps]
    for row in grid:
        assert row == sorted(row) and all(s > 0 and s % 16 == 0 for s in row)
    for col in zip(*grid):
        assert list(col) == sorted(col)
    # the header, a word per class, a pair of words per tile of 1,024 rows
    assert grid[0][0] >= 16 + 4 + 8 and grid[4][0] >= 16 + 4 + 2 * 8
    assert grid[-1][-1] < 2 ** 25
    for cap, k in ((0, 1), (-1, 1), (7, 0), (7, -1), (7, 65537)):
        assert lib.rvz_replay_stale_scratch_size(cap, k) < 0, (cap, k)
    ns = (0, 1, 31, 32, 33, 64, 65, 4096, 32768, 2 ** 30)
    sizes = [lib.rvz_replay_refresh_scratch_size(n) for n in ns]
    assert sizes == sorted(sizes) and all(s >= 4 * n + 8 * 2 * n and s % 16 == 0
                                          for s, n in zip(sizes, ns))
    assert sizes[0] == 8 * 64
    assert lib.rvz_replay_refresh_scratch_size(-1) < 0
    assert lib.rvz_replay_refresh_scratch_size(2 ** 30 + 1) < 0


def _brute(stamp, start, live, n, lo, below):
    """The selection by counting, with no sort: how many rows each class may still give is
    settled class by class, then one walk over the rows in order takes them."""
    cap = len(stamp)
    held = [int(stamp[(start + i) % cap]) for i in range(live)]
    quota, left = {}, n
    for c in range(below - lo):
        members = sum(1 for s in held if 0 <= s < below and (s - lo if s > lo else 0) == c)
        quota[c] = min(members, left)
        left -= quota[c]
    slots = []
    for i, s in enumerate(held):
        if not 0 <= s < below:
            continue
        c = s - lo if s > lo else 0
        if quota[c]:
            quota[c] -= 1
            slots.append((start + i) % cap)
    return slots + [-1] * (n - len(slots)), len(slots)


def test_restatement_agrees_with_a_sorted_selection():
    rng = np.random.default_rng(5)
    for trial in range(200):
        cap = int(rng.integers(1, 40))
        live = int(rng.integers(1, cap + 1))
        start = int(rng.integers(0, cap))
        lo = int(rng.integers(0, 4))
        below = lo + int(rng.integers(1, 5))
        n = int(rng.integers(0, cap + 3))
        stamp = rng.integers(-1, below + 2, cap).astype(np.int32)
        got, count = R.stale(stamp, start, live, n, lo, below)
        want, k = _brute(stamp, start, live, n, lo, below)
        assert got.tolist() == want and count[0] == k, trial
        held = [int(stamp[(start + i) % cap]) for i in range(live)]
        assert count[1] == sum(s < 0 for s in held), trial
        # the classes taken are the smallest: none left behind is below one that was taken
        taken = set(got[:k].tolist())
        cls = lambda s: max(int(stamp[s]) - lo, 0)               # noqa: E731
        left = [cls((start + i) % cap) for i in range(live)
                if (start + i) % cap not in taken and 0 <= held[i] < below]
        assert not taken or not left or max(cls(s) for s in taken) <= min(left), trial
    # every stamp at or below lo shares class 0: the older row wins, whatever its stamp
    got, count = R.stale(np.array([3, 0, 2, 1, 5], np.int32), 0, 5, 2, 3, 5)
    assert got.tolist() == [0, 1] and count.tolist() == [2, 0]
    got, count = R.stale(np.array([4, 3, 4, 3, -7], np.int32), 3, 5, 3, 3, 5)
    assert got.tolist() == [3, 0, 1] and count.tolist() == [3, 1]  # rows 3, 4(-7), 0, 1, 2


def test_restatement_of_roots_and_refresh():
    mover = np.array([1, 2, 4, 1 << 40], np.uint64)
    opponent = np.array([2, 2, 8, 1], np.uint64)
    b, w, st, bad = R.roots(mover, opponent, [0, -1, 1, 4, -2, 2, 3], 6)
    assert b.tolist() == [1, 0, 0, 0, 0, 4, 0] and w.tolist() == [2, 0, 0, 0, 0, 8, 0]
    assert st.tolist() == [list(R.LIVE_ROW)] + [list(R.OVER_ROW)] * 4 + [list(R.LIVE_ROW),
                                                                        list(R.OVER_ROW)]
    assert bad.tolist() == [4]                   # overlap, slot 4, slot -2, a bit off the 6x6 board
    assert R.roots(mover, opponent, [3], 8)[3].tolist() == [0]
    assert R.row_sum(np.full(65, 1 / 65)) == pytest.approx(1.0, abs=1e-12)
    assert R.row_sum(np.arange(37.0)) == 36 * 37 / 2
    pol = np.zeros((3, 37), np.float32)
    p = np.zeros((5, 37))
    p[:, 0] = 1.0
    p[1, :2] = 0.5
    p[3, 1] = 1e-8                               # the sum is off
    p[4, :2] = (1.5, -0.5)                       # a negative entry
    got, stamp, counts = R.refresh(pol, [7, 8, 9], [2, 2, -1, 0, 1], p, [0, 0, 0, 0, 0], 4)
    assert got[2, :2].tolist() == [0.5, 0.5] and stamp.tolist() == [7, 8, 4]
    assert not got[:2].any() and counts.tolist() == [1, 3]


def test_wrappers_refuse_before_any_device_call():
    import rvz
    stamp = torch.zeros(7, dtype=torch.int32)
    good = dict(stamp=stamp, start=5, live=3, n=0, lo=0, below=2)
    slot, count = rvz.replay_stale(**good)       # n = 0: nothing launches, CPU tensors will do
    assert slot.shape == (0,) and slot.dtype == torch.int32 and count.tolist() == [0, 0]
    for mut in (dict(stamp=stamp.long()), dict(stamp=stamp.reshape(7, 1)),
                dict(stamp=torch.zeros(14, dtype=torch.int32)[::2]), dict(start=7),
                dict(start=True), dict(live=0), dict(live=8), dict(n=-1), dict(n=1.0),
                dict(lo=-1), dict(below=0), dict(lo=2), dict(below=65537), dict(below=2.0)):
        with pytest.raises(rvz.RvzError) as err:
            rvz.replay_stale(**{**good, **mut})
        assert str(err.value).startswith("replay_stale:"), str(err.value)
    i64 = lambda n: torch.zeros(n, dtype=torch.int64)           # noqa: E731
    none = torch.zeros(0, dtype=torch.int32)
    for bs in (8, 6):
        b, w, st, bad = rvz.replay_roots(i64(7), i64(7), none, bs)
        assert b.shape == w.shape == (0,) and st.shape == (0, 4) and bad.tolist() == [0]
        assert b.dtype == torch.int64 and st.dtype == torch.int32
    for mut in (dict(mover=i64(7).int()), dict(opponent=i64(8)), dict(slot=torch.zeros(0)),
                dict(slot=torch.zeros(0, 1, dtype=torch.int32)), dict(mover=i64(0),
                                                                      opponent=i64(0))):
        with pytest.raises(rvz.RvzError) as err:
            rvz.replay_roots(**{**dict(mover=i64(7), opponent=i64(7), slot=none, board_size=8),
                                **mut})
        assert str(err.value).startswith("replay_roots:"), str(err.value)
    with pytest.raises(rvz.RvzError):
        rvz.replay_roots(i64(7), i64(7), none, 7)
    good = dict(policy=torch.zeros(7, 65), stamp=stamp, slot=none, p=torch.zeros(0, 65,
                dtype=torch.float64), idx=none, new_stamp=3)
    assert rvz.replay_refresh(**good).tolist() == [0, 0]
    assert rvz.replay_refresh(**{**good, "policy": torch.zeros(7, 37),
                                 "p": torch.zeros(0, 37, dtype=torch.float64)}).tolist() == [0, 0]
    for mut in (dict(policy=torch.zeros(7, 64)), dict(policy=torch.zeros(7, 65).double()),
                dict(stamp=stamp.long()), dict(stamp=torch.zeros(8, dtype=torch.int32)),
                dict(p=torch.zeros(0, 65)), dict(p=torch.zeros(0, 37, dtype=torch.float64)),
                dict(slot=torch.zeros(1, dtype=torch.int32)), dict(idx=torch.zeros(0)),
                dict(new_stamp=-1), dict(new_stamp=2 ** 31), dict(new_stamp=1.0)):
        with pytest.raises(rvz.RvzError) as err:
            rvz.replay_refresh(**{**good, **mut})
        assert str(err.value).startswith("replay_refresh:"), str(err.value)


def _rows(n, bs=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    npol = bs * bs + 1
    pol = torch.rand(n, npol, generator=g)
    return (torch.arange(n, dtype=torch.int64) + 1, torch.arange(n, dtype=torch.int64) << 8,
            pol / pol.sum(1, keepdim=True), torch.ones(n))


def test_buffer_without_stamps_is_the_buffer_of_before():
    import rvz
    buf = rvz.ReplayBuffer(8, 8, "cpu")
    assert not hasattr(buf, "stamp") and buf.stamps is False
    buf.append(*_rows(3), iteration=0)
    with pytest.raises(ValueError, match="stamps=True"):
        buf.append(*_rows(3), iteration=0, stamp=0)
    with pytest.raises(ValueError, match="stamps=True"):
        buf.reanalyse(None, None, 4, 0, 1, 2)
    # the attributes of the buffer of before, and the flag
    assert set(vars(buf)) == {"capacity", "board_size", "window_iterations", "device", "batcher",
                              "prioritized", "weighted", "mover", "opponent", "policy", "value",
                              "start", "_live", "_ledger", "stamps"}


def test_buffer_stamps_follow_the_rows():
    import rvz
    buf = rvz.ReplayBuffer(8, 8, "cpu", stamps=True)
    assert buf.stamp.dtype == torch.int32 and buf.stamp.shape == (8,)
    buf.append(*_rows(5), iteration=0)
    buf.append(*_rows(2), iteration=1)
    buf.append(*_rows(3), iteration=2, stamp=7)                 # wraps: slots 7, 0, 1
    assert buf.stamp.tolist() == [7, 7, 0, 0, 0, 1, 1, 7] and buf.start == 2 and len(buf) == 8
    for bad in (True, 1.0, -1, 2 ** 31):
        with pytest.raises(ValueError, match="stamp"):
            buf.append(*_rows(1), iteration=2, stamp=bad)

    class _Engine:
        board_size, n_games, memo_on = 8, 4, False
    for name, value in (("noise", (0.3, 0.25, 0)), ("pool", (5, 0)), ("schedule", (10, 0.0))):
        eng = _Engine()
        setattr(eng, name, value)
        with pytest.raises(ValueError, match="reanalyse"):
            buf.reanalyse(eng, None, 4, 0, 1, 2)
    eng = _Engine()
    eng.board_size = 6
    with pytest.raises(ValueError, match="6x6"):
        buf.reanalyse(eng, None, 4, 0, 1, 2)
    with pytest.raises(ValueError, match="below"):
        buf.reanalyse(_Engine(), None, 4, 3, 3, 5)
    out = buf.reanalyse(_Engine(), None, 0, 0, 1, 2)            # no rows asked for: nothing runs
    assert out["slot"].shape == (0,) and out["counts"].tolist() == [0, 0]
    for bad in (-1, 9, True, 1.0):
        with pytest.raises(ValueError, match="first"):
            buf.reanalyse(_Engine(), None, 4, 0, 1, 2, first=bad)
    out = buf.reanalyse(_Engine(), None, 4, 0, 1, 2, first=8)   # every held row left out
    assert out["slot"].tolist() == [-1] * 4 and out["counts"].tolist() == [0, 0]


def test_rows_leaving_are_the_rows_the_next_append_drops():
    import rvz
    buf = rvz.ReplayBuffer(32, 8, "cpu", window_iterations=3, stamps=True)
    assert buf.rows_leaving(0) == 0
    for it, n in ((0, 5), (1, 4), (2, 3)):
        buf.append(*_rows(n), iteration=it)
        assert buf.rows_leaving(it) == 0         # what that append dropped is gone already
    assert buf.rows_leaving(3) == 5 and buf.rows_leaving(4) == 9 and buf.rows_leaving(9) == 12
    held = len(buf)
    leaving = buf.rows_leaving(3)
    buf.append(*_rows(2), iteration=3)
    assert len(buf) == held - leaving + 2 and buf.rows_by_iteration()[0] == (1, 4)
    assert rvz.ReplayBuffer(32, 8, "cpu").rows_leaving(7) == 0  # no window: nothing leaves


def test_trainer_arguments():
    from rvz.pipeline import SelfPlayTrainer
    for kw in (dict(reanalyse_rows=8), dict(reanalyse_rows=8, reanalyse_age=1),
               dict(reanalyse_age=1, replay_iterations=2),
               dict(reanalyse_rows=-1, replay_iterations=2),
               dict(reanalyse_rows=8, reanalyse_age=-1, replay_iterations=2),
               dict(reanalyse_rows=True, replay_iterations=2),
               dict(reanalyse_rows=8, replay_iterations=1),
               dict(reanalyse_rows=8, reanalyse_age=1, replay_iterations=2)):
        with pytest.raises(ValueError, match="reanalyse"):
            SelfPlayTrainer(None, 4, **kw)
