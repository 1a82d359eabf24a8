"""A NumPy restatement of the three record-side calls of replay reanalysis (include/rvz.h:
rvz_replay_stale, rvz_replay_roots, rvz_replay_refresh), written from the contract and not from
the kernels: plain loops over rows, no tiles, no table. The reference of every bit-for-bit
statement in tests/test_reanalyse_cpu.py and tests/test_gpu_reanalyse.py."""
import numpy as np

LIVE_ROW = (1, 0, -1, 0)         # a live game, black to move, no winner, no pass behind it
OVER_ROW = (1, 1, 0, 0)          # a game that is over: the engine searches nothing for it


def stale(stamp, start, live, n, lo, below):
    """(out_slot int32 [n], out_count int32 [2])."""
    stamp = np.asarray(stamp, np.int32)
    cap = len(stamp)
    assert 1 <= live <= cap and 0 <= start < cap and n >= 0
    assert 0 <= lo < below and below - lo <= 65536
    rows, bad = [], 0                            # (class, logical row)
    for i in range(live):
        s = int(stamp[(start + i) % cap])
        if s < 0:
            bad += 1
        elif s < below:
            rows.append((max(s - lo, 0), i))
    # the smallest classes, ties to the older row; then back into logical-row order
    taken = sorted(i for _, i in sorted(rows)[:n])
    out = np.full(n, -1, np.int32)
    out[:len(taken)] = [(start + i) % cap for i in taken]
    return out, np.array([len(taken), bad], np.int32)


def roots(mover, opponent, slot, board_size):
    """(black uint64 [n], white uint64 [n], status int32 [n, 4], bad int32 [1])."""
    mover, opponent = np.asarray(mover).view(np.uint64), np.asarray(opponent).view(np.uint64)
    cap, n = len(mover), len(slot)
    board = (1 << (board_size * board_size)) - 1
    black, white = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    status = np.tile(np.array(OVER_ROW, np.int32), (n, 1))
    bad = 0
    for r, s in enumerate(int(x) for x in slot):
        if s == -1:
            continue
        if not 0 <= s < cap:
            bad += 1
            continue
        b, w = int(mover[s]), int(opponent[s])
        if b & w or (b | w) & ~board:
            bad += 1
            continue
        black[r], white[r], status[r] = b, w, LIVE_ROW
    return black, white, status, np.array([bad], np.int32)


def row_sum(row):
    """The float64 sum the kernel's wavefront forms: lane l holds row[l] (0 from the row's end
    on), lane 0 adds row[64] where there is one, then the xor butterfly d = 32 .. 1."""
    row = np.asarray(row, np.float64)
    x = np.zeros(64, np.float64)
    m = min(len(row), 64)
    x[:m] = row[:m]
    if len(row) > 64:
        x[0] = x[0] + row[64]
    lanes = np.arange(64)
    d = 32
    while d:
        x = x + x[lanes ^ d]
        d >>= 1
    return x[0]


def skipped(cap, slot, row, idx):
    if not 0 <= slot < cap or idx == -2:
        return True
    row = np.asarray(row, np.float64)
    if not np.all(np.isfinite(row)) or np.any(row < 0):
        return True
    return not abs(row_sum(row) - 1.0) <= 1e-9


def refresh(policy, stamp, slot, p, idx, new_stamp):
    """(policy, stamp, counts int32 [2]): copies of the ring after the sequential loop."""
    policy, stamp = np.array(policy, np.float32), np.array(stamp, np.int32)
    p = np.asarray(p, np.float64)
    cap = len(stamp)
    written, skips = set(), 0
    for r in range(len(slot)):
        s = int(slot[r])
        if skipped(cap, s, p[r], int(idx[r])):
            skips += 1
            continue
        policy[s] = p[r].astype(np.float32)
        stamp[s] = new_stamp
        written.add(s)
    return policy, stamp, np.array([len(written), skips], np.int32)
