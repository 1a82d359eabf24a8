"""rvz_solve_moves against the composition it replaces (children by rvz.board_legal /
rvz.board_apply, then rvz.solve_window on them with the mapped windows) on 32,768 seeded 8x8
playout positions at E empties: (a) rvz.solve_moves at (-64, 64), ordering off; (b)
rvz.solve_moves_wld at its default ordering; (c) the composition at each one's window and
ordering. Usage: exp_solve_moves.py E OUT.json   (profiles/solve04_moves_e10.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-reversi_amd")]
import torch  # noqa: E402

import rvz  # noqa: E402
from oracle import oracle as O  # noqa: E402

E, OUT = int(sys.argv[1]), sys.argv[2]
N, LIMIT = 32768, 2 ** 24
dev = torch.device("cuda:0")
bits = torch.arange(64, dtype=torch.int64, device=dev)


def popcount(x):
    return ((x.unsqueeze(1) >> bits) & 1).sum(1)


def positions():
    """tools/exp_solve_wld.py's generator: the same rows."""
    g0 = O.new_game(8)
    u64 = lambda v: v - (1 << 64) if v >= (1 << 63) else v
    b = torch.full((N,), u64(g0.black), dtype=torch.int64, device=dev)
    w = torch.full((N,), u64(g0.white), dtype=torch.int64, device=dev)
    st = torch.tensor([[g0.side, 0, -1, 0]], dtype=torch.int32, device=dev).repeat(N, 1)
    gen = torch.Generator(device=dev).manual_seed(0)
    for _ in range(64):
        act = (st[:, 1] == 0) & (64 - popcount(b | w) > E)
        idx = torch.nonzero(act).reshape(-1)
        if idx.numel() == 0:
            break
        bb, ww, ss = b[idx].contiguous(), w[idx].contiguous(), st[idx].contiguous()
        legal = rvz.board_legal(bb, ww, ss, 8)
        p = ((legal.unsqueeze(1) >> bits) & 1).to(torch.float32)
        sq = torch.multinomial(p, 1, generator=gen).reshape(-1).to(torch.int32)
        ok = rvz.board_apply(bb, ww, ss, sq, 8)
        assert bool((ok != 0).all())
        b[idx], w[idx], st[idx] = bb, ww, ss
    return b, w, st


def composition(b, w, st, alpha, beta, order):
    """(scores, count, nodes) in rvz_solve_moves' layout from the public pieces. Roots that are
    over or cannot move are left to the caller (this workload's roots at E empties can move)."""
    live = st[:, 1] == 0
    legal = torch.where(live, rvz.board_legal(b, w, st, 8), torch.zeros_like(b))
    row, sq = torch.nonzero((legal.unsqueeze(1) >> bits) & 1, as_tuple=True)
    cb, cw, cs = b[row].contiguous(), w[row].contiguous(), st[row].contiguous()
    rvz.board_apply(cb, cw, cs, sq.to(torch.int32), 8)
    kept = cs[:, 0] == st[row, 0]
    score = torch.empty_like(sq, dtype=torch.int32)
    nodes = torch.empty_like(sq)
    for sel, (lo, hi), sign in ((kept, (alpha, beta), 1), (~kept, (-beta, -alpha), -1)):
        s, m, k = rvz.solve_window(cb[sel], cw[sel], cs[sel], 8, 14, LIMIT, lo, hi, order)
        score[sel] = torch.where(m == -4, torch.full_like(s, rvz.SOLVE_ABANDONED), sign * s)
        nodes[sel] = k
    scores = torch.full((N, 65), rvz.SOLVE_NOT_A_MOVE, dtype=torch.int32, device=dev)
    allnodes = torch.zeros((N, 65), dtype=torch.int64, device=dev)
    scores[row, sq] = score
    allnodes[row, sq] = nodes
    return scores, torch.bincount(row, minlength=N).to(torch.int32), allnodes


def timed(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z), out


def measure(name, fn, reps=5):
    warm_ms, warm = timed(fn)
    runs = []
    for _ in range(reps):
        ms, out = timed(fn)
        assert all(torch.equal(x, y) for x, y in zip(out, warm)), name
        runs.append(ms)
    scores, count, nodes = warm
    res = {"config": name, "warm_ms": warm_ms, "runs_ms": runs,
           "median_ms": sorted(runs)[len(runs) // 2], "min_ms": min(runs), "max_ms": max(runs),
           "timed_runs": reps, "nodes_total": int(nodes.sum()),
           "longest_move_nodes": int(nodes.max()), "moves": int((nodes > 0).sum()),
           "rows_with_an_abandoned_move": int((scores == rvz.SOLVE_ABANDONED).any(1).sum())}
    print(json.dumps(res), flush=True)
    return res, warm


b, w, st = positions()
emp = 64 - popcount(b | w)
info = {"rows": N, "board": 8, "empties": E, "max_empties": 14, "node_limit": LIMIT,
        "generator": "tools/exp_solve_wld.py's: torch.Generator(cuda).manual_seed(0), "
                     "torch.multinomial uniform over rvz.board_legal, rvz.board_apply",
        "rows_over": int((st[:, 1] != 0).sum()), "rows_at_E": int((emp == E).sum())}
print(json.dumps(info), flush=True)
WLD = rvz.engine.WLD_ORDER_MIN_EMPTIES
results = []
for tag, alpha, beta, order, fused in (
        ("a", -64, 64, 0, lambda: rvz.solve_moves(b, w, st, 8, 14, LIMIT, -64, 64, 0)),
        ("b", -1, 1, WLD, lambda: rvz.solve_moves(b, w, st, 8, 14, LIMIT, -1, 1, WLD))):
    f, fo = measure(f"({tag}) rvz_solve_moves ({alpha},{beta}) order_min_empties={order}", fused)
    c, co = measure(f"(c) board_apply children + rvz_solve_window at ({tag})'s window and "
                    f"ordering", lambda: composition(b, w, st, alpha, beta, order))
    # the two agree on every root the composition covers (live roots with a legal square)
    rows = fo[1] >= 1
    passing = rows & (fo[0][:, 64] != rvz.SOLVE_NOT_A_MOVE)
    rows = rows & ~passing
    f["equals_composition"] = all(bool(torch.equal(x[rows], y[rows])) for x, y in zip(fo, co))
    f["pass_roots"], f["rows_not_searched"] = int(passing.sum()), int((fo[1] < 1).sum())
    f["ratio_to_composition"] = f["median_ms"] / c["median_ms"]
    results += [f, c]
    info["results"] = results
    with open(OUT, "w") as fh:
        json.dump(info, fh, indent=1)
print("done", time.strftime("%H:%M:%S"), flush=True)
