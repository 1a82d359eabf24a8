"""A short A/B of one library (RVZ_LIB) on the two negamax kernels' long rows: rvz_alphabeta at
depth 7 on tools/exp_alphabeta.py's 32,768 rows at 30 discs (warm + 1 timed run, about a minute
each) and rvz_solve on tools/exp_solve_wld.py's rows at 10 empties (warm + 4 timed); node totals
and output checksums to compare between libraries. Usage: exp_negamax_screen.py OUT.json
(profiles/neg02_screen_*.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-reversi_amd")]
import torch  # noqa: E402

import rvz  # noqa: E402
from oracle import oracle as O  # noqa: E402

OUT = sys.argv[1]
N, LIMIT = 32768, 2 ** 24
dev = torch.device("cuda:0")
bits = torch.arange(64, dtype=torch.int64, device=dev)


def popcount(x):
    return ((x.unsqueeze(1) >> bits) & 1).sum(1)


def positions(empties):
    g0 = O.new_game(8)
    u64 = lambda v: v - (1 << 64) if v >= (1 << 63) else v
    b = torch.full((N,), u64(g0.black), dtype=torch.int64, device=dev)
    w = torch.full((N,), u64(g0.white), dtype=torch.int64, device=dev)
    st = torch.tensor([[g0.side, 0, -1, 0]], dtype=torch.int32, device=dev).repeat(N, 1)
    gen = torch.Generator(device=dev).manual_seed(0)
    for _ in range(64):
        act = (st[:, 1] == 0) & (64 - popcount(b | w) > empties)
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


def timed(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z), out


def measure(name, fn, reps):
    warm_ms, warm = timed(fn)
    runs = []
    for _ in range(reps):
        ms, out = timed(fn)
        assert all(torch.equal(x, y) for x, y in zip(out, warm)), name
        runs.append(ms)
    score, move, nodes = warm
    res = {"config": name, "lib": os.path.basename(os.environ.get("RVZ_LIB", "")), "warm_ms": warm_ms,
           "runs_ms": runs, "nodes_total": int(nodes.sum()),
           "longest_row_nodes": int(nodes.max()), "rows_abandoned": int((move == -4).sum()),
           "score_sum": int(score.long().sum()), "move_sum": int(move.long().sum())}
    print(json.dumps(res), flush=True)
    return res


res = []
b, w, st = positions(34)
res.append(measure("rvz_alphabeta depth 7, 30 discs",
                   lambda: rvz.alphabeta(b, w, st, 8, 7, None, LIMIT), 1))
b, w, st = positions(10)
res.append(measure("rvz_solve, 10 empties", lambda: rvz.solve(b, w, st, 8, 14, LIMIT), 4))
with open(OUT, "w") as fh:
    json.dump(res, fh, indent=1)
