"""rvz_alphabeta on 32,768 seeded 8x8 playout positions at 30 discs, depths 2, 4, 6 and 8 with the
default table: positions/s, total nodes and nodes/s, next to rvz_solve's nodes/s on the 10-empties
set of tools/exp_solve_wld.py (the same machine shape, the only comparable number the project
has). Stream events, one warm run + timed runs, outputs compared between runs.
Usage: exp_alphabeta.py OUT.json   (profiles/ab01_depths.json)"""
import json
import os
import sys
import time

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
    """tools/exp_solve_wld.py's generator, stopped at `empties` empty squares."""
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
    med = sorted(runs)[len(runs) // 2]
    res = {"config": name, "warm_ms": warm_ms, "runs_ms": runs, "median_ms": med,
           "min_ms": min(runs), "max_ms": max(runs), "timed_runs": reps,
           "positions_per_s": N / (med * 1e-3), "nodes_total": int(nodes.sum()),
           "nodes_per_s": int(nodes.sum()) / (med * 1e-3), "longest_row_nodes": int(nodes.max()),
           "mean_row_nodes": float(nodes.double().mean()),
           "rows_abandoned": int((move == -4).sum()), "rows_over": int((move == -2).sum())}
    print(json.dumps(res), flush=True)
    return res


info = {"rows": N, "board": 8, "node_limit": LIMIT, "weights": "rvz.alphabeta_weights(8)",
        "generator": "tools/exp_solve_wld.py's: torch.Generator(cuda).manual_seed(0), "
                     "torch.multinomial uniform over rvz.board_legal, rvz.board_apply",
        "device": torch.cuda.get_device_name(0),
        "cus": torch.cuda.get_device_properties(0).multi_processor_count, "results": []}
b, w, st = positions(34)
info["alphabeta_rows_at_30_discs"] = int((popcount(b | w) == 30).sum())
for depth in (2, 4, 6, 8):
    info["results"].append(measure(f"rvz_alphabeta depth {depth}, 30 discs",
                                   lambda: rvz.alphabeta(b, w, st, 8, depth, None, LIMIT),
                                   5 if depth < 8 else 2))
    with open(OUT, "w") as fh:
        json.dump(info, fh, indent=1)
b, w, st = positions(10)
info["solve_rows_at_10_empties"] = int((64 - popcount(b | w) == 10).sum())
info["results"].append(measure("rvz_solve, 10 empties", lambda: rvz.solve(b, w, st, 8, 14, LIMIT), 3))
with open(OUT, "w") as fh:
    json.dump(info, fh, indent=1)
print("done", time.strftime("%H:%M:%S"), flush=True)
