"""rvz_solve against rvz_solve_window (-1, 1) with order_min_empties in {0, 4, 5, 6, 7} on 32,768
seeded 8x8 playout positions at E empties. Usage: exp_solve_wld.py E OUT.json
(profiles/solve02_wld_e10.json, solve02_wld_e12.json)"""
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


def timed(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z), out


def measure(name, fn, ref=None):
    warm_ms, warm = timed(fn)
    reps = 5 if warm_ms < 12000 else (3 if warm_ms < 30000 else 1)
    runs = []
    for _ in range(reps):
        ms, out = timed(fn)
        assert all(torch.equal(x, y) for x, y in zip(out, warm)), name
        runs.append(ms)
    score, move, nodes = warm
    res = {"config": name, "warm_ms": warm_ms, "runs_ms": runs,
           "median_ms": sorted(runs)[len(runs) // 2], "timed_runs": reps,
           "nodes_total": int(nodes.sum()), "longest_row_nodes": int(nodes.max()),
           "rows_at_node_limit": int((move == -4).sum())}
    if ref is not None:       # the sign agrees with rvz_solve wherever both solved the row
        both = (move != -4) & (ref[1] != -4)
        res["sign_mismatches"] = int((torch.sign(score) != torch.sign(ref[0]))[both].sum())
    print(json.dumps(res), flush=True)
    return res, warm


b, w, st = positions()
emp = 64 - popcount(b | w)
info = {"rows": N, "board": 8, "empties": E, "max_empties": 14, "node_limit": LIMIT,
        "generator": "torch.Generator(cuda).manual_seed(0), torch.multinomial uniform over "
                     "rvz.board_legal, rvz.board_apply, from the start position until E empties",
        "rows_over": int((st[:, 1] != 0).sum()), "rows_at_E": int((emp == E).sum())}
print(json.dumps(info), flush=True)
results = []
base, ref = measure("rvz_solve", lambda: rvz.solve(b, w, st, 8, 14, LIMIT))
results.append(base)
for order in (0, 4, 5, 6, 7):
    r, _ = measure(f"rvz_solve_window(-1,1) order_min_empties={order}",
                   lambda: rvz.solve_window(b, w, st, 8, 14, LIMIT, -1, 1, order), ref)
    r["ratio_to_rvz_solve"] = r["median_ms"] / base["median_ms"]
    results.append(r)
    info["results"] = results
    with open(OUT, "w") as f:
        json.dump(info, f, indent=1)
print("done", time.strftime("%H:%M:%S"), flush=True)
