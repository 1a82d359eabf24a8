"""rvz_openings against the same enumeration written from Python with rvz.board_legal /
rvz.board_apply / torch.unique, at 8x8, plies 6 and 8: the median of 7 runs with min and max,
written as profiles/openings01_enumerate.json.

The torch form expands a level by one board_apply call per square (64 masked launches a level),
drops the finished children and de-duplicates with torch.unique(dim=0) on (black, white, side)
rows, restoring first-occurrence order from the inverse indices; its rows are checked against
rvz.openings' before anything is timed.

    python tools/measure_openings.py [--out profiles/openings01_enumerate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-reversi_amd"))

import rvz  # noqa: E402


def torch_openings(bs: int, plies: int):
    dev = "cuda"
    first = rvz.openings(bs, 0)
    b, w, st = first["black"], first["white"], first["status"]
    for _ in range(plies):
        legal = rvz.board_legal(b, w, st, bs)
        n = b.numel()
        cb, cw, cs, order = [], [], [], []
        for sq in range(bs * bs):
            bit = torch.tensor(1 << sq if sq < 63 else -2 ** 63, dtype=torch.int64, device=dev)
            rows = torch.nonzero(legal & bit).reshape(-1)
            if not rows.numel():
                continue
            nb, nw, ns = b[rows], w[rows], st[rows]            # copies: board_apply is in place
            rvz.board_apply(nb, nw, ns, torch.full((rows.numel(),), sq, dtype=torch.int32,
                                                   device=dev), bs)
            live = ns[:, 1] == 0
            cb.append(nb[live])
            cw.append(nw[live])
            cs.append(ns[live, 0].to(torch.int64))
            order.append(rows[live] * (bs * bs) + sq)          # (parent, square) order
        key = torch.cat(order).argsort()
        cand = torch.stack([torch.cat(cb)[key], torch.cat(cw)[key], torch.cat(cs)[key]], dim=1)
        uniq, inv = torch.unique(cand, dim=0, return_inverse=True)
        firsts = torch.full((uniq.shape[0],), cand.shape[0], dtype=torch.int64, device=dev)
        firsts.scatter_reduce_(0, inv, torch.arange(cand.shape[0], device=dev), "amin")
        keep = cand[firsts.sort().values]
        b, w = keep[:, 0].contiguous(), keep[:, 1].contiguous()
        st = torch.zeros(keep.shape[0], 4, dtype=torch.int32, device=dev)
        st[:, 0] = keep[:, 2].to(torch.int32)
        st[:, 2] = -1
    return b, w, st


def timed(fn, runs=7):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3),
            "max_ms": round(max(out), 3), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "openings01_enumerate.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "board_size": 8, "cases": []}
    for plies in (6, 8):
        got = rvz.openings(8, plies)
        tb, tw, tst = torch_openings(8, plies)
        assert torch.equal(tb, got["black"]) and torch.equal(tw, got["white"])
        assert torch.equal(tst, got["status"])
        k = timed(lambda: rvz.openings(8, plies))
        t = timed(lambda: torch_openings(8, plies))
        res["cases"].append({"plies": plies, "rows": int(got["stats"][0]),
                             "largest_level_candidates": int(got["stats"][4]),
                             "rvz_openings": k, "torch_enumeration": t,
                             "ratio_torch_over_rvz": round(t["median_ms"] / k["median_ms"], 2)})
        print(json.dumps(res["cases"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
