"""Where one C2-shaped reanalysis pass spends its time: 4,096 ring rows searched again at 800
simulations (batch 64) with a 6x64 net through LeafEvaluator, on an engine of 4,096 games with
compacted leaf batches: the steps of ReplayBuffer.reanalyse one by one, each between two device
synchronisations (host wall time, so a step holds its host enqueueing): rvz.replay_stale,
rvz.replay_roots, Engine.set_state, Engine.search, Engine.act, rvz.replay_refresh. The ring holds
distinct real positions (rvz.openings, ply 7), all stamped 0. One warm pass, then RUNS passes;
per step the median with min and max, and its share of the pass's median total.
Usage: measure_reanalyse_share.py OUT.json     (profiles/reanalyse01_share.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-reversi_amd")]
import torch  # noqa: E402

import rvz  # noqa: E402

OUT = sys.argv[1]
ROWS, SIMS, BATCH, RUNS = 4096, 800, 64, 3
STEPS = ("replay_stale", "replay_roots", "set_state", "search", "act", "replay_refresh")


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ev = rvz.LeafEvaluator(rvz.AlphaZeroNetwork(8, 6, 64).to(dev).eval())
    eng = rvz.Engine(ROWS, num_simulations=SIMS, batch_size=BATCH, compact_leaves=True)
    o = rvz.openings(8, 7)
    cap = 2 * ROWS
    b, w, side = o["black"][:cap], o["white"][:cap], o["status"][:cap, 0]
    assert b.numel() == cap
    buf = rvz.ReplayBuffer(cap, 8, dev, stamps=True)
    pol = torch.full((cap, 65), 1.0 / 65, device=dev)
    buf.append(torch.where(side == 1, b, w), torch.where(side == 1, w, b), pol,
               torch.zeros(cap, device=dev), iteration=0)
    u = torch.full((ROWS,), 0.5, dtype=torch.float64, device=dev)
    times = {s: [] for s in STEPS}
    for run in range(RUNS + 1):
        buf.stamp.zero_()
        t = {}

        def step(name, fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            t[name] = (time.perf_counter() - t0) * 1e3
            return out
        slot, count = step("replay_stale", lambda: rvz.replay_stale(buf.stamp, buf.start, len(buf),
                                                                    ROWS, 0, 1))
        roots = step("replay_roots", lambda: rvz.replay_roots(buf.mover, buf.opponent, slot, 8))
        step("set_state", lambda: eng.set_state(*roots[:3]))
        step("search", lambda: eng.search(ev))
        idx, p = step("act", lambda: eng.act(1.0, u=u, apply=False))
        counts = step("replay_refresh", lambda: rvz.replay_refresh(buf.policy, buf.stamp, slot, p,
                                                                   idx, 1))
        eng.check()
        assert count.tolist() == [ROWS, 0] and counts.tolist() == [ROWS, 0]
        print(json.dumps({"run": run, "ms": t}), flush=True)
        if run:
            for s in STEPS:
                times[s].append(t[s])
    med = {s: sorted(v)[len(v) // 2] for s, v in times.items()}
    total = sum(med.values())
    res = {"device": torch.cuda.get_device_name(0), "rows": ROWS, "simulations": SIMS,
           "batch": BATCH, "net": "6x64", "runs": RUNS, "total_median_ms": total,
           "steps": {s: {"runs_ms": times[s], "median_ms": med[s], "min_ms": min(times[s]),
                         "max_ms": max(times[s]), "share": med[s] / total} for s in STEPS},
           "share_search": med["search"] / total,
           "share_three_calls": (med["replay_stale"] + med["replay_roots"] +
                                 med["replay_refresh"]) / total}
    print(json.dumps(res), flush=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
