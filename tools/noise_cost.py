"""Cost of the Dirichlet root noise at the C2 workload (4,096 games x 800 simulations, the 6x64
net, fused self-play with the memo, the deferred last batch and the cross-game table):
board-steps per second with the noise off and with Engine.root_noise(0.3, 0.25), alternating,
`--runs` runs each, every run a fresh engine, warmed up, timed with device events over whole
launches. Prints one JSON line. The games differ between the two settings (the noise changes the
searches), so this is a throughput figure of two workloads, not an A/B of one.

    python tools/noise_cost.py [--runs 3] [--plies 30] [--games 4096]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-reversi_amd"))


def one_run(net, games, sims, plies, warmup, noise):
    import rvz
    eng = rvz.Engine(games, sims, 64, memo=True)
    eng.table(1 << 20, 14)
    if noise:
        eng.root_noise(*noise)
    run = rvz.SelfPlayRunner(eng, rvz.LeafEvaluator(net), autoreset=True, seed_base=42,
                             skip_last_eval=True, fused=True)
    run.start()
    for _ in range(warmup):
        run.ply()
    torch.cuda.synchronize()
    s0 = int(run.steps.item())
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(plies):
        run.ply()
    t1.record()
    torch.cuda.synchronize()
    run.check()
    return (int(run.steps.item()) - s0) / (t0.elapsed_time(t1) * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--plies", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=800)
    a = ap.parse_args()
    import rvz
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(8, 6, 64).cuda().eval()
    off, on = [], []
    for _ in range(a.runs):
        off.append(one_run(net, a.games, a.sims, a.plies, a.warmup, None))
        on.append(one_run(net, a.games, a.sims, a.plies, a.warmup, (0.3, 0.25)))
    mo, mn = statistics.median(off), statistics.median(on)
    print(json.dumps({"workload": f"{a.games} games x {a.sims} sims, 6x64, fused",
                      "steps_per_s_noise_off": off, "steps_per_s_noise_on": on,
                      "median_off": mo, "median_on": mn, "on_over_off": mn / mo}))


if __name__ == "__main__":
    main()
