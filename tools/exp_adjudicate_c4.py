"""C4-shaped self-play (10x128 net, 800 simulations, fused) with adjudicate_empties in {0, 8, 10}:
selfplay_s of generate() and the adjudication's own time. Usage:
exp_adjudicate_c4.py GAMES OUT.json (profiles/solve02_c4_adjudicate.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-reversi_amd")]
import torch  # noqa: E402

import rvz  # noqa: E402
from rvz.pipeline import SelfPlayTrainer  # noqa: E402
from rvz.trainer import adjudicate  # noqa: E402

G, OUT = int(sys.argv[1]), sys.argv[2]
dev = torch.device("cuda:0")
torch.manual_seed(0)
net = rvz.AlphaZeroNetwork(8, 10, 128).to(dev)
res = {"games": G, "net": "10x128", "num_simulations": 800, "batch_size": 64, "fused": True,
       "runs": []}
for N in (0, 8, 10):
    spt = SelfPlayTrainer(net, G, 800, 64, seed=42, train_steps=0, adjudicate_empties=N)
    row = {"adjudicate_empties": N, "selfplay_s": []}
    for rep in range(2):                      # the first generate() warms the kernels
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        data = spt.generate()
        torch.cuda.synchronize(dev)
        row["selfplay_s"].append(time.perf_counter() - t0)
    row["samples"] = int(data["states"].shape[0])
    for k in ("adjudicated", "adjudicate_unsolved", "already_over"):
        row[k] = int(data.get(k, 0))
    if N:
        b, w, st = spt.eng.get_state()
        ms = []
        for rep in range(3):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            adjudicate(b, w, st, 8, check_depth=False)
            z.record()
            z.synchronize()
            ms.append(a.elapsed_time(z))
        row["adjudicate_ms"] = ms
        _, _, nodes = rvz.solve_wld(b, w, st, 8)
        row["adjudicate_nodes_total"] = int(nodes.sum())
        row["adjudicate_longest_row_nodes"] = int(nodes.max())
    print(json.dumps(row), flush=True)
    res["runs"].append(row)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    del spt, data
    torch.cuda.empty_cache()
