"""rvz_merge_positions on real self-play records: how many training rows are duplicates, and what
the merge costs.

1. One fused self-play iteration (SelfPlayTrainer, 6x64 random-init net, GAMES games from the
   start at SIMS simulations, default settings), and one more with Dirichlet root noise (0.3,
   0.25): the rows before and after merging, the ten largest groups, and per ply the share of rows
   that lie in a group of two or more.
2. The call's time at the iteration's row count and at 2^21 rows (the iteration's records tiled:
   synthetic, every group's count multiplied), with and without the per-workgroup LDS
   pre-reduction of large groups (RVZ_MERGE_HOT=0), against the composition that gives the same
   means without it: torch.unique(dim=0, return_inverse=True) on the [n, 2] int64 keys, a float64
   index_add_ and a division. rvz_timer events, two warm runs, then timed runs alternating the
   forms; allocation of outputs and scratch inside the window.
Usage: exp_merge.py OUT.json [GAMES] [SIMS]   (profiles/merge01_c2.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-reversi_amd")]
import torch  # noqa: E402

import rvz  # noqa: E402
from rvz._lib import Timer, stream_handle  # noqa: E402
from rvz.pipeline import SelfPlayTrainer  # noqa: E402

OUT = sys.argv[1]
GAMES = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
SIMS = int(sys.argv[3]) if len(sys.argv) > 3 else 800
REPS = 7
dev = torch.device("cuda:0")


def iteration(noise):
    """The kept records of one iteration in records_to_training's order (game-major):
    black, white, status, policy, value, ply."""
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(8, 6, 64).to(dev)
    spt = SelfPlayTrainer(net, GAMES, num_simulations=SIMS, seed=42, root_noise=noise)
    data = spt.generate()
    run = spt.runner
    P, G = run.rec_idx.shape
    live = (run.rec_idx >= 0).t().reshape(-1)
    black = run.rec_black.t().reshape(-1)[live].contiguous()
    white = run.rec_white.t().reshape(-1)[live].contiguous()
    side = run.rec_side.t().reshape(-1)[live].to(torch.int32)
    ply = torch.arange(P, device=dev).unsqueeze(0).expand(G, P).reshape(-1)[live]
    st = torch.zeros(black.numel(), 4, dtype=torch.int32, device=dev)
    st[:, 0], st[:, 2] = side, -1
    rows = (black, white, st, data["policy_targets"].contiguous(),
            data["value_targets"].reshape(-1).contiguous(), ply)
    torch.cuda.synchronize()
    del spt
    return rows


def duplicate_share(rows):
    black, white, st, pol, val, ply = rows
    mg = rvz.merge_positions(black, white, st, pol, val)
    n, m = black.numel(), mg["m"]
    size = mg["count"][mg["group"].long()]                    # every input row's group size
    top = torch.argsort(mg["count"], descending=True, stable=True)[:10]
    per_ply = []
    for p in range(int(ply.max()) + 1):
        at = ply == p
        per_ply.append({"ply": p, "rows": int(at.sum()),
                        "share_in_groups_of_2_or_more": float((size[at] >= 2).float().mean())})
    return {"merge_input_rows": n, "merge_rows": m, "duplicate_rows": n - m,
            "duplicate_share": (n - m) / n, "malformed_rows": int((mg["group"] < 0).sum()),
            "rows_in_groups_of_2_or_more": int((size >= 2).sum()),
            "groups_of_2_or_more": int((mg["count"] >= 2).sum()),
            "largest_groups": [{"count": int(mg["count"][j]), "first_row": int(mg["first"][j]),
                                "ply_of_first_row": int(ply[mg["first"][j].long()])}
                               for j in top.tolist()],
            "per_ply": per_ply}


def composed(black, white, st, pol, val):
    mine = (st[:, 0] == 1)
    keys = torch.stack([torch.where(mine, black, white), torch.where(mine, white, black)], dim=1)
    _, inv, cnt = torch.unique(keys, dim=0, return_inverse=True, return_counts=True)
    sums = torch.zeros(cnt.numel(), pol.shape[1] + 1, dtype=torch.float64, device=dev)
    sums.index_add_(0, inv, torch.cat([pol, val.unsqueeze(1)], dim=1).double())
    return (sums / cnt.unsqueeze(1)).float(), inv


def hot_off(fn):
    def run():
        os.environ["RVZ_MERGE_HOT"] = "0"
        try:
            return fn()
        finally:
            del os.environ["RVZ_MERGE_HOT"]
    return run


def timing(rows, label):
    black, white, st, pol, val = rows[:5]
    n = black.numel()

    def kernel():
        return rvz.merge_positions(black, white, st, pol, val, trim=False)

    forms = {"rvz_merge_positions": kernel,
             "rvz_merge_positions without the LDS pre-reduction": hot_off(kernel),
             "torch.unique + index_add_ (float64) + division": lambda: composed(*rows[:5])}
    mg = kernel()
    mean, inv = composed(*rows[:5])
    ok = mg["group"] >= 0
    ours = torch.cat([mg["policy"], mg["value"].unsqueeze(1)], dim=1)[mg["group"][ok].long()]
    gap = float((ours - mean[inv[ok]]).abs().max())
    m = int(mg["m"])
    del mg, mean, inv, ours
    times = {name: [] for name in forms}
    for rep in range(REPS + 2):
        for name, fn in forms.items():
            t = Timer(2)
            h = stream_handle(dev)
            t.record(h)
            out = fn()
            t.record(h)
            torch.cuda.synchronize()
            if rep >= 2:
                times[name].append(t.elapsed(0, 1))
            del out
    res = {"rows": n, "distinct": m, "what": label, "timed_runs": REPS,
           "max_abs_difference_of_means_kernel_vs_composition": gap, "forms": []}
    for name, runs in times.items():
        res["forms"].append({"form": name, "runs_ms": runs, "median_ms": sorted(runs)[len(runs) // 2],
                             "min_ms": min(runs), "max_ms": max(runs)})
    med = {f["form"]: f["median_ms"] for f in res["forms"]}
    res["composition_over_kernel"] = med["torch.unique + index_add_ (float64) + division"] / \
        med["rvz_merge_positions"]
    res["without_over_with_pre_reduction"] = \
        med["rvz_merge_positions without the LDS pre-reduction"] / med["rvz_merge_positions"]
    print(json.dumps(res), flush=True)
    return res


info = {"games": GAMES, "sims": SIMS, "net": "6x64 random init (torch.manual_seed(0))", "board": 8,
        "device": torch.cuda.get_device_name(0),
        "timer": "rvz_timer events around each call, allocation inside the window; two warm "
                 "runs of every form, then the forms alternating within each repeat",
        "iterations": {}, "timing": []}
base = None
for label, noise in (("default", None), ("root_noise_0.3_0.25", (0.3, 0.25))):
    rows = iteration(noise)
    info["iterations"][label] = duplicate_share(rows)
    print(label, json.dumps({k: v for k, v in info["iterations"][label].items()
                             if k not in ("per_ply",)}), flush=True)
    if base is None:
        base = rows
n = base[0].numel()
info["timing"].append(timing(base, "the default iteration's records"))
at = torch.arange(1 << 21, device=dev) % n
tiled = tuple(t[at].contiguous() for t in base[:5])
info["timing"].append(timing(tiled, "synthetic: the default iteration's records tiled to 2^21 "
                                    "rows (every group's count multiplied)"))
with open(OUT, "w") as fh:
    json.dump(info, fh, indent=1)
print("done", flush=True)
