"""rvz_training_rows at 2^20 rows on 8x8 with fan = 1 and fan = 8, against the composition that
produces the same arrays without it: rvz.board_canonical, then torch.rot90 / flip per image and an
index gather on the policy. rvz_timer events, two warm runs, then timed runs alternating the forms;
the outputs of the two forms are compared element for element first. Bytes per second are the
bytes the algorithm must move (inputs read once, every output byte written once) over the time.
Usage: exp_symmetry.py OUT.json [LOG2_ROWS]   (profiles/sym01_rows.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-reversi_amd")]
import torch  # noqa: E402

import rvz  # noqa: E402
from rvz._lib import Timer, stream_handle  # noqa: E402

OUT = sys.argv[1]
N = 1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 20)
REPS = 7
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(0)


def rand64():
    hi = torch.randint(0, 1 << 32, (N,), generator=gen, device=dev, dtype=torch.int64)
    lo = torch.randint(0, 1 << 32, (N,), generator=gen, device=dev, dtype=torch.int64)
    return (hi << 32) | lo


occupied, colour = rand64() | rand64(), rand64()          # about 3/4 of the squares hold a disc
black, white = occupied & colour, occupied & ~colour
status = torch.zeros(N, 4, dtype=torch.int32, device=dev)
status[:, 0] = torch.randint(1, 3, (N,), generator=gen, device=dev, dtype=torch.int32)
status[:, 2] = -1
policy = torch.rand(N, 65, generator=gen, device=dev)
sym = torch.randint(0, 8, (N,), generator=gen, device=dev, dtype=torch.int32)

# out[s] = in[SRC[k][s]] (include/rvz.h), for the composition's policy gather
SRC = torch.stack([torch.cat([(torch.fliplr(torch.rot90(torch.arange(64).reshape(8, 8), k & 3))
                               if k & 4 else torch.rot90(torch.arange(64).reshape(8, 8), k & 3))
                              .reshape(-1), torch.tensor([64])]) for k in range(8)]).to(dev)


def image(x, k):
    y = torch.rot90(x, k & 3, dims=(-2, -1))
    return torch.flip(y, dims=(-1,)) if k & 4 else y


def composed_all():
    planes = rvz.board_canonical(black, white, status, 8)
    states = torch.stack([image(planes, k) for k in range(8)], dim=1).reshape(8 * N, 3, 8, 8)
    pol = torch.stack([policy[:, SRC[k]] for k in range(8)], dim=1).reshape(8 * N, 65)
    return states, pol


def composed_one():
    planes = rvz.board_canonical(black, white, status, 8)
    states = torch.empty_like(planes)
    for k in range(8):
        m = sym == k
        states[m] = image(planes[m], k)
    return states, torch.gather(policy, 1, SRC[sym.long()])


FORMS = {
    "rvz_training_rows fan=1": lambda: rvz.training_rows(black, white, status, policy, sym, 8),
    "rvz_training_rows fan=1 with quirk": lambda: rvz.training_rows(black, white, status, policy,
                                                                    sym, 8, quirk=True),
    "composition fan=1": composed_one,
    "rvz_training_rows fan=8": lambda: rvz.training_rows(black, white, status, policy, None, 8,
                                                         all_images=True),
    "rvz_training_rows fan=8 with quirk": lambda: rvz.training_rows(black, white, status, policy,
                                                                    None, 8, all_images=True,
                                                                    quirk=True),
    "composition fan=8": composed_all,
}


def must_move(name):
    fan = 8 if "fan=8" in name else 1
    return N * (8 + 8 + 16 + 260 + (4 if fan == 1 else 0)) + \
        N * fan * (768 + 260 + (4 if "quirk" in name else 0))


for fan in ("fan=1", "fan=8"):
    a = FORMS[f"rvz_training_rows {fan}"]()
    b = FORMS[f"composition {fan}"]()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), fan
    del a, b
torch.cuda.synchronize()

info = {"rows": N, "board": 8, "timer": "rvz_timer events around each call, output allocation "
        "(torch.empty) inside the window", "timed_runs": REPS, "order": "two warm runs of every "
        "form, then the forms alternating within each repeat",
        "device": torch.cuda.get_device_name(0), "outputs_equal": True, "results": []}
times = {name: [] for name in FORMS}
for rep in range(REPS + 2):
    for name, fn in FORMS.items():
        t = Timer(2)
        h = stream_handle(dev)
        t.record(h)
        out = fn()
        t.record(h)
        torch.cuda.synchronize()
        if rep >= 2:
            times[name].append(t.elapsed(0, 1))
        del out
for name, runs in times.items():
    med = sorted(runs)[len(runs) // 2]
    res = {"form": name, "runs_ms": runs, "median_ms": med, "min_ms": min(runs),
           "max_ms": max(runs), "bytes_must_move": must_move(name),
           "bytes_per_s_at_median": must_move(name) / (med * 1e-3)}
    print(json.dumps(res), flush=True)
    info["results"].append(res)
med = {r["form"]: r["median_ms"] for r in info["results"]}
info["composition_over_kernel"] = {f: med[f"composition {f}"] / med[f"rvz_training_rows {f}"]
                                   for f in ("fan=1", "fan=8")}
with open(OUT, "w") as fh:
    json.dump(info, fh, indent=1)
print("done", json.dumps(info["composition_over_kernel"]), flush=True)
