"""The time of one training batch drawn from a 2^21-row 8x8 ring by rvz_replay_batch (compact
records, a random symmetry per row), at nb = 64 and nb = 4,096, against what DDPTrainer.train_epoch
does for a batch: three gathers data[...][idx] from the expanded arrays of the same rows, idx a
slice of a host permutation copied to the device; and against those gathers with idx already on
the device; a fourth form is the kernel's C-ABI call alone into outputs allocated once, the least
the host can do per batch. The outputs are compared element for element first (the kernel under the identity,
given the gathers' idx). rvz_timer events around BATCHES consecutive batches, every batch another
step / another slice; two warm runs of every form, then the forms alternating within each repeat.
The time is the stream's between the two events, so it holds the host's enqueueing where that is
slower than the device. Output allocation (torch.empty / the gathers' results) is inside the window.
Usage: exp_replay.py OUT.json [LOG2_ROWS]   (profiles/replay01_batch.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-reversi_amd")]
import torch  # noqa: E402

import rvz  # noqa: E402
from rvz._lib import Timer, ptr, stream_handle  # noqa: E402

OUT = sys.argv[1]
N = 1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 21)
REPS, BATCHES = 7, 200
SIZES = (64, 4096)
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(0)


def rand64():
    hi = torch.randint(0, 1 << 32, (N,), generator=gen, device=dev, dtype=torch.int64)
    lo = torch.randint(0, 1 << 32, (N,), generator=gen, device=dev, dtype=torch.int64)
    return (hi << 32) | lo


occupied, colour = rand64() | rand64(), rand64()          # about 3/4 of the squares hold a disc
mover, opponent = occupied & colour, occupied & ~colour
policy = torch.rand(N, 65, generator=gen, device=dev)
value = torch.rand(N, generator=gen, device=dev) * 2 - 1
del occupied, colour
START = N // 3                                             # a ring that wraps

# the parent's data: the same rows expanded, in logical order (oldest first)
logical = (START + torch.arange(N, device=dev)) % N
status = torch.zeros(N, 4, dtype=torch.int32, device=dev)
status[:, 0], status[:, 2] = 1, -1
states_x, policy_x = rvz.training_rows(mover[logical], opponent[logical], status,
                                       policy[logical].contiguous(),
                                       torch.zeros(N, dtype=torch.int32, device=dev), 8)
data = {"states": states_x, "policy_targets": policy_x,
        "value_targets": value[logical].reshape(N, 1).contiguous()}
del status, logical
order = torch.randperm(N, generator=torch.Generator().manual_seed(0))       # on the host
order_dev = order.to(dev)


def kernel(nb, s):
    return rvz.replay_batch(mover, opponent, policy, value, START, N, nb, 0, s)


LIB, RING = rvz.load(), [ptr(t) for t in (mover, opponent, policy, value)]
HELD = {nb: kernel(nb, 0) for nb in SIZES}       # outputs allocated once
HELD_PTR = {nb: [ptr(t) for t in HELD[nb]] for nb in SIZES}
STREAM = stream_handle(dev)


def kernel_raw(nb, s):
    """The C-ABI call alone, into outputs allocated once: the least the host does per batch."""
    rc = LIB.rvz_replay_batch(8, N, *RING, START, N, nb, None, None, 1, 0, s, *HELD_PTR[nb],
                              STREAM)
    assert rc == 0, rc
    return HELD[nb]


def gathers_host_idx(nb, s):
    idx = order[s * nb:(s + 1) * nb].to(dev)
    return data["states"][idx], data["policy_targets"][idx], data["value_targets"][idx]


def gathers_device_idx(nb, s):
    idx = order_dev[s * nb:(s + 1) * nb]
    return data["states"][idx], data["policy_targets"][idx], data["value_targets"][idx]


FORMS = {"rvz_replay_batch": kernel,
         "rvz_replay_batch, the C-ABI call into outputs allocated once": kernel_raw,
         "three gathers, idx from the host permutation (train_epoch)": gathers_host_idx,
         "three gathers, idx on the device": gathers_device_idx}

for nb in SIZES:
    idx = order_dev[:nb]
    a = rvz.replay_batch(mover, opponent, policy, value, START, N, nb, 0, 0, random_sym=False,
                         idx=idx)
    b = gathers_device_idx(nb, 0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), nb
    assert torch.equal(a[3].long(), (START + idx) % N) and not bool(a[4].any())
    del a, b
torch.cuda.synchronize()

info = {"rows": N, "board": 8, "ring_bytes": N * 280, "expanded_bytes": N * 1032,
        "timer": f"rvz_timer events around {BATCHES} consecutive batches (stream time: the "
        "larger of the host's enqueueing and the device's work), output allocation inside",
        "timed_runs": REPS, "batches_per_run": BATCHES,
        "order": "two warm runs of every form, then the forms alternating within each repeat",
        "device": torch.cuda.get_device_name(0), "outputs_equal": True, "results": []}
for nb in SIZES:
    times = {name: [] for name in FORMS}
    for rep in range(REPS + 2):
        for name, fn in FORMS.items():
            t = Timer(2)
            h = stream_handle(dev)
            torch.cuda.synchronize()
            t.record(h)
            for s in range(BATCHES):
                out = fn(nb, s)
            t.record(h)
            torch.cuda.synchronize()
            if rep >= 2:
                times[name].append(t.elapsed(0, 1) / BATCHES * 1e3)
            del out
    for name, runs in times.items():
        res = {"form": name, "nb": nb, "runs_us_per_batch": runs,
               "median_us_per_batch": sorted(runs)[len(runs) // 2],
               "min_us_per_batch": min(runs), "max_us_per_batch": max(runs),
               "bytes_must_move_per_batch": nb * (280 + 1040) if name.startswith("rvz_replay_batch")
               else nb * (8 + 2 * 1032)}
        print(json.dumps(res), flush=True)
        info["results"].append(res)
med = {(r["form"], r["nb"]): r["median_us_per_batch"] for r in info["results"]}
info["gathers_over_kernel"] = {
    str(nb): {f: med[(f, nb)] / med[("rvz_replay_batch", nb)] for f in FORMS
              if f != "rvz_replay_batch"} for nb in SIZES}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(info, fh, indent=1)
print("done", json.dumps(info["gathers_over_kernel"]), flush=True)
