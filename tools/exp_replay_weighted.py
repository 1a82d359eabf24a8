"""The time of one training batch drawn in proportion to per-row weights from a 2^21-row 8x8 ring
by rvz_replay_batch_weighted (the table of prefix sums built once, outside the window), at
nb = 64 and nb = 4,096, against what a user has without it: torch.multinomial(w, nb,
replacement=True) on the weights in logical order followed by rvz.replay_batch(idx=...), existing
code that is not under test; the uniform rvz.replay_batch beside them for scale; the kernel's
C-ABI call alone into outputs allocated once; and the table build (rvz_replay_cdf) alone, at the
default tile and at the other tiles. Then the same at 2^25 rows, where the question is whether
the torch path runs at all: the error it raises, or its time, is recorded.
rvz_timer events around BATCHES consecutive calls, every batch another step; two warm runs of
every form, then the forms alternating within each repeat. The time is the stream's between the
two events, so it holds the host's enqueueing where that is slower than the device. Output
allocation is inside the window except for the C-ABI forms.
Usage: exp_replay_weighted.py OUT.json [LOG2_ROWS [LOG2_BIG_ROWS]]
(profiles/replayw01_batch.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-reversi_amd")]
import torch  # noqa: E402

import rvz  # noqa: E402
from rvz._lib import Timer, ptr, stream_handle  # noqa: E402

OUT = sys.argv[1]
LOG2 = int(sys.argv[2]) if len(sys.argv) > 2 else 21
LOG2_BIG = int(sys.argv[3]) if len(sys.argv) > 3 else 25
REPS, BATCHES = 7, 100
SIZES = (64, 4096)
TILES = (0, 8, 9, 10, 12)
dev = torch.device("cuda:0")
LIB = rvz.load()
STREAM = stream_handle(dev)


def ring(n, seed):
    """A ring of n random records and weights like a merged, decayed window's: a count in
    [1, 8] (most rows 1) times a recency factor 0.9^age over 20 iterations, 1% of the rows 0."""
    gen = torch.Generator(device=dev).manual_seed(seed)

    def rand64():
        hi = torch.randint(0, 1 << 32, (n,), generator=gen, device=dev, dtype=torch.int64)
        lo = torch.randint(0, 1 << 32, (n,), generator=gen, device=dev, dtype=torch.int64)
        return (hi << 32) | lo

    occupied, colour = rand64() | rand64(), rand64()
    mover, opponent = occupied & colour, occupied & ~colour
    del occupied, colour
    policy = torch.rand(n, 65, generator=gen, device=dev)
    value = torch.rand(n, generator=gen, device=dev) * 2 - 1
    count = torch.rand(n, generator=gen, device=dev).pow(8).mul(8).floor().add(1)
    start = n // 3                                         # a ring that wraps
    age = (19 - ((torch.arange(n, device=dev) - start) % n) * 20 // n).float()
    weight = count * torch.pow(torch.tensor(0.9, device=dev), age)
    weight[torch.rand(n, generator=gen, device=dev) < 0.01] = 0.0
    return (mover, opponent, policy, value), weight, start


def timed(forms, nb):
    """{form: [us per call]} over REPS timed runs of BATCHES calls, after two warm runs."""
    times = {name: [] for name in forms}
    for rep in range(REPS + 2):
        for name, fn in forms.items():
            t = Timer(2)
            torch.cuda.synchronize()
            t.record(STREAM)
            for s in range(BATCHES):
                out = fn(nb, s)
            t.record(STREAM)
            torch.cuda.synchronize()
            if rep >= 2:
                times[name].append(t.elapsed(0, 1) / BATCHES * 1e3)
            del out
    return times


def summary(name, nb, runs, **more):
    res = {"form": name, "nb": nb, "runs_us": runs, "median_us": sorted(runs)[len(runs) // 2],
           "min_us": min(runs), "max_us": max(runs), **more}
    print(json.dumps(res), flush=True)
    return res


def measure(log2_rows, info):
    n = 1 << log2_rows
    rows, weight, start = ring(n, log2_rows)
    logical = weight[(start + torch.arange(n, device=dev)) % n].contiguous()
    table = rvz.replay_cdf(weight, start, n)
    ring_ptr = [ptr(t) for t in rows]
    total, invalid = int(table[0]), int(table[1])
    entry = {"rows": n, "total_weight": total / 65536, "invalid_weights": invalid,
             "table_bytes": table.numel() * 8, "results": []}

    def weighted(nb, s):
        return rvz.replay_batch_weighted(*rows, table, start, n, nb, 0, s)

    held = {nb: weighted(nb, 0) for nb in SIZES}
    held_ptr = {nb: [ptr(t) for t in held[nb]] for nb in SIZES}

    def weighted_raw(nb, s):
        rc = LIB.rvz_replay_batch_weighted(8, n, *ring_ptr, ptr(table), start, n, nb, None, None,
                                           None, 1, 0, s, *held_ptr[nb], STREAM)
        assert rc == 0, rc
        return held[nb]

    def uniform(nb, s):
        return rvz.replay_batch(*rows, start, n, nb, 0, s)

    def multinomial(nb, s):
        idx = torch.multinomial(logical, nb, replacement=True)
        return rvz.replay_batch(*rows, start, n, nb, 0, s, idx=idx)

    forms = {"rvz_replay_batch_weighted": weighted,
             "rvz_replay_batch_weighted, the C-ABI call into outputs allocated once": weighted_raw,
             "rvz_replay_batch (uniform, for scale)": uniform}
    try:                                                   # does the torch path run at this size?
        multinomial(64, 0)
        torch.cuda.synchronize()
        forms["torch.multinomial + rvz_replay_batch(idx)"] = multinomial
        entry["torch_multinomial"] = "runs"
    except RuntimeError as err:
        entry["torch_multinomial"] = f"refused: {str(err).splitlines()[0]}"
    print(json.dumps({"rows": n, "torch_multinomial": entry["torch_multinomial"]}), flush=True)

    # the draw's frequencies follow the weights: 2^20 draws in 16 equal slices of the logical rows
    nbig = 1 << 20
    out = rvz.replay_batch_weighted(*rows, table, start, n, nbig, 1, 0)
    at = (out[3].long() - start) % n
    got = torch.bincount(at * 16 // n, minlength=16).double() / nbig
    want = logical.double().reshape(16, -1).sum(1) / logical.double().sum()
    entry["max_slice_frequency_error"] = float((got - want).abs().max())
    entry["slice_frequency_5_sigma"] = float(5 * (want * (1 - want) / nbig).sqrt().max())
    assert bool((logical[at] > 0).all())
    del out, at

    for nb in SIZES:
        for name, runs in timed(forms, nb).items():
            entry["results"].append(summary(name, nb, runs))

    # the table build alone, into a buffer allocated once
    builds = {}
    for tl in TILES:
        buf = torch.empty(LIB.rvz_replay_cdf_size(n, tl) // 8, dtype=torch.int64, device=dev)

        def build(nb, s, tl=tl, buf=buf):
            rc = LIB.rvz_replay_cdf(n, ptr(weight), start, n, tl, ptr(buf), STREAM)
            assert rc == 0, rc
            return buf

        build(0, 0)
        torch.cuda.synchronize()
        assert torch.equal(buf[:4 + n], table[:4 + n]), tl
        builds[f"rvz_replay_cdf, tile_log2 = {tl}" + (" (the default, 11)" if tl == 0 else "")] = \
            build
    for name, runs in timed(builds, 0).items():
        entry["results"].append(summary(name, None, runs, bytes_must_move=n * (4 + 8)))
    info["rings"].append(entry)


info = {"board": 8, "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
        "timer": f"rvz_timer events around {BATCHES} consecutive calls (stream time: the larger "
        "of the host's enqueueing and the device's work)", "timed_runs": REPS,
        "calls_per_run": BATCHES,
        "order": "two warm runs of every form, then the forms alternating within each repeat",
        "weights": "count in [1, 8] x 0.9^age over 20 iterations, 1% of the rows 0",
        "rings": []}
for log2_rows in (LOG2, LOG2_BIG):
    measure(log2_rows, info)
    torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(info, fh, indent=1)
print("done", flush=True)
