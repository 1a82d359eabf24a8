"""The record side of replay reanalysis on a 2^21-row ring at 4,096 and 32,768 selected rows:
rvz_replay_stale, rvz_replay_roots and rvz_replay_refresh, each as C-ABI calls into buffers
allocated once, against the torch expression of the same result: a stable argsort of the masked
age classes and a sort of the first n back into row order for the selection, an indexed gather for
the roots, and .float() with an indexed assignment for the scatter (the selected slots are
distinct, so the assignment needs no last-wins rule; the torch forms skip the validity checks).
The results of the two forms are compared before anything is timed.
rvz_timer events around CALLS consecutive calls; two warm runs of every form, then the forms
alternating within each repeat; median of REPS runs with min and max. The time is the stream's
between the two events, so an eager form holds the host's enqueueing where that is slower than
the device.
Usage: measure_reanalyse.py OUT.json [LOG2_ROWS]     (profiles/reanalyse01_select.json)"""
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
REPS, CALLS = 7, 20
SIZES = (4096, 32768)
BS, NPOL = 8, 65
LO, BELOW, NEW = 0, 6, 9         # stamps 0 .. 7 over the ring: six eligible classes
dev = torch.device("cuda:0")
LIB = rvz.load()


def timed(forms):
    times = {name: [] for name in forms}
    for rep in range(REPS + 2):
        for name, fn in forms.items():
            t = Timer(2)
            torch.cuda.synchronize()
            stream = stream_handle(dev)
            t.record(stream)
            for _ in range(CALLS):
                fn()
            t.record(stream)
            torch.cuda.synchronize()
            if rep >= 2:
                times[name].append(t.elapsed(0, 1) / CALLS * 1e3)
    return times


def main():
    cap = 1 << LOG2
    start, live = cap // 3, cap
    g = torch.Generator(device=dev).manual_seed(1)
    stamp = torch.randint(0, 8, (cap,), generator=g, device=dev, dtype=torch.int32)
    mover = torch.randint(0, 2 ** 62, (cap,), generator=g, device=dev, dtype=torch.int64)
    opponent = torch.randint(0, 2 ** 62, (cap,), generator=g, device=dev, dtype=torch.int64) \
        & ~mover
    policy = torch.rand(cap, NPOL, generator=g, device=dev)
    results = []
    for n in SIZES:
        s_size = LIB.rvz_replay_stale_scratch_size(cap, BELOW - LO)
        r_size = LIB.rvz_replay_refresh_scratch_size(n)
        s_scratch = torch.empty(s_size, dtype=torch.uint8, device=dev)
        r_scratch = torch.empty(r_size, dtype=torch.uint8, device=dev)
        slot = torch.empty(n, dtype=torch.int32, device=dev)
        count = torch.empty(2, dtype=torch.int32, device=dev)
        black, white = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2))
        status = torch.empty(n, 4, dtype=torch.int32, device=dev)
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        p = torch.rand(n, NPOL, generator=g, device=dev, dtype=torch.float64)
        p = (p / p.sum(1, keepdim=True)).contiguous()
        idx = torch.zeros(n, dtype=torch.int32, device=dev)
        pol, stm = policy.clone(), stamp.clone()
        stream = stream_handle(dev)

        def stale():
            LIB.rvz_replay_stale(cap, stamp.data_ptr(), start, live, n, LO, BELOW, ptr(s_scratch),
                                 s_size, slot.data_ptr(), count.data_ptr(), stream)

        def roots():
            LIB.rvz_replay_roots(BS, cap, ptr(mover), ptr(opponent), n, slot.data_ptr(),
                                 ptr(black), ptr(white), ptr(status), bad.data_ptr(), stream)

        def refresh():
            LIB.rvz_replay_refresh(BS, cap, ptr(pol), stm.data_ptr(), n, slot.data_ptr(), ptr(p),
                                   idx.data_ptr(), NEW, ptr(r_scratch), r_size, counts.data_ptr(),
                                   stream)

        order = (start + torch.arange(live, device=dev)) % cap      # logical row -> slot
        live_row = torch.tensor([1, 0, -1, 0], dtype=torch.int32, device=dev)
        t_out = {}

        def t_stale():
            st = stamp[order]
            cls = torch.where((st >= 0) & (st < BELOW), (st - LO).clamp(min=0),
                              torch.full_like(st, 1 << 20))
            first = torch.argsort(cls, stable=True)[:n]
            t_out["slot"] = order[torch.sort(first).values]

        def t_roots():
            sl = t_out["slot"]
            t_out["roots"] = (mover[sl], opponent[sl], live_row.expand(n, 4).contiguous())

        def t_refresh():
            sl = t_out["slot"]
            pol[sl] = p.float()
            stm[sl] = NEW

        # the two forms agree (every class here holds more than n rows, so all n are eligible)
        stale(); roots(); refresh()
        torch.cuda.synchronize()
        got = (slot.clone(), black.clone(), white.clone(), pol.clone(), stm.clone())
        pol.copy_(policy); stm.copy_(stamp)
        t_stale(); t_roots(); t_refresh()
        torch.cuda.synchronize()
        assert count.tolist() == [n, 0] and bad.item() == 0 and counts.tolist() == [n, 0]
        assert torch.equal(got[0].long(), t_out["slot"])
        assert torch.equal(got[1], t_out["roots"][0]) and torch.equal(got[2], t_out["roots"][1])
        assert torch.equal(got[3], pol) and torch.equal(got[4], stm)
        forms = {"rvz_replay_stale": stale, "rvz_replay_roots": roots,
                 "rvz_replay_refresh": refresh, "torch argsort selection": t_stale,
                 "torch indexed gather": t_roots, "torch indexed scatter": t_refresh}
        for name, runs in timed(forms).items():
            res = {"form": name, "ring_rows": cap, "n": n, "runs_us": runs,
                   "median_us": sorted(runs)[len(runs) // 2], "min_us": min(runs),
                   "max_us": max(runs)}
            print(json.dumps(res), flush=True)
            results.append(res)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": REPS, "calls": CALLS,
                   "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
