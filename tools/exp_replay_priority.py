"""What prioritized replay adds to a training step on a 2^21-row ring, at nb = 64 and nb = 4,096:
rvz_replay_is_weight alone, rvz_replay_priority alone, and the whole addition (is_weight, priority,
then the rvz_replay_cdf rebuild), each as C-ABI calls into buffers allocated once, eager and
replayed from a HIP graph; against the torch expression of the same result: min and pow for the
importance weights, pow and clamp for the priorities, and a last-wins index_put_ made deterministic
by a stable sort of the slots that hands every member of a run of equal slots the run's last value
(so the duplicate writes all carry the same bytes), followed by the same rvz_replay_cdf. The torch
form skips the validity checks (its inputs here are all valid) and its power is the device
library's, not the correctly rounded one: its results are compared to the kernels' within 2 ulp.
The batch is a real draw (rvz_replay_batch_weighted) and its loss rows are random.
rvz_timer events around CALLS consecutive calls (or graph replays); two warm runs of every form,
then the forms alternating within each repeat. The time is the stream's between the two events, so
an eager form holds the host's enqueueing where that is slower than the device.
Usage: exp_replay_priority.py OUT.json [LOG2_ROWS]     (profiles/priority01_step.json)"""
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
REPS, CALLS = 7, 100
SIZES = (64, 4096)
BETA, ALPHA, FLOOR, CAP = 0.4, 0.6, 2.0 ** -8, 2.0 ** 8
dev = torch.device("cuda:0")
LIB = rvz.load()


def timed(forms):
    """{form: [us per call]} over REPS timed runs of CALLS calls, after two warm runs."""
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


def summary(name, nb, runs, **more):
    res = {"form": name, "nb": nb, "runs_us": runs, "median_us": sorted(runs)[len(runs) // 2],
           "min_us": min(runs), "max_us": max(runs), **more}
    print(json.dumps(res), flush=True)
    return res


def graphed(fn):
    """fn captured once on the capture stream; returns the replay, or None with the reason."""
    try:
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        g.replay()
        torch.cuda.synchronize()
        return g.replay, None
    except RuntimeError as err:
        return None, str(err).splitlines()[0]


def measure(info):
    n = 1 << LOG2
    gen = torch.Generator(device=dev).manual_seed(LOG2)
    mover = torch.randint(0, 1 << 62, (n,), generator=gen, device=dev, dtype=torch.int64)
    policy = torch.rand(n, 65, generator=gen, device=dev)
    value = torch.rand(n, generator=gen, device=dev) * 2 - 1
    weight0 = torch.rand(n, generator=gen, device=dev).pow(4).mul(16).clamp(FLOOR, CAP)
    start = n // 3
    table = rvz.replay_cdf(weight0, start, n)
    for nb in SIZES:
        draw = rvz.replay_batch_weighted(mover, ~mover & ((1 << 62) - 1), policy, value, table,
                                         start, n, nb, 0, 1)
        slot, prob = draw[3], draw[5]
        lp = torch.rand(nb, generator=gen, device=dev, dtype=torch.float64) * 5
        rows = torch.stack([lp, torch.rand(nb, generator=gen, device=dev, dtype=torch.float64),
                            lp * torch.rand(nb, generator=gen, device=dev, dtype=torch.float64)],
                           1).contiguous()
        weight = weight0.clone()
        top = torch.ones(1, device=dev)
        isw = torch.empty(nb, device=dev)
        pri = torch.empty(nb, device=dev)
        state = torch.empty(nb, dtype=torch.int32, device=dev)
        s_isw = torch.empty(LIB.rvz_replay_is_weight_scratch_size(nb), dtype=torch.uint8,
                            device=dev)
        s_pri = torch.empty(LIB.rvz_replay_priority_scratch_size(nb), dtype=torch.uint8,
                            device=dev)
        cdf = torch.empty_like(table)

        def is_weight():
            rc = LIB.rvz_replay_is_weight(nb, ptr(prob), ptr(slot), BETA, ptr(s_isw), ptr(isw),
                                          None, stream_handle(dev))
            assert rc == 0, rc

        def priority():
            rc = LIB.rvz_replay_priority(n, ptr(weight), nb, ptr(slot), ptr(rows), 1.0, 1.0, 1,
                                         ALPHA, FLOOR, CAP, ptr(s_pri), ptr(top), ptr(pri),
                                         ptr(state), stream_handle(dev))
            assert rc == 0, rc

        def rebuild():
            rc = LIB.rvz_replay_cdf(n, ptr(weight), start, n, 0, ptr(cdf), stream_handle(dev))
            assert rc == 0, rc

        def whole():
            is_weight()
            priority()
            rebuild()

        t_weight = weight0.clone()
        t_top = torch.ones(1, device=dev)
        ar = torch.arange(nb, device=dev)
        slot64 = slot.long()

        def torch_is_weight():
            return (prob.min().double() / prob.double()).pow(BETA).float()

        def torch_priority():
            e = (rows[:, 0] - rows[:, 2]).clamp(min=0) + rows[:, 1]
            p = e.pow(ALPHA).clamp(FLOOR, CAP).float()
            s, order = torch.sort(slot64, stable=True)
            is_last = torch.ones_like(s, dtype=torch.bool)
            is_last[:-1] = s[1:] != s[:-1]
            cand = torch.where(is_last, ar, nb)
            last = torch.flip(torch.cummin(torch.flip(cand, [0]), 0).values, [0])
            t_weight.index_put_((s,), p[order][last])
            torch.maximum(t_top, p.max(), out=t_top)
            return p

        def torch_whole():
            torch_is_weight()
            torch_priority()
            rc = LIB.rvz_replay_cdf(n, ptr(t_weight), start, n, 0, ptr(cdf), stream_handle(dev))
            assert rc == 0, rc

        # the two forms write the same slots, to values within 2 ulp of each other
        whole()
        t_isw, t_pri = torch_is_weight(), torch_priority()
        torch.cuda.synchronize()
        changed = weight != weight0
        assert torch.equal(changed, t_weight != weight0) and int(state.min()) >= 0

        def ulp(a, b):
            return int((a.view(torch.int32) - b.view(torch.int32)).abs().max())
        entry = {"nb": nb, "slots_written": int(changed.sum()),
                 "rows_superseded": int((state == 0).sum()),
                 "torch_max_ulp": {"weight": ulp(weight, t_weight), "is_weight": ulp(isw, t_isw),
                                   "priority": ulp(pri, t_pri)}}
        assert max(entry["torch_max_ulp"].values()) <= 2, entry
        print(json.dumps(entry), flush=True)

        eager = {"rvz_replay_is_weight": is_weight, "rvz_replay_priority": priority,
                 "rvz_replay_cdf (the rebuild)": rebuild,
                 "is_weight + priority + cdf (the step's addition)": whole,
                 "torch: min, pow": torch_is_weight,
                 "torch: pow, clamp, stable sort, cummin, index_put_": torch_priority,
                 "torch forms + rvz_replay_cdf": torch_whole}
        forms = {name + ", eager": fn for name, fn in eager.items()}
        for name, fn in eager.items():
            replay, why = graphed(fn)
            if replay is None:
                entry.setdefault("not_capturable", {})[name] = why
            else:
                forms[name + ", graph replay"] = replay
        entry["results"] = [summary(name, nb, runs) for name, runs in timed(forms).items()]
        info["batches"].append(entry)


info = {"board": 8, "rows": 1 << LOG2, "device": torch.cuda.get_device_name(0),
        "torch": torch.__version__, "beta": BETA, "alpha": ALPHA, "floor": FLOOR, "cap": CAP,
        "timer": f"rvz_timer events around {CALLS} consecutive calls or graph replays (stream "
        "time: the larger of the host's enqueueing and the device's work)", "timed_runs": REPS,
        "calls_per_run": CALLS,
        "order": "two warm runs of every form, then the forms alternating within each repeat",
        "batches": []}
measure(info)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(info, fh, indent=1)
print("done", flush=True)
