"""Continuous self-play records, measured on the MI355X (profiles/records01_games_*.json).

1. Per call: rvz_records_games on a window of 120 plies at 4,096 and at 32,768 slots (8x8), as
   the C-ABI call into buffers allocated once and through rvz.records_games (which allocates its
   outputs), against the torch expression it replaces: records_to_training(compact=True) on whole
   lockstep games of the same number of records ([60 plies, twice the slots]). The windows are 128
   synthetic columns of random playouts (tests/records_games_ref.py; the slots open at different
   move numbers) tiled over the slots. rvz_timer events around CALLS consecutive calls, two warm
   runs, then REPS timed runs with the forms alternating; the torch form synchronises with the
   host at its boolean-mask gathers, so its time includes those round trips.
2. The self-play phase: board-steps/s of SelfPlayTrainer.generate() with continuous_plies = 60
   (one launch of 60 plies with autoreset, records_games, games_to_training, roll) against the
   lockstep generate() (60 plies without reset, records_to_training(compact=True)), the same
   net, seed and shape, both trainers resident, alternating; the evaluator is refreshed before
   every run (no memo or table entries carry over); one warm run, then REPS timed ones.
Usage: bench_records.py OUTDIR [GAMES SIMS BLOCKS FILTERS]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-reversi_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import records_games_ref as RG  # noqa: E402
import rvz  # noqa: E402
from oracle import oracle as O  # noqa: E402
from rvz._lib import Timer, stream_handle  # noqa: E402
from rvz.pipeline import SelfPlayTrainer  # noqa: E402
from rvz.trainer import records_to_training  # noqa: E402

OUT = sys.argv[1]
GAMES, SIMS, BLOCKS, FILTERS = (int(x) for x in (sys.argv[2:6] + ["4096", "800", "6", "64"][
    len(sys.argv) - 2:]))
REPS, CALLS, COLS, PLIES = 7, 10, 128, 120
dev = torch.device("cuda:0")
LIB = rvz.load()


def spread(runs):
    return {"runs": runs, "median": sorted(runs)[len(runs) // 2], "min": min(runs),
            "max": max(runs)}


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


def lockstep(cols):
    """cols whole games from the start as [60, cols] records and their final status."""
    rng = np.random.default_rng(1)
    black, white = np.zeros((60, cols), np.uint64), np.zeros((60, cols), np.uint64)
    side, idx = np.zeros((60, cols), np.int32), np.full((60, cols), -2, np.int32)
    final = np.zeros((cols, 4), np.int32)
    for g in range(cols):
        game = O.new_game(8)
        for k, rec in enumerate(RG.stream(O, 8, rng, 60)):
            if k and rec[:2] == (int(game.black), int(game.white)):
                break                                       # the next game's start position
            black[k, g], white[k, g], side[k, g], idx[k, g] = rec
            last = O.Game(rec[0], rec[1], rec[2], 0, -1, 0)
            assert O.make_move(last, rec[3], 8)
        final[g] = (last.side, last.over, last.winner, last.passed)
    p = rng.random((60, cols, 65))
    p /= p.sum(axis=2, keepdims=True)
    return black, white, side, idx, p, final


def per_call():
    O.lib()
    win = RG.window(O, 8, PLIES, COLS, 0, offsets={g: 7 * g % 60 for g in range(COLS)})
    lock = lockstep(COLS)
    results = []
    for G in (4096, 32768):
        tile = lambda a, n=G // COLS: np.concatenate([a] * n, axis=1)
        b, w, s, i, p = RG.tensors(*(tile(a) for a in win), device=dev)
        n = PLIES * G
        outs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2)] + \
            [torch.empty(n, 65, device=dev), torch.empty(n, device=dev),
             torch.empty(n, dtype=torch.int32, device=dev)]
        m = torch.zeros(1, dtype=torch.int32, device=dev)
        stats = torch.zeros(8, dtype=torch.int64, device=dev)
        scratch = torch.empty(LIB.rvz_records_scratch_size(PLIES, G), dtype=torch.uint8,
                              device=dev)
        lb, lw, ls, li, lp = RG.tensors(*(tile(a, 2 * G // COLS) for a in lock[:5]), device=dev)
        lf = torch.from_numpy(np.concatenate([lock[5]] * (2 * G // COLS))).to(dev)

        def raw():
            rc = LIB.rvz_records_games(8, PLIES, G, b.data_ptr(), w.data_ptr(), s.data_ptr(),
                                       i.data_ptr(), p.data_ptr(), 60, scratch.data_ptr(),
                                       m.data_ptr(), *(t.data_ptr() for t in outs), None,
                                       stats.data_ptr(), stream_handle(dev))
            assert rc == 0, rc

        forms = {"rvz_records_games": raw,
                 "rvz.records_games": lambda: rvz.records_games(b, w, s, i, p, 8, emit_from=60),
                 "records_to_training(compact=True)":
                     lambda: records_to_training(lb, lw, ls, li, lp, lf, 8, compact=True)}
        times = timed(forms)
        raw()
        rows_torch = int(forms["records_to_training(compact=True)"]()["mover"].numel())
        for name, runs in times.items():
            res = {"form": name, "slots": G, "plies": PLIES, "records": n, "unit": "us per call",
                   "rows": int(m) if name.startswith("rvz") else rows_torch, **spread(runs)}
            print(json.dumps(res), flush=True)
            results.append(res)
    return results


def selfplay():
    def trainer(**kw):
        torch.manual_seed(0)
        net = rvz.AlphaZeroNetwork(8, BLOCKS, FILTERS).to(dev)
        return SelfPlayTrainer(net, GAMES, num_simulations=SIMS, seed=42, replay_iterations=2,
                               **kw)
    forms = {"continuous_plies=60": trainer(continuous_plies=60), "lockstep": trainer()}
    runs = {name: [] for name in forms}
    rows = {name: [] for name in forms}
    for rep in range(REPS + 1):
        for name, spt in forms.items():
            spt.evaluator.refresh()
            torch.cuda.synchronize()
            steps0 = int(spt.runner.steps.item())
            t0 = time.perf_counter()
            data = spt.generate()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            spt.iteration += 1
            if rep >= 1:
                runs[name].append((int(spt.runner.steps.item()) - steps0) / dt)
                rows[name].append(int(data["mover"].numel()))
    results = []
    for name in forms:
        res = {"form": name, "games": GAMES, "sims": SIMS, "net": f"{BLOCKS}x{FILTERS}",
               "unit": "board-steps/s", "rows_per_run": rows[name], **spread(runs[name])}
        print(json.dumps(res), flush=True)
        results.append(res)
    return results


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    info = {"device": torch.cuda.get_device_name(0), "reps": REPS, "calls_per_run": CALLS}
    with open(os.path.join(OUT, "records01_games_calls.json"), "w") as f:
        json.dump({**info, "results": per_call()}, f, indent=1)
    with open(os.path.join(OUT, "records01_games_selfplay.json"), "w") as f:
        json.dump({**info, "results": selfplay()}, f, indent=1)
