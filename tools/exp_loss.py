"""The time of one loss call with its gradients at n = 64 and n = 4,096 rows on 8x8:
rvz.policy_value_loss (rvz_policy_value_loss: float64, weighted, outputs and scratch allocated per
call), its C-ABI call alone into buffers allocated once, and the same loss and gradients written
as a torch float32 expression (log_softmax, the masked products, the sums, the weighting, the
squared error, torch.autograd.grad), eager; then the kernel call and the torch expression each
captured in a HIP graph and replayed, which leaves the device's time and takes the host's
enqueueing out. The losses and gradients are compared first (float32 against float64: 1e-4
relative). rvz_timer events around CALLS consecutive calls, two warm runs of every form, then the
forms alternating within each repeat. The eager times hold the host's enqueueing where that is
slower than the device.
Usage: exp_loss.py OUT.json   (profiles/loss01_call.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-reversi_amd")]
import torch  # noqa: E402

import rvz  # noqa: E402
from rvz._lib import Timer, ptr, stream_handle  # noqa: E402

OUT = sys.argv[1]
REPS, CALLS = 7, 200
SIZES = (64, 4096)
WP, WV = 1.0, 1.0
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(0)


def inputs(n):
    z = torch.randn(n, 65, generator=gen, device=dev) * 3
    y = torch.tanh(torch.randn(n, generator=gen, device=dev))
    visits = torch.randint(0, 50, (n, 65), generator=gen, device=dev).float() * \
        (torch.rand(n, 65, generator=gen, device=dev) < 0.4)
    visits[:, 0] += 1
    pi = visits / visits.sum(1, keepdim=True)
    t = torch.randint(-1, 2, (n,), generator=gen, device=dev).float()
    w = torch.randint(1, 4097, (n,), generator=gen, device=dev).float()
    return z, y, pi, t, w


def torch_loss(z, y, pi, t, w):
    zg, yg = z.detach().requires_grad_(True), y.detach().requires_grad_(True)
    logp = torch.log_softmax(zg, dim=1)
    lp = -torch.where(pi > 0, pi * logp, torch.zeros_like(logp)).sum(1)
    lv = (yg - t) ** 2
    W = w.sum()
    loss = (w * (WP * lp + WV * lv)).sum() / W
    gz, gy = torch.autograd.grad(loss, (zg, yg))
    return loss.detach(), gz, gy


def timed(fn, timer, stream):
    a = timer.record(stream)
    for _ in range(CALLS):
        fn()
    b = timer.record(stream)
    torch.cuda.synchronize()
    return timer.elapsed(a, b) * 1000.0 / CALLS             # us per call


result = {"device": torch.cuda.get_device_name(0), "calls_per_run": CALLS, "repeats": REPS,
          "unit": "us per call", "sizes": {}}
lib = rvz.load()
for n in SIZES:
    z, y, pi, t, w = inputs(n)
    ker = rvz.policy_value_loss(z, y, pi, t, w, WP, WV)
    tl, tgz, tgy = torch_loss(z, y, pi, t, w)
    rel = abs(ker["loss"].item() - tl.item()) / abs(ker["loss"].item())
    gerr = (ker["grad_logits"] - tgz).abs().max().item() / tgz.abs().max().item()
    assert rel < 1e-4 and gerr < 1e-4, (rel, gerr)
    assert (ker["grad_value"] - tgy).abs().max().item() <= 1e-4 * tgy.abs().max().item()

    scratch = torch.empty(lib.rvz_loss_scratch_size(8, n), dtype=torch.uint8, device=dev)
    out_loss = torch.empty(8, dtype=torch.float64, device=dev)
    gl, gv = torch.empty(n, 65, device=dev), torch.empty(n, device=dev)
    stream = stream_handle(dev)

    def raw():
        rc = lib.rvz_policy_value_loss(8, n, z.data_ptr(), y.data_ptr(), pi.data_ptr(),
                                       t.data_ptr(), w.data_ptr(), WP, WV, ptr(scratch),
                                       out_loss.data_ptr(), None, gl.data_ptr(), gv.data_ptr(),
                                       stream)
        assert rc == 0

    forms = {"kernel": lambda: rvz.policy_value_loss(z, y, pi, t, w, WP, WV),
             "kernel_c_abi": raw,
             "torch_f32": lambda: torch_loss(z, y, pi, t, w)}
    # graph replays: the device's time of each form
    side = torch.cuda.Stream()
    graphs = {}
    for name in ("kernel", "torch_f32"):
        with torch.cuda.stream(side):
            for _ in range(3):
                forms[name]()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g):
                keep = forms[name]()
        except RuntimeError as e:                            # reported, the eager forms stand
            result.setdefault("capture_errors", {})[f"{name}_{n}"] = str(e)[:200]
            continue
        graphs[name] = (g, keep)
        forms[name + "_graph"] = g.replay
    timer = Timer(2 * (REPS + 2) * len(forms) + 4)
    stream = stream_handle(dev)
    for _ in range(2):                                       # warm
        for fn in forms.values():
            timed(fn, timer, stream)
    runs = {name: [] for name in forms}
    for _ in range(REPS):
        for name, fn in forms.items():
            runs[name].append(timed(fn, timer, stream))
    entry = {"loss_rel_diff_f32_vs_f64": rel, "grad_rel_diff_f32_vs_f64": gerr}
    for name, xs in runs.items():
        xs = sorted(xs)
        entry[name] = {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "runs": runs[name]}
    result["sizes"][str(n)] = entry
    print(n, {k: round(v["median"], 2) for k, v in entry.items() if isinstance(v, dict)},
          flush=True)

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(result, f, indent=1)
