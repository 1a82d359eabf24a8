"""rvz_policy_value_loss on the GPU against the NumPy float64 reference (tests/loss_ref.py), its
determinism, graph capture, the autograd form, and DDPTrainer(policy_target="full").

The bound on every float64 output: within 1e-12 * max(1, scale) of the reference, scale the
largest |logp| of the batch. Derivation: the kernel and the reference compute the same float64
formulas on the same float32 inputs and differ only in the order of their sums and in the last
bit of exp and log. Differences of float32 inputs (z - m, y - t) are exact in float64; exp and
log are within an ulp; a sum of A <= 65 terms stays below 65 eps relative to the sum of the
magnitudes, which for pi . logp is at most S * scale. So a row's Lp, H and lse are off by less
than about 140 eps * scale = 1.5e-14 * scale (eps = 2^-53), the weighted means over rows add a
few eps of their own relative to values that are again at most scale, and 1e-12 leaves roughly
60 times that. Counts (W on integer weights, the malformed rows) and the agreement numerator are
sums of integers below 2^53, exact in any order, so they and the agreement are compared for
equality. A float32 gradient is the float64 value rounded once: the two float64 values differ
far below a float32 ulp, so the results are equal or adjacent float32 numbers.
Outputs are pre-filled with NaN before every raw call, so a comparison also shows that every
element was written."""
import functools

import numpy as np
import pytest
import torch

import loss_ref as LR

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 257, 4097)
KINDS = ("none", "counts", "zeros")
MALFORMED = 12                       # malformed rows in _inputs at n >= 63 (3 need a weight)


@functools.lru_cache(maxsize=None)
def _inputs(bs, n, kind):
    """The shared inputs of one (board, n, weights) case, host arrays; never modified."""
    A = bs * bs + 1
    g = np.random.default_rng(1000 * bs + n)
    z = g.standard_normal((n, A)) * np.where(np.arange(n) % 2 == 0, 1.0, 30.0)[:, None]
    for r in range(n):
        if r % 7 == 3:
            z[r, g.integers(A)] += 1e4                       # needs the max subtraction
        if r % 7 == 5:
            z[r, g.integers(A)] -= 1e4
    z = z.astype(np.float32)
    pi = np.zeros((n, A), np.float32)
    for r in range(n):
        k = r % 4
        if k == 0 or k == 3:                                 # normalised visit counts with zeros
            v = g.integers(1, 200, A) * (g.random(A) < 0.35)
            v[g.integers(A)] += 1
            pi[r] = (v / v.sum()).astype(np.float32)
        elif k == 1:                                         # one-hot, the pass index included
            pi[r, A - 1 if r % 8 == 1 else g.integers(A)] = 1.0
        else:                                                # uniform over k moves
            m = int(g.integers(2, 9))
            pi[r, g.choice(A, m, replace=False)] = np.float32(1.0 / m)
    if n >= 2:
        pi[n // 2] = 0.0                                     # one all-zero row
    y = np.tanh(g.standard_normal(n)).astype(np.float32)
    t = g.choice(np.array([-1.0, 0.0, 1.0, 1.0 / 3, -0.25], np.float32), n)
    if kind == "none":
        w = None
    elif kind == "counts":
        w = g.integers(1, 4097, n).astype(np.float32)
        w[g.random(n) < 0.1] = 0.0
    else:
        w = np.zeros(n, np.float32)
    if n >= 63:                                              # one row of each malformed kind
        z[10, 3] = np.nan
        z[11, A - 1] = -np.inf
        y[12] = np.nan
        y[13] = np.inf
        pi[14, 5] = -1e-3
        pi[15, 0] = 1.5
        pi[16, 7] = np.nan
        t[17] = 1.5
        t[18] = np.nan
        if w is not None:
            w[19], w[20], w[21] = -1.0, np.inf, np.nan
    for a in (z, pi, y, t) + (() if w is None else (w,)):
        a.setflags(write=False)
    return z, y, pi, t, w


@functools.lru_cache(maxsize=None)
def _reference(bs, n, kind, wp=1.0, wv=1.0):
    z, y, pi, t, w = _inputs(bs, n, kind)
    return LR.batch(z, y, pi, t, w, wp, wv)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(bs, dev, wp=1.0, wv=1.0, rows=True, grads=True, stream=None, out=None):
    """rvz_policy_value_loss through the C-ABI on NaN-filled outputs: (out_loss, rows,
    grad_logits, grad_value)."""
    import rvz
    from rvz._lib import ptr
    z, y, pi, t, w = dev
    n, A = z.shape
    lib = rvz.load()
    if out is None:
        out = (torch.full((8,), float("nan"), dtype=torch.float64, device="cuda"),
               torch.full((n, 3), float("nan"), dtype=torch.float64, device="cuda"),
               torch.full((n, A), float("nan"), device="cuda"),
               torch.full((n,), float("nan"), device="cuda"))
    scratch = torch.full((lib.rvz_loss_scratch_size(bs, n),), 0xFF, dtype=torch.uint8,
                         device="cuda")                      # NaN bit patterns: no preparation
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    a = [None if x is None else x.data_ptr() for x in (z, y, pi, t, w)]
    rc = lib.rvz_policy_value_loss(bs, n, *a, wp, wv, ptr(scratch), out[0].data_ptr(),
                                   out[1].data_ptr() if rows else None,
                                   out[2].data_ptr() if grads else None,
                                   out[3].data_ptr() if grads else None, stream)
    assert rc == 0, rc
    return out + (scratch,)                                  # the scratch lives until the sync


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _adjacent(got, want):
    """got == want, or got is the float32 next to want on either side."""
    up = np.nextafter(want, np.float32(np.inf))
    down = np.nextafter(want, np.float32(-np.inf))
    return (got == want) | (got == up) | (got == down)


def _compare(got, ref, what):
    out_loss, rows, gl, gv = (x.cpu().numpy() for x in got[:4])
    bound = 1e-12 * max(1.0, ref["scale"])
    err = np.abs(out_loss - ref["out_loss"])
    print(what, "scale", ref["scale"], "out_loss err", err.max(), "rows err",
          np.abs(rows - ref["rows"]).max(), "bound", bound)
    assert np.isfinite(out_loss).all() and np.isfinite(rows).all(), what
    assert np.isfinite(gl).all() and np.isfinite(gv).all(), what
    assert (err <= bound).all(), (what, err, bound)
    assert (np.abs(rows - ref["rows"]) <= bound).all(), what
    for k in (4, 5, 6, 7):                                   # W, the agreement, the count, 0
        assert out_loss[k] == ref["out_loss"][k], (what, k)
    assert _adjacent(gl, ref["grad_logits"]).all(), what
    assert _adjacent(gv, ref["grad_value"]).all(), what


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bs", [8, 6])
def test_kernel_against_the_reference(bs, n, kind):
    host = _inputs(bs, n, kind)
    ref = _reference(bs, n, kind)
    if n >= 63:
        assert ref["out_loss"][6] == (MALFORMED if kind != "none" else MALFORMED - 3)
    got = _raw(bs, [_dev(a) for a in host])
    _compare(got, ref, (bs, n, kind))
    if kind == "zeros":
        assert not got[0][:6].any()
        assert not got[2].any() and not got[3].any()


def test_loss_weights_scale_the_loss_and_the_gradients():
    bs, n = 8, 65
    host = _inputs(bs, n, "counts")
    ref = _reference(bs, n, "counts", 0.3, 2.5)
    _compare(_raw(bs, [_dev(a) for a in host], 0.3, 2.5), ref, "weights 0.3 / 2.5")
    zero = _raw(bs, [_dev(a) for a in host], 0.0, 0.0)
    assert zero[0][0].item() == 0.0 and not zero[2].any() and not zero[3].any()


@pytest.mark.parametrize("bs", [8, 6])
def test_determinism(bs):
    """Two calls give equal bytes; a row's out_row has the same bytes at n = 65 and alone."""
    dev = [_dev(a) for a in _inputs(bs, 65, "counts")]
    a, b = _raw(bs, dev), _raw(bs, dev)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(_bits(x), _bits(y))
    big = [_dev(a) for a in _inputs(bs, 4097, "counts")]
    a, b = _raw(bs, big), _raw(bs, big)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(_bits(x), _bits(y))
    full = _raw(bs, dev)
    for r in (0, 1, 3, 5, 32, 33, 64):
        alone = _raw(bs, [x[r:r + 1].clone() for x in dev])
        assert torch.equal(_bits(alone[1][0]), _bits(full[1][r])), r


def test_python_surface_and_grads_off():
    import rvz
    bs, n = 8, 257
    host = _inputs(bs, n, "counts")
    ref = _reference(bs, n, "counts")
    z, y, pi, t, w = (_dev(a) for a in host)
    out = rvz.policy_value_loss(z, y.reshape(n, 1), pi, t.reshape(n, 1), w, rows=True)
    assert out["grad_value"].shape == (n, 1) and out["rows"].shape == (n, 3)
    _compare((out["out_loss"], out["rows"], out["grad_logits"], out["grad_value"].reshape(n)),
             ref, "python surface")
    for i, k in enumerate(("loss", "policy_loss", "value_loss", "target_entropy", "weight_sum",
                           "agreement", "malformed")):
        assert out[k].dim() == 0 and out[k].item() == out["out_loss"][i].item()
    off = rvz.policy_value_loss(z, y, pi, t, w, rows=True, grads=False)
    assert "grad_logits" not in off and "grad_value" not in off
    assert torch.equal(_bits(off["out_loss"]), _bits(out["out_loss"]))
    assert torch.equal(_bits(off["rows"]), _bits(out["rows"]))
    assert "rows" not in rvz.policy_value_loss(z, y, pi, t, w)
    # through the C-ABI: null gradients leave the buffers as they were
    raw = _raw(bs, (z, y, pi, t, w), grads=False)
    assert torch.isnan(raw[2]).all() and torch.isnan(raw[3]).all()
    assert torch.equal(_bits(raw[0]), _bits(out["out_loss"]))
    empty = rvz.policy_value_loss(z[:0], y[:0], pi[:0], t[:0])
    assert not empty["out_loss"].any() and empty["grad_logits"].shape == (0, 65)


def test_graph_capture():
    """The call captured in a torch.cuda.graph and replayed: the eager bytes, also after the
    inputs changed and changed back."""
    import rvz
    bs, n = 8, 257
    z, y, pi, t, w = (_dev(a) for a in _inputs(bs, n, "counts"))
    eager = rvz.policy_value_loss(z, y, pi, t, w, rows=True)                     # warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = rvz.policy_value_loss(z, y, pi, t, w, rows=True)
    keep = z.clone()
    z.mul_(0.5)
    graph.replay()
    assert not torch.equal(_bits(out["grad_logits"]), _bits(eager["grad_logits"]))
    z.copy_(keep)
    graph.replay()
    for k in ("out_loss", "rows", "grad_logits", "grad_value"):
        assert torch.equal(_bits(out[k]), _bits(eager[k])), k


def test_full_policy_loss_is_differentiable():
    import rvz
    bs, n = 6, 65
    z, y, pi, t, w = (_dev(a) for a in _inputs(bs, n, "counts"))
    plain = rvz.policy_value_loss(z, y, pi, t, w, 0.5, 2.0, board_size=bs)
    zg, yg = z.clone().requires_grad_(True), y.clone().reshape(n, 1).requires_grad_(True)
    loss, pl, vl, stats = rvz.full_policy_loss(zg, yg, pi, t, w, 0.5, 2.0, board_size=bs)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    assert loss.item() == plain["loss"].float().item()
    assert pl.item() == plain["policy_loss"].item() and vl.item() == plain["value_loss"].item()
    assert set(stats) == {"target_entropy", "agreement", "weight_sum", "malformed"}
    for k, v in stats.items():
        assert v.is_cuda and v.dim() == 0 and v.item() == plain[k].item(), k
    (loss * 3.0).backward()
    assert torch.equal(zg.grad, plain["grad_logits"] * 3.0)
    assert torch.equal(yg.grad, plain["grad_value"].reshape(n, 1) * 3.0)


def _soft_batch(bs=8, n=64, seed=5):
    g = torch.Generator().manual_seed(seed)
    states = (torch.rand(n, 3, bs, bs, generator=g) > 0.6).float()
    policy = torch.rand(n, bs * bs + 1, generator=g) * (torch.rand(n, bs * bs + 1,
                                                                   generator=g) < 0.3)
    policy[:, 0] += 0.01
    policy = policy / policy.sum(1, keepdim=True)
    values = torch.randint(-1, 2, (n, 1), generator=g).float()
    return {"states": states.cuda(), "policy_targets": policy.cuda(),
            "value_targets": values.cuda()}


def _net():
    import rvz
    torch.manual_seed(0)
    return rvz.AlphaZeroNetwork(8, 2, 64).cuda()


def test_trainer_full_lowers_the_policy_kl():
    from rvz.trainer import DDPTrainer
    data = _soft_batch()
    tr = DDPTrainer(_net(), policy_target="full")
    outs = [tr.train_epoch(data, seed=0) for _ in range(30)]
    for o in outs:
        assert o["steps"] == 1
        for k in ("train/loss", "train/policy_loss", "train/value_loss", "train/policy_kl",
                  "train/policy_agreement"):
            assert np.isfinite(o[k]), k
    print("policy KL", outs[0]["train/policy_kl"], "->", outs[-1]["train/policy_kl"])
    assert outs[-1]["train/policy_kl"] < outs[0]["train/policy_kl"]


def test_trainer_count_weights_of_one_are_the_unweighted_run():
    """With count_weights and counts that are all 1, the step's loss call gets float32 ones and
    returns the bytes of the unweighted call on the same logits: loss, statistics and both
    gradients, so the optimizer sees the same step. (The parameters after the step are compared
    bit for bit on the CPU, tests/test_loss_cpu.py; on the GPU the convolutions' backward
    kernels differ run to run, tests/test_gpu_pipeline.py.)"""
    import rvz
    from rvz.trainer import DDPTrainer
    data = _soft_batch()
    ones = dict(data, position_counts=torch.ones(64, dtype=torch.int32, device="cuda"))
    calls = []

    def recording(logits, value, pt, vt, weights, wp, wv, board):
        plain = rvz.policy_value_loss(logits, value, pt, vt, None, wp, wv, board)
        given = rvz.policy_value_loss(logits, value, pt, vt, weights, wp, wv, board)
        calls.append((weights, plain, given))
        return rvz.full_policy_loss(logits, value, pt, vt, weights, wp, wv, board)

    tr = DDPTrainer(_net(), policy_target="full", count_weights=True, loss_fn=recording)
    out = tr.train_epoch(ones, seed=0)
    assert out["steps"] == 1 == len(calls)
    weights, plain, given = calls[0]
    assert weights.dtype == torch.float32 and weights.shape == (64,) and bool((weights == 1).all())
    for k in ("out_loss", "grad_logits", "grad_value"):
        assert torch.equal(_bits(plain[k]), _bits(given[k])), k
    assert out["train/policy_loss"] == plain["policy_loss"].item()
    assert out["train/value_loss"] == plain["value_loss"].item()
    assert out["train/policy_kl"] == (plain["policy_loss"] - plain["target_entropy"]).item()
    # and the unweighted run itself: one step from the same net on the same batch reports the
    # same loss dict (the losses are computed before the step)
    assert DDPTrainer(_net(), policy_target="full").train_epoch(data, seed=0) == out
