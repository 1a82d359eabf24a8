"""NumPy float64 reference of rvz_score_loss (include/rvz.h has the definition): a row at a time
(`row`), then the batch (`batch`), and the same through torch tensors in the result layout of
rvz.score_loss (`as_kernel`), which rvz.loss.differentiable_score turns into a score_loss_fn for
DDPTrainer on a host without a GPU.

The cumulative distribution and its mirror image are sequential np.cumsum; a row's scalar sums
are the kernel's: lane l of 64 adds its CPL = ceil(K / 64) consecutive classes lowest first, then
wave_reduce's butterfly (`wave_sum`). The cross-row sums are tests/loss_ref.py's."""
import numpy as np


def wave_sum(x):
    """rvz_wave.hip.h's wave_reduce with +: 64 values, d = 32, 16, ... 1, x = x + x[lane ^ d]."""
    x = np.asarray(x, np.float64).copy()
    assert x.shape == (64,)
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        x = x + x[lane ^ d]
    return x[0]


def row_sum(terms):
    """A row's scalar sum over its K classes: each lane's consecutive classes lowest first, then
    the butterfly."""
    K = len(terms)
    cpl = -(-K // 64)
    padded = np.zeros(64 * cpl)
    padded[:K] = terms
    lanes = padded.reshape(64, cpl)
    part = lanes[:, 0].copy()
    for i in range(1, cpl):
        part = part + lanes[:, i]
    return wave_sum(part)


def malformed(z, margin, w, nsq):
    """The malformed-row rules; NaN fails each test."""
    z = np.asarray(z, np.float32)
    t, w = np.float32(margin), np.float32(w)
    return bool(not np.isfinite(z).all() or not (-nsq <= t <= nsq) or t != np.trunc(t) or
                not (w >= 0 and np.isfinite(w)))


def row(z, margin):
    """One well-formed row: float32 inputs, float64 arithmetic. Returns a dict with c, lse, p, C,
    e, R, Qr, Lpdf, Lcdf, mean and agree."""
    z = np.asarray(z, np.float32).astype(np.float64)
    K = len(z)
    nsq = (K - 1) // 2
    c = int(np.float32(margin)) + nsq
    k = np.arange(K)
    m = z.max()
    lse = m + np.log(row_sum(np.exp(z - m)))
    p = np.exp(z - lse)
    C = np.cumsum(p)
    e = C - (k >= c)
    e[K - 1] = 0.0                                           # the last threshold is left out
    R = np.cumsum(e[::-1])[::-1]
    return {"c": c, "lse": lse, "p": p, "C": C, "e": e, "R": R, "Qr": row_sum(e * C),
            "Lpdf": lse - z[c], "Lcdf": row_sum(e * e) / (K - 1),
            "mean": row_sum(p * (k - nsq)), "agree": float(np.argmax(z) == c)}


def batch(logits, margin, weight=None, pdf_weight=1.0, cdf_weight=1.0):
    """The whole call. Returns a dict: out_loss float64 [8], rows float64 [n, 4], grad_logits
    float32 [n, K], grad64 (the same before its rounding to float32) and omega float64 [n] (each
    row's effective weight)."""
    logits = np.asarray(logits, np.float32)
    margin = np.asarray(margin, np.float32).reshape(-1)
    n, K = logits.shape
    nsq = (K - 1) // 2
    wt = np.ones(n, np.float32) if weight is None else np.asarray(weight, np.float32)
    omega, abserr = np.zeros(n), np.zeros(n)
    rows, parts = np.zeros((n, 4)), [None] * n
    bad = 0
    for r in range(n):
        if malformed(logits[r], margin[r], wt[r], nsq):
            bad += 1
            continue
        q = parts[r] = row(logits[r], margin[r])
        omega[r] = np.float64(wt[r])
        abserr[r] = abs(q["mean"] - np.float64(margin[r]))
        rows[r] = q["Lpdf"], q["Lcdf"], q["mean"], q["agree"]
    W = omega.sum()
    out = np.zeros(8)
    out[4], out[6] = W, bad
    g64 = np.zeros((n, K))
    if W > 0:
        out[1] = (omega * rows[:, 0]).sum() / W
        out[2] = (omega * rows[:, 1]).sum() / W
        out[3] = (omega * abserr).sum() / W
        out[5] = (omega * rows[:, 3]).sum() / W
        out[0] = pdf_weight * out[1] + cdf_weight * out[2]
        cw = cdf_weight * (2.0 / (K - 1))
        for r in range(n):
            q = parts[r]
            if q is None or omega[r] == 0:
                continue
            hot = (np.arange(K) == q["c"]).astype(np.float64)
            g64[r] = (omega[r] / W) * (pdf_weight * (q["p"] - hot) +
                                       cw * q["p"] * (q["R"] - q["Qr"]))
    return {"out_loss": out, "rows": rows, "grad_logits": g64.astype(np.float32), "grad64": g64,
            "omega": omega}


def longdouble_batch(logits, margin, weight=None, pdf_weight=1.0, cdf_weight=1.0):
    """An independent evaluation in np.longdouble, whole arrays at a time and plain sums (no lane
    order): out_loss [8] and rows [n, 4], longdouble. Malformed rows by `malformed`."""
    L = np.longdouble
    z32 = np.asarray(logits, np.float32)
    t32 = np.asarray(margin, np.float32).reshape(-1)
    n, K = z32.shape
    nsq = (K - 1) // 2
    wt = np.ones(n, np.float32) if weight is None else np.asarray(weight, np.float32)
    good = np.array([not malformed(z32[r], t32[r], wt[r], nsq) for r in range(n)], bool)
    z = np.where(good[:, None], z32, np.float32(0)).astype(L)
    t = np.where(good, t32, np.float32(0)).astype(L)
    w = np.where(good, wt, np.float32(0)).astype(L)
    rows = longdouble_rows(z, t) * good[:, None]
    W = w.sum()
    out = np.zeros(8, L)
    out[4], out[6] = W, (~good).sum()
    if W > 0:
        out[1] = (w * rows[:, 0]).sum() / W
        out[2] = (w * rows[:, 1]).sum() / W
        out[3] = (w * np.abs(rows[:, 2] - t) * good).sum() / W
        out[5] = (w * rows[:, 3]).sum() / W
        out[0] = L(pdf_weight) * out[1] + L(cdf_weight) * out[2]
    return {"out_loss": out, "rows": rows}


def longdouble_rows(z, t):
    """{Lpdf, Lcdf, mean, agree} of well-formed rows, longdouble [n, 4]; z longdouble [n, K] (any
    values, not only float32 ones: the finite differences move them), t the margins [n]."""
    L = np.longdouble
    n, K = z.shape
    nsq = (K - 1) // 2
    k = np.arange(K)
    c = t.astype(np.int64) + nsq
    m = z.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(axis=1))
    p = np.exp(z - lse[:, None])
    e = (np.cumsum(p, axis=1) - (k[None, :] >= c[:, None]))[:, :K - 1]
    zc = z[np.arange(n), c]
    return np.stack([lse - zc, (e * e).sum(axis=1) / L(K - 1),
                     (p * (k - nsq).astype(L)).sum(axis=1),
                     (np.argmax(z, axis=1) == c).astype(L)], axis=1)


# ---------------------------------------------------------------- the tests' shared inputs
EDGE_ROWS = 5                         # inputs' rows 0 .. 4 at n >= 65
MALFORMED = 7                         # malformed rows in inputs at n >= 65 (3 need a weight)


def edge_rows(bs):
    """The five edge rows: (logits float32 [5, K], margin float32 [5]). Row 0: c = 0; row 1:
    c = K - 1; row 2: all-equal logits (Lpdf = log K, mean = 0); row 3: +1000 at c (loss 0,
    gradient 0); row 4: +1000 at the far end, class K - 1 against c = 3
    (Lcdf = |far - c| / (K - 1))."""
    nsq = bs * bs
    K = 2 * nsq + 1
    g = np.random.default_rng(7 + bs)
    z = g.standard_normal((5, K)).astype(np.float32)
    t = np.array([-nsq, nsq, 2, -5, 3 - nsq], np.float32)
    z[2] = 0.25
    z[3, int(t[3]) + nsq] = 1000.0
    z[4, K - 1] = 1000.0
    return z, t


def inputs(bs, n, weighted):
    """The inputs of one case, host arrays, never modified: logits N(0, 1) times a per-row scale
    from {0.1, 1, 4, 10}, integer margins over the whole range, integer weights with zeros among
    them; at n >= 65 the edge rows in front and the planted malformed rows 10 .. 16 (a NaN and a
    -inf logit, margins 0.5 and S*S + 1, weights -1, inf and NaN)."""
    nsq = bs * bs
    K = 2 * nsq + 1
    g = np.random.default_rng(1000 * bs + n)
    scale = g.choice(np.array([0.1, 1.0, 4.0, 10.0]), n)
    z = (g.standard_normal((n, K)) * scale[:, None]).astype(np.float32)
    t = g.integers(-nsq, nsq + 1, n).astype(np.float32)
    w = None
    if weighted:
        w = g.integers(1, 4097, n).astype(np.float32)
        w[g.random(n) < 0.1] = 0.0
        if n == 1:
            w[0] = 3.0
    if n >= 65:
        z[:EDGE_ROWS], t[:EDGE_ROWS] = edge_rows(bs)
        if w is not None:
            w[:EDGE_ROWS] = 2.0
        z[10, 3], z[11, K - 1] = np.nan, -np.inf
        t[12], t[13] = 0.5, nsq + 1
        if w is not None:
            w[14], w[15], w[16] = -1.0, np.inf, np.nan
    for a in (z, t) + (() if w is None else (w,)):
        a.setflags(write=False)
    return z, t, w


NAMES = ("loss", "pdf_loss", "cdf_loss", "abs_error", "weight_sum", "agreement", "malformed")


def as_kernel(logits, margin, weights=None, pdf_weight=1.0, cdf_weight=1.0, board_size=8,
              rows=False, grads=True):
    """`batch` with rvz.score_loss's signature and result dict, on CPU tensors."""
    import torch
    assert logits.shape[1] == 2 * board_size * board_size + 1
    ref = batch(logits.detach().numpy(), margin.numpy(),
                None if weights is None else weights.numpy(), pdf_weight, cdf_weight)
    out_loss = torch.from_numpy(ref["out_loss"])
    out = {"out_loss": out_loss}
    out.update({k: out_loss[i] for i, k in enumerate(NAMES)})
    if rows:
        out["rows"] = torch.from_numpy(ref["rows"])
    if grads:
        out["grad_logits"] = torch.from_numpy(ref["grad_logits"])
    return out
