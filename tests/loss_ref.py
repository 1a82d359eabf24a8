"""NumPy float64 reference of rvz_policy_value_loss (include/rvz.h has the definition): a row at
a time (`row`), then the batch (`batch`), and the same through torch tensors in the result layout
of rvz.policy_value_loss (`as_kernel`), which rvz.loss.differentiable turns into a loss_fn for
DDPTrainer on a host without a GPU."""
import numpy as np


def malformed(z, y, pi, t, w):
    """The malformed-row rules; NaN fails each test."""
    z, pi = np.asarray(z, np.float32), np.asarray(pi, np.float32)
    y, t, w = np.float32(y), np.float32(t), np.float32(w)
    return bool(not np.isfinite(z).all() or not np.isfinite(y) or
                not ((pi >= 0) & (pi <= 1)).all() or not -1 <= t <= 1 or
                not (w >= 0 and np.isfinite(w)))


def row(z, y, pi, t):
    """One well-formed row: float32 inputs, float64 arithmetic. Returns a dict with lse, logp, p,
    S, Lp, Lv, H and agree."""
    z = np.asarray(z, np.float32).astype(np.float64)
    pi = np.asarray(pi, np.float32).astype(np.float64)
    y, t = np.float64(np.float32(y)), np.float64(np.float32(t))
    m = z.max()
    lse = m + np.log(np.exp(z - m).sum())
    logp = z - lse
    pos = pi > 0
    return {"lse": lse, "logp": logp, "p": np.exp(logp), "S": pi.sum(),
            "Lp": -(pi[pos] * logp[pos]).sum(), "H": -(pi[pos] * np.log(pi[pos])).sum(),
            "Lv": (y - t) ** 2, "agree": float(np.argmax(z) == np.argmax(pi))}


def batch(logits, value, policy_target, value_target, weight=None, policy_weight=1.0,
          value_weight=1.0):
    """The whole call. Returns a dict: out_loss float64 [8], rows float64 [n, 3], grad_logits
    float32 [n, A], grad_value float32 [n], and for the tests' bounds scale (the largest |logp| of
    a well-formed row), omega float64 [n] (each row's effective weight) and agree float64 [n]."""
    logits = np.asarray(logits, np.float32)
    pt = np.asarray(policy_target, np.float32)
    value = np.asarray(value, np.float32).reshape(-1)
    vt = np.asarray(value_target, np.float32).reshape(-1)
    n, A = logits.shape
    wt = np.ones(n, np.float32) if weight is None else np.asarray(weight, np.float32)
    omega, agree = np.zeros(n), np.zeros(n)
    rows, parts = np.zeros((n, 3)), [None] * n
    bad, scale = 0, 0.0
    for r in range(n):
        if malformed(logits[r], value[r], pt[r], vt[r], wt[r]):
            bad += 1
            continue
        q = parts[r] = row(logits[r], value[r], pt[r], vt[r])
        omega[r], agree[r] = np.float64(wt[r]), q["agree"]
        rows[r] = q["Lp"], q["Lv"], q["H"]
        scale = max(scale, float(np.abs(q["logp"]).max()))
    W = omega.sum()
    out = np.zeros(8)
    out[4], out[6] = W, bad
    gl, gv = np.zeros((n, A), np.float32), np.zeros(n, np.float32)
    if W > 0:
        out[1] = (omega * rows[:, 0]).sum() / W
        out[2] = (omega * rows[:, 1]).sum() / W
        out[3] = (omega * rows[:, 2]).sum() / W
        out[5] = (omega * agree).sum() / W
        out[0] = policy_weight * out[1] + value_weight * out[2]
        for r in range(n):
            q = parts[r]
            if q is None or omega[r] == 0:
                continue
            pi = pt[r].astype(np.float64)
            gl[r] = ((policy_weight * omega[r] / W) * (q["S"] * q["p"] - pi)).astype(np.float32)
            d = np.float64(value[r]) - np.float64(vt[r])
            gv[r] = np.float32((value_weight * omega[r] / W) * 2.0 * d)
    return {"out_loss": out, "rows": rows, "grad_logits": gl, "grad_value": gv, "scale": scale,
            "omega": omega, "agree": agree}


def as_kernel(logits, value, policy_targets, value_targets, weights=None, policy_weight=1.0,
              value_weight=1.0, board_size=8, rows=False, grads=True):
    """`batch` with rvz.policy_value_loss's signature and result dict, on CPU tensors."""
    import torch
    names = ("loss", "policy_loss", "value_loss", "target_entropy", "weight_sum", "agreement",
             "malformed")
    assert logits.shape[1] == board_size * board_size + 1
    ref = batch(logits.detach().numpy(), value.detach().numpy(), policy_targets.numpy(),
                value_targets.numpy(), None if weights is None else weights.numpy(),
                policy_weight, value_weight)
    out_loss = torch.from_numpy(ref["out_loss"])
    out = {"out_loss": out_loss}
    out.update({k: out_loss[i] for i, k in enumerate(names)})
    if rows:
        out["rows"] = torch.from_numpy(ref["rows"])
    if grads:
        out["grad_logits"] = torch.from_numpy(ref["grad_logits"])
        out["grad_value"] = torch.from_numpy(ref["grad_value"]).reshape(value.shape)
    return out
