"""The policy/value loss on the full policy target: AlphaZero's own -pi . log p + (y - t)^2.

``merge_positions`` gives the mean search policy of every record of a position and the number of
records behind it, ``exact_policy`` the uniform distribution over the proven-optimal moves, MCTS
a visit distribution: ``policy_value_loss`` (rvz_policy_value_loss, include/rvz.h has the
definition) trains on the whole distribution, weighted per row, where the reference's criterion
keeps only its argmax. One deterministic HIP call computes the loss, its statistics and both
gradients in float64; ``full_policy_loss`` makes it a differentiable torch function, which
``DDPTrainer(policy_target="full")`` uses.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import _lib
from ._lib import RvzError, check, is_number, ptr

OUT_LOSS = ("loss", "policy_loss", "value_loss", "target_entropy", "weight_sum", "agreement",
            "malformed")        # out_loss[0 .. 7); out_loss[7] is 0


def _addr(t: Optional[torch.Tensor]):
    """Device address of a contiguous device tensor (the loss kernels read and write single
    dwords, so only the scratch needs ptr()'s 16-byte alignment)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RvzError("rvz buffers must be device tensors (no host fallback)")
    return t.data_ptr()


def check_loss_args(logits, value, policy_targets, value_targets, weights, policy_weight,
                    value_weight, board_size) -> int:
    """The shape, dtype and weight rules of policy_value_loss, checked before any device call;
    returns n."""
    _lib.check_board_size(board_size)
    npol = board_size * board_size + 1
    for name, t in (("logits", logits), ("value", value), ("policy_targets", policy_targets),
                    ("value_targets", value_targets)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise RvzError(f"policy_value_loss: {name} must be a float32 tensor")
    if logits.dim() != 2 or logits.shape[1] != npol:
        raise RvzError(f"policy_value_loss: logits must be [n, {npol}]")
    n = logits.shape[0]
    if policy_targets.shape != (n, npol):
        raise RvzError(f"policy_value_loss: policy_targets must be [n, {npol}]")
    for name, t in (("value", value), ("value_targets", value_targets)):
        if t.shape not in ((n,), (n, 1)):
            raise RvzError(f"policy_value_loss: {name} must be [n] or [n, 1]")
    if weights is not None and (not isinstance(weights, torch.Tensor) or
                                weights.dtype != torch.float32 or weights.shape != (n,)):
        raise RvzError("policy_value_loss: weights must be None or float32 [n]")
    if n * npol >= 2 ** 31:
        raise RvzError("policy_value_loss: n * (S*S + 1) does not fit int32")
    for name, x in (("policy_weight", policy_weight), ("value_weight", value_weight)):
        if not is_number(x, 0.0, math.inf, hi_open=True):
            raise RvzError(f"policy_value_loss: {name} must be a finite number >= 0, not {x!r}")
    return n


def policy_value_loss(logits: torch.Tensor, value: torch.Tensor, policy_targets: torch.Tensor,
                      value_targets: torch.Tensor, weights: Optional[torch.Tensor] = None,
                      policy_weight: float = 1.0, value_weight: float = 1.0, board_size: int = 8,
                      rows: bool = False, grads: bool = True) -> Dict[str, torch.Tensor]:
    """rvz_policy_value_loss: the weighted loss of a batch on its full policy targets, with its
    gradients, in float64 (include/rvz.h has the definition). logits and policy_targets float32
    [n, S*S+1], value (the net's tanh output) and value_targets float32 [n] or [n, 1], weights
    None (every row 1) or float32 [n], device tensors. Returns a dict of device tensors: "out_loss"
    float64 [8] and 0-d views of its entries "loss" (policy_weight * P + value_weight * V),
    "policy_loss" P, "value_loss" V, "target_entropy", "weight_sum" W, "agreement" and
    "malformed" (the rows dropped with weight 0: a non-finite logit or value, a target out of
    range, a negative or non-finite weight); with rows=True "rows" float64 [n, 3], each row's
    {Lp, Lv, H}; with grads=True "grad_logits" float32 [n, S*S+1] and "grad_value" float32 in
    value's shape, the derivatives of "loss". The call runs on the current stream, allocates its
    scratch and outputs, and never synchronises with the host; n = 0 launches nothing and
    returns zeros."""
    n = check_loss_args(logits, value, policy_targets, value_targets, weights, policy_weight,
                        value_weight, board_size)
    lib = _lib.load()
    dev = logits.device
    z = logits.detach().contiguous()
    y = value.detach().reshape(n).contiguous()
    pi = policy_targets.detach().to(dev).contiguous()
    t = value_targets.detach().to(dev).reshape(n).contiguous()
    w = None if weights is None else weights.detach().to(dev).contiguous()
    f64 = {"dtype": torch.float64, "device": dev}
    out_loss = torch.empty(8, **f64) if n else torch.zeros(8, **f64)
    out = {"out_loss": out_loss}
    out.update({name: out_loss[i] for i, name in enumerate(OUT_LOSS)})
    if rows:
        out["rows"] = torch.empty(n, 3, **f64)
    if grads:
        out["grad_logits"] = torch.empty(n, logits.shape[1], dtype=torch.float32, device=dev)
        out["grad_value"] = torch.empty(value.shape, dtype=torch.float32, device=dev)
    if n:
        size = lib.rvz_loss_scratch_size(board_size, n)
        if size < 0:
            raise RvzError(f"policy_value_loss: no scratch for n = {n}")
        scratch = torch.empty(size, dtype=torch.uint8, device=dev)
        check(lib.rvz_policy_value_loss(board_size, n, _addr(z), _addr(y), _addr(pi), _addr(t),
                                        _addr(w), float(policy_weight), float(value_weight),
                                        ptr(scratch), _addr(out_loss), _addr(out.get("rows")),
                                        _addr(out.get("grad_logits")), _addr(out.get("grad_value")),
                                        _lib.stream_handle(dev)), None, "rvz_policy_value_loss")
    return out


class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, value, kernel, args, rows=False):
        out = kernel(logits.detach(), value.detach(), *args, rows=rows, grads=True)
        ctx.save_for_backward(out["grad_logits"], out["grad_value"])
        ctx.shapes = (logits.shape, value.shape)
        return out["loss"].to(logits.dtype)

    @staticmethod
    def backward(ctx, grad_output):
        gl, gv = ctx.saved_tensors
        g = grad_output.to(gl.dtype)
        return (g * gl).reshape(ctx.shapes[0]), (g * gv).reshape(ctx.shapes[1]), None, None, None


def differentiable(kernel):
    """A function of full_policy_loss's signature around any `kernel` of policy_value_loss's
    signature and results (tests on a host without a GPU wrap the NumPy reference). rows=True:
    the kernel is asked for its per-row output and stats["rows"] holds it."""
    def loss_fn(logits, value, policy_targets, value_targets, weights=None, policy_weight=1.0,
                value_weight=1.0, board_size=8, rows: bool = False):
        holder = {}

        def call(*a, **k):
            holder["out"] = kernel(*a, **k)
            return holder["out"]
        args = (policy_targets, value_targets, weights, policy_weight, value_weight, board_size)
        loss = (_Loss.apply(logits, value, call, args, True) if rows else
                _Loss.apply(logits, value, call, args))
        out = holder["out"]
        stats = {k: out[k] for k in ("target_entropy", "agreement", "weight_sum", "malformed")}
        if rows:
            stats["rows"] = out["rows"]
        return loss, out["policy_loss"], out["value_loss"], stats
    return loss_fn


_full = differentiable(policy_value_loss)


def full_policy_loss(logits: torch.Tensor, value: torch.Tensor, policy_targets: torch.Tensor,
                     value_targets: torch.Tensor, weights: Optional[torch.Tensor] = None,
                     policy_weight: float = 1.0, value_weight: float = 1.0, board_size: int = 8,
                     rows: bool = False):
    """policy_value_loss as a differentiable torch function (one rvz_policy_value_loss call in
    the forward, which also computes the gradients; the backward multiplies the saved gradients
    by the upstream factor). Returns (loss, policy_loss, value_loss, stats): loss a 0-d tensor of
    logits' dtype, differentiable with respect to logits and value; policy_loss and value_loss
    the weighted means P and V, 0-d float64; stats the 0-d float64 device tensors
    "target_entropy", "agreement", "weight_sum" and "malformed", and with rows=True "rows", the
    float64 [n, 3] tensor of each row's {Lp, Lv, H} (what rvz.replay_priority reads). Nothing
    synchronises with the host."""
    if rows:
        return _full(logits, value, policy_targets, value_targets, weights, policy_weight,
                     value_weight, board_size, rows=True)
    return _full(logits, value, policy_targets, value_targets, weights, policy_weight,
                 value_weight, board_size)


# ------------------------------------------------------------------ the ownership loss
OWN_LOSS = {"loss": 0, "weight_sum": 4, "agreement": 5, "malformed": 6}    # out_loss's entries


def check_ownership_loss_args(logits, targets, weights, board_size) -> int:
    """The shape and dtype rules of ownership_loss, checked before any device call; returns n."""
    _lib.check_board_size(board_size)
    nsq = board_size * board_size
    for name, t in (("logits", logits), ("targets", targets)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise RvzError(f"ownership_loss: {name} must be a float32 tensor")
    if logits.dim() != 2 or logits.shape[1] != nsq:
        raise RvzError(f"ownership_loss: logits must be [n, {nsq}]")
    n = logits.shape[0]
    if targets.shape != (n, nsq):
        raise RvzError(f"ownership_loss: targets must be [n, {nsq}]")
    if weights is not None and (not isinstance(weights, torch.Tensor) or
                                weights.dtype != torch.float32 or weights.shape != (n,)):
        raise RvzError("ownership_loss: weights must be None or float32 [n]")
    if n * (nsq + 1) >= 2 ** 31:
        raise RvzError("ownership_loss: n * (S*S + 1) does not fit int32")
    return n


def ownership_loss(logits: torch.Tensor, targets: torch.Tensor,
                   weights: Optional[torch.Tensor] = None, board_size: int = 8,
                   rows: bool = False, grads: bool = True) -> Dict[str, torch.Tensor]:
    """rvz_ownership_loss: the weighted loss of an ownership head on a batch's final-ownership
    targets, mean_a (tanh(o_a) - t_a)^2 per row, with its gradient, in float64 (include/rvz.h has
    the definition). logits and targets float32 [n, S*S] (targets: replay_ownership's, every
    entry -1, 0 or +1), weights None (every row 1) or float32 [n], device tensors. Returns a dict
    of device tensors: "out_loss" float64 [8] and 0-d views of its entries "loss", "weight_sum",
    "agreement" (the weighted mean over rows of the share of the owned squares whose logit has
    the owner's sign) and "malformed" (the rows dropped with weight 0: a non-finite logit, a
    target that is not -1, 0 or +1, a negative or non-finite weight); with rows=True "rows"
    float64 [n, 2], each row's {L, agree}; with grads=True "grad_logits" float32 [n, S*S], the
    derivative of "loss". The call runs on the current stream, allocates its scratch and outputs,
    and never synchronises with the host; n = 0 launches nothing and returns zeros."""
    n = check_ownership_loss_args(logits, targets, weights, board_size)
    lib = _lib.load()
    dev = logits.device
    o = logits.detach().contiguous()
    t = targets.detach().to(dev).contiguous()
    w = None if weights is None else weights.detach().to(dev).contiguous()
    f64 = {"dtype": torch.float64, "device": dev}
    out_loss = torch.empty(8, **f64) if n else torch.zeros(8, **f64)
    out = {"out_loss": out_loss}
    out.update({name: out_loss[i] for name, i in OWN_LOSS.items()})
    if rows:
        out["rows"] = torch.empty(n, 2, **f64)
    if grads:
        out["grad_logits"] = torch.empty(n, logits.shape[1], dtype=torch.float32, device=dev)
    if n:
        size = lib.rvz_ownership_loss_scratch_size(board_size, n)
        if size < 0:
            raise RvzError(f"ownership_loss: no scratch for n = {n}")
        scratch = torch.empty(size, dtype=torch.uint8, device=dev)
        check(lib.rvz_ownership_loss(board_size, n, _addr(o), _addr(t), _addr(w), ptr(scratch),
                                     _addr(out_loss), _addr(out.get("rows")),
                                     _addr(out.get("grad_logits")), _lib.stream_handle(dev)),
              None, "rvz_ownership_loss")
    return out


class _OwnLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, kernel, args):
        out = kernel(logits.detach(), *args, grads=True)
        ctx.save_for_backward(out["grad_logits"])
        ctx.shape = logits.shape
        return out["loss"].to(logits.dtype)

    @staticmethod
    def backward(ctx, grad_output):
        (gl,) = ctx.saved_tensors
        return (grad_output.to(gl.dtype) * gl).reshape(ctx.shape), None, None


def differentiable_ownership(kernel):
    """A function of full_ownership_loss's signature around any `kernel` of ownership_loss's
    signature and results (tests on a host without a GPU wrap the NumPy reference)."""
    def loss_fn(logits, targets, weights=None, board_size=8):
        holder = {}

        def call(*a, **k):
            holder["out"] = kernel(*a, **k)
            return holder["out"]
        loss = _OwnLoss.apply(logits, call, (targets, weights, board_size))
        out = holder["out"]
        return loss, {k: out[k] for k in ("agreement", "weight_sum", "malformed")}
    return loss_fn


_full_own = differentiable_ownership(ownership_loss)


def full_ownership_loss(logits: torch.Tensor, targets: torch.Tensor,
                        weights: Optional[torch.Tensor] = None, board_size: int = 8):
    """ownership_loss as a differentiable torch function (one rvz_ownership_loss call in the
    forward, which also computes the gradient; the backward multiplies the saved gradient by the
    upstream factor). Returns (loss, stats): loss a 0-d tensor of logits' dtype, differentiable
    with respect to logits; stats the 0-d float64 device tensors "agreement", "weight_sum" and
    "malformed". Nothing synchronises with the host."""
    return _full_own(logits, targets, weights, board_size)


# ------------------------------------------------------------------ the score loss
SCORE_LOSS = ("loss", "pdf_loss", "cdf_loss", "abs_error", "weight_sum", "agreement",
              "malformed")      # out_loss[0 .. 7); out_loss[7] is 0


def check_score_loss_args(logits, margin, weights, pdf_weight, cdf_weight, board_size) -> int:
    """The shape, dtype and weight rules of score_loss, checked before any device call; returns
    n."""
    _lib.check_board_size(board_size)
    k = 2 * board_size * board_size + 1
    for name, t in (("logits", logits), ("margin", margin)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise RvzError(f"score_loss: {name} must be a float32 tensor")
    if logits.dim() != 2 or logits.shape[1] != k:
        raise RvzError(f"score_loss: logits must be [n, {k}]")
    n = logits.shape[0]
    if margin.shape != (n,):
        raise RvzError("score_loss: margin must be [n]")
    if weights is not None and (not isinstance(weights, torch.Tensor) or
                                weights.dtype != torch.float32 or weights.shape != (n,)):
        raise RvzError("score_loss: weights must be None or float32 [n]")
    if n * k >= 2 ** 31:
        raise RvzError("score_loss: n * (2*S*S + 1) does not fit int32")
    for name, x in (("pdf_weight", pdf_weight), ("cdf_weight", cdf_weight)):
        if not is_number(x, 0.0, math.inf, hi_open=True):
            raise RvzError(f"score_loss: {name} must be a finite number >= 0, not {x!r}")
    return n


def score_loss(logits: torch.Tensor, margin: torch.Tensor,
               weights: Optional[torch.Tensor] = None, pdf_weight: float = 1.0,
               cdf_weight: float = 1.0, board_size: int = 8, rows: bool = False,
               grads: bool = True) -> Dict[str, torch.Tensor]:
    """rvz_score_loss: the weighted loss of a final-score head on a batch's final disc margins,
    with its gradient, in float64 (include/rvz.h has the definition). logits float32
    [n, 2*S*S+1], class k the margin k - S*S from the mover's side; margin float32 [n]
    (replay_ownership's, ReplayBuffer(ownership=True).sample's: an integer in [-S*S, S*S]);
    weights None (every row 1) or float32 [n]; device tensors. Returns a dict of device tensors:
    "out_loss" float64 [8] and 0-d views of its entries "loss" (pdf_weight * P + cdf_weight * Q),
    "pdf_loss" P (the cross-entropy of the margin's class), "cdf_loss" Q (the mean squared
    distance of the cumulative distributions), "abs_error" (the weighted mean of |the
    distribution's mean - margin|, in discs), "weight_sum" W, "agreement" (the weighted share of
    rows whose first largest logit is the margin's class) and "malformed" (the rows dropped with
    weight 0: a non-finite logit, a margin that is no integer in range, a negative or non-finite
    weight); with rows=True "rows" float64 [n, 4], each row's {Lpdf, Lcdf, mean, agree}; with
    grads=True "grad_logits" float32 [n, 2*S*S+1], the derivative of "loss". The call runs on the
    current stream, allocates its scratch and outputs, and never synchronises with the host;
    n = 0 launches nothing and returns zeros."""
    n = check_score_loss_args(logits, margin, weights, pdf_weight, cdf_weight, board_size)
    lib = _lib.load()
    dev = logits.device
    z = logits.detach().contiguous()
    t = margin.detach().to(dev).contiguous()
    w = None if weights is None else weights.detach().to(dev).contiguous()
    f64 = {"dtype": torch.float64, "device": dev}
    out_loss = torch.empty(8, **f64) if n else torch.zeros(8, **f64)
    out = {"out_loss": out_loss}
    out.update({name: out_loss[i] for i, name in enumerate(SCORE_LOSS)})
    if rows:
        out["rows"] = torch.empty(n, 4, **f64)
    if grads:
        out["grad_logits"] = torch.empty(n, logits.shape[1], dtype=torch.float32, device=dev)
    if n:
        size = lib.rvz_score_loss_scratch_size(board_size, n)
        if size < 0:
            raise RvzError(f"score_loss: no scratch for n = {n}")
        scratch = torch.empty(size, dtype=torch.uint8, device=dev)
        check(lib.rvz_score_loss(board_size, n, _addr(z), _addr(t), _addr(w), float(pdf_weight),
                                 float(cdf_weight), ptr(scratch), _addr(out_loss),
                                 _addr(out.get("rows")), _addr(out.get("grad_logits")),
                                 _lib.stream_handle(dev)), None, "rvz_score_loss")
    return out


def differentiable_score(kernel):
    """A function of full_score_loss's signature around any `kernel` of score_loss's signature
    and results (tests on a host without a GPU wrap the NumPy reference)."""
    def loss_fn(logits, margin, weights=None, pdf_weight=1.0, cdf_weight=1.0, board_size=8):
        holder = {}

        def call(*a, **k):
            holder["out"] = kernel(*a, **k)
            return holder["out"]
        loss = _OwnLoss.apply(logits, call, (margin, weights, pdf_weight, cdf_weight, board_size))
        out = holder["out"]
        return loss, {k: out[k] for k in ("pdf_loss", "cdf_loss", "abs_error", "agreement",
                                          "weight_sum", "malformed")}
    return loss_fn


_full_score = differentiable_score(score_loss)


def full_score_loss(logits: torch.Tensor, margin: torch.Tensor,
                    weights: Optional[torch.Tensor] = None, pdf_weight: float = 1.0,
                    cdf_weight: float = 1.0, board_size: int = 8):
    """score_loss as a differentiable torch function (one rvz_score_loss call in the forward,
    which also computes the gradient; the backward multiplies the saved gradient by the upstream
    factor). Returns (loss, stats): loss a 0-d tensor of logits' dtype, differentiable with
    respect to logits; stats the 0-d float64 device tensors "pdf_loss", "cdf_loss", "abs_error",
    "agreement", "weight_sum" and "malformed". Nothing synchronises with the host."""
    return _full_score(logits, margin, weights, pdf_weight, cdf_weight, board_size)
