"""The final-score head without a GPU: what rvz_score_loss refuses before any HIP call, the NumPy
reference (tests/score_ref.py) against an independent np.longdouble evaluation and against finite
differences, the edge rows' exact values, the Python surface's argument checks, the network's
training-only head, and score_coef through DDPTrainer / SelfPlayTrainer on CPU tensors with the
reference in the kernel's place."""
import functools
import math

import numpy as np
import pytest
import torch

import ownership_ref as OR
import replay_ref as RR
import score_ref as SR

EINVAL = -22
CASES = [(bs, n, weighted) for bs in (8, 6) for n in (1, 65, 4097) for weighted in (False, True)]


@functools.lru_cache(maxsize=None)
def _reference(bs, n, weighted):
    return SR.batch(*SR.inputs(bs, n, weighted), 1.0, 1.0)


# ---------------------------------------------------------------- the entry point's refusals
def test_score_loss_refuses_bad_arguments_without_a_gpu():
    import rvz
    lib = rvz.load()
    q = 0x10000
    #       bs n  logits margin weight pdf cdf scratch out_loss out_row grad stream
    good = [8, 9, q, q, None, 1.0, 1.0, q, q, None, None, None]
    for k, v in ((0, 7), (0, 4), (1, -1), (1, 2 ** 31 // 129 + 1), (5, -1.0),
                 (5, float("nan")), (5, float("inf")), (6, -0.5), (6, float("inf")),
                 (2, None), (3, None), (7, None), (8, None), (7, q + 8)):
        args = list(good)
        args[k] = v
        assert lib.rvz_score_loss(*args) == EINVAL, (k, v)
    args = list(good)
    args[0], args[1] = 6, 2 ** 31 // 73 + 1
    assert lib.rvz_score_loss(*args) == EINVAL                    # 6x6: * 73 reaches 2^31
    none = list(good)
    none[1] = 0
    for k in (2, 3, 7, 8):                                        # n = 0: nothing is needed
        none[k] = None
    assert lib.rvz_score_loss(*none) == 0
    for bs in (6, 8):
        sizes = [lib.rvz_score_loss_scratch_size(bs, n) for n in (0, 1, 64, 4096, 4097, 10 ** 6)]
        assert sizes == [lib.rvz_loss_scratch_size(bs, n) for n in (0, 1, 64, 4096, 4097, 10 ** 6)]
        assert sizes == sorted(sizes) and sizes[0] >= 64
        K = 2 * bs * bs + 1
        assert lib.rvz_score_loss_scratch_size(bs, 2 ** 31 // K) > 0
        assert lib.rvz_score_loss_scratch_size(bs, 2 ** 31 // K + 1) < 0
    assert lib.rvz_score_loss_scratch_size(7, 4) < 0 and lib.rvz_score_loss_scratch_size(8, -1) < 0


def test_python_surface_checks_arguments_before_any_device_call():
    import rvz
    z, t = torch.zeros(4, 129), torch.zeros(4)
    for args in ((z.double(), t), (z, t.double()), (z[:, :128], t), (z, t[:3]), (z, t[:, None]),
                 (z.numpy(), t), (z, t, torch.ones(3)), (z, t, torch.ones(4).double())):
        with pytest.raises(rvz.RvzError, match="score_loss"):
            rvz.score_loss(*args)
    for kw in (dict(pdf_weight=-1.0), dict(cdf_weight=float("nan")), dict(pdf_weight=True),
               dict(cdf_weight=float("inf"))):
        with pytest.raises(rvz.RvzError, match="weight"):
            rvz.score_loss(z, t, **kw)
    with pytest.raises(rvz.RvzError):
        rvz.score_loss(z, t, board_size=7)
    with pytest.raises(rvz.RvzError, match="device"):             # no host fallback
        rvz.score_loss(z, t)
    with pytest.raises(rvz.RvzError, match="score_loss"):
        rvz.score_loss(torch.zeros(4, 73), t, board_size=8)


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize("bs,n,weighted", CASES)
def test_reference_against_longdouble(bs, n, weighted):
    """Every out_loss / rows entry of the float64 reference within 1e-12 * max(1, |ref|) of an
    independent np.longdouble evaluation, on the GPU tests' inputs."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("np.longdouble is no wider than float64 here: no independent reference")
    host = SR.inputs(bs, n, weighted)
    ref = _reference(bs, n, weighted)
    wide = SR.longdouble_batch(*host)
    if n >= 65:
        assert ref["out_loss"][6] == (SR.MALFORMED if weighted else SR.MALFORMED - 3)
        assert ref["grad_logits"].any() and not ref["grad_logits"][10:14].any()
        assert not ref["rows"][10:14].any()
    for name in ("out_loss", "rows"):
        want = wide[name]
        err = np.abs(ref[name].astype(np.longdouble) - want) / np.maximum(1, np.abs(want))
        print(bs, n, weighted, name, "max err", float(err.max()))
        assert np.isfinite(ref[name]).all() and (err <= 1e-12).all(), name
    for k in (4, 6, 7):                                      # W on integer weights, count, zero
        assert ref["out_loss"][k] == float(wide["out_loss"][k])
    assert np.isfinite(ref["grad64"]).all()
    # a row's gradient sums to 0 twice over: sum (p - onehot) = 0 and sum_k p_k (R_k - Qr) = 0
    assert np.abs(ref["grad64"].sum(axis=1)).max() <= 1e-12


def test_reference_gradient_against_finite_differences():
    """The reference's float64 gradient against central differences of the longdouble loss.

    The loss L(z) = sum_r (w_r / W) (a Lpdf_r + b Lcdf_r) is smooth in z; perturbing z_k of one
    row by +-h, (L(z + h) - L(z - h)) / 2h differs from dL/dz_k by at most h^2 / 6 * max |L'''|
    plus the rounding of the difference. Third derivatives in one coordinate: for Lpdf = lse - z_c
    it is p (1 - p) (1 - 2p), at most 0.1; for Lcdf, the mean over j of e_j^2 with
    e_j' = p_k ([k <= j] - C_j), |e_j| <= 1, |e_j'| <= 1, |e_j''| <= 2, |e_j'''| <= 6, so
    |(e^2)'''| = |6 e' e'' + 2 e e'''| <= 24. With a = b = 1 and w_r / W <= 1 the truncation is at
    most h^2 / 6 * 24.1 < 4.1 h^2. Rounding: L is below 1100 here (the +1000 rows) and is a sum
    of some 10^3 longdouble operations of relative error eps = 1.1e-19 each, so the difference
    carries at most about 2 * 1100 * 10^3 * eps / 2h = 1.2e-13 / h. h = 1e-5 gives
    4.1e-10 + 1.2e-8; h = 1e-4 gives 4.1e-8 + 1.2e-9. The minimum of the sum over h is near
    h = 1e-4 * 0.25; the test uses h = 2^-15 = 3.05e-5: 3.8e-9 + 3.9e-9 < 1e-8, the bound."""
    if np.finfo(np.longdouble).eps > 1.1e-19:
        pytest.fail("np.longdouble is not the 80-bit format the bound is derived for")
    h = np.longdouble(2.0 ** -15)
    for bs in (8, 6):
        z32, t32, w32 = SR.inputs(bs, 65, True)
        pick = np.array([0, 1, 2, 3, 4, 5, 20, 33, 47, 64])          # the edge rows and five more
        z32, t32, w32 = z32[pick], t32[pick], w32[pick]
        w32 = np.where(w32 > 0, w32, np.float32(1.0))
        ref = SR.batch(z32, t32, w32, 0.75, 1.5)
        n, K = z32.shape
        share = w32.astype(np.longdouble) / w32.astype(np.longdouble).sum()
        z, t = z32.astype(np.longdouble), t32.astype(np.longdouble)

        def row_losses(zz):
            rows = SR.longdouble_rows(zz, t)
            return np.longdouble(0.75) * rows[:, 0] + np.longdouble(1.5) * rows[:, 1]
        worst = 0.0
        for k in range(K):                                   # one coordinate of every row at once
            up, down = z.copy(), z.copy()
            up[:, k] += h
            down[:, k] -= h
            fd = share * (row_losses(up) - row_losses(down)) / (2 * h)
            worst = max(worst, float(np.abs(fd - ref["grad64"][:, k]).max()))
        print(bs, "largest |finite difference - gradient|", worst)
        assert worst <= 1e-8, (bs, worst)


@pytest.mark.parametrize("bs", [8, 6])
def test_reference_edge_rows(bs):
    z, t = SR.edge_rows(bs)
    nsq, K = bs * bs, 2 * bs * bs + 1
    rows = [SR.row(z[r], t[r]) for r in range(5)]
    assert rows[0]["c"] == 0 and rows[1]["c"] == K - 1
    assert (rows[0]["e"][:K - 1] <= 1e-15).all() and (rows[1]["e"] >= 0).all()  # T = 1 / T = 0
    assert abs(rows[2]["Lpdf"] - math.log(K)) <= 1e-12 and abs(rows[2]["mean"]) <= 1e-12
    assert rows[3]["Lpdf"] == 0.0 and rows[3]["Lcdf"] == 0.0 and rows[3]["agree"] == 1.0
    assert rows[3]["mean"] == t[3]
    far, c = K - 1, rows[4]["c"]
    assert c == 3 and abs(rows[4]["Lcdf"] - abs(far - c) / (K - 1)) <= 1e-12
    assert abs(rows[4]["Lpdf"] - (1000.0 - float(z[4, c]))) <= 1e-12 and rows[4]["mean"] == nsq
    out = SR.batch(z, t, None, 1.0, 1.0)
    assert not out["grad64"][3].any() and not out["grad_logits"][3].any()
    assert np.isfinite(out["out_loss"]).all() and out["out_loss"][4] == 5
    one = SR.batch(z[3:4], t[3:4], None, 1.0, 1.0)           # +1000 at c alone: loss 0
    assert one["out_loss"][:4].tolist() == [0.0, 0.0, 0.0, 0.0] and one["out_loss"][5] == 1.0
    # all weights 0, and an empty batch: zeros, no NaN
    zero = SR.batch(z, t, np.zeros(5, np.float32), 1.0, 1.0)
    assert not zero["out_loss"].any() and not zero["grad64"].any()


# ---------------------------------------------------------------- the network's head
def test_score_head_leaves_the_net_as_it_was():
    import rvz
    from rvz.network import h2_covers, pack_resnet_params
    nets = {}
    for own in (False, True):
        for score in (False, True):
            torch.manual_seed(0)
            nets[own, score] = rvz.AlphaZeroNetwork(6, 2, 64, ownership_head=own,
                                                    score_head=score).eval()
    torch.manual_seed(0)
    before = rvz.AlphaZeroNetwork(6, 2, 64)
    off = nets[False, False]
    assert list(off.state_dict()) == list(before.state_dict())
    assert not any("score" in k for k in nets[True, False].state_dict())
    new = {"score_conv.weight", "score_conv.bias", "score_fc.weight", "score_fc.bias"}
    assert set(nets[False, True].state_dict()) - set(off.state_dict()) == new
    assert set(nets[True, True].state_dict()) - set(nets[True, False].state_dict()) == new
    assert list(nets[True, True].state_dict())[-4:] == ["score_conv.weight", "score_conv.bias",
                                                        "score_fc.weight", "score_fc.bias"]
    for base, head in ((off, nets[False, True]), (nets[True, False], nets[True, True])):
        for k, v in base.state_dict().items():               # own_conv's values included
            assert torch.equal(v, head.state_dict()[k]), k
    on = nets[False, True]
    assert on.score_fc.weight.shape == (73, 72) and on.score_conv.weight.shape == (2, 64, 1, 1)
    assert not on.score_fc.bias.any() and not on.score_conv.bias.any()
    assert not on.score_fc.weight.any() and on.score_conv.weight.any()
    assert pack_resnet_params(on).numpy().tobytes() == pack_resnet_params(off).numpy().tobytes()
    assert h2_covers(on, device="cuda") == h2_covers(off, device="cuda")
    x = (torch.rand(5, 3, 6, 6) > 0.5).float()
    with torch.no_grad():
        p0, v0 = off(x)
        for key, net in nets.items():
            p, v = net(x)
            assert torch.equal(p, p0) and torch.equal(v, v0), key
            q, u = net.predict(x)
            assert torch.equal(q, p0) and torch.equal(u, v0), key
        with pytest.raises(ValueError, match="ownership_head"):
            off.forward_aux(x)
        out = nets[True, False].forward_aux(x)
        assert len(out) == 3 and out[2].shape == (5, 36)
        out = nets[False, True].forward_aux(x)
        assert len(out) == 3 and out[2].shape == (5, 73)
        both = nets[True, True].forward(x, aux=True)
        assert len(both) == 4 and both[2].shape == (5, 36) and both[3].shape == (5, 73)
        assert torch.equal(both[2], nets[True, False].forward_aux(x)[2])
        for o in (out, both):
            assert torch.equal(o[0], p0) and torch.equal(o[1], v0)


# ---------------------------------------------------------------- the trainers
def _cpu_buffer(bs, ownership=True):
    import rvz
    mover, opponent, policy, value = RR.ring(bs, 40)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int64) if a.dtype == np.uint64
                                                        else a))
    kw = dict(ownership=True, ownership_batcher=OR.as_batcher) if ownership else {}
    buf = rvz.ReplayBuffer(64, bs, "cpu", batcher=RR.batcher, **kw)
    fin = dict(final_mover=t(mover), final_opponent=t(opponent)) if ownership else {}
    buf.append(t(mover), t(opponent), t(policy), t(value), 0, **fin)
    return buf


def test_trainer_score_coef_rules_and_a_step():
    import rvz
    from rvz.loss import differentiable_ownership
    from rvz.trainer import DDPTrainer
    bs = 6
    torch.manual_seed(1)
    on = rvz.AlphaZeroNetwork(bs, 1, 64, score_head=True)
    off = rvz.AlphaZeroNetwork(bs, 1, 64)
    for model, c in ((on, 0.0), (off, 0.5)):
        with pytest.raises(ValueError, match="score"):
            DDPTrainer(model, score_coef=c)
    for c in (-1.0, True, float("nan"), "x"):
        with pytest.raises(ValueError, match="score_coef"):
            DDPTrainer(on, score_coef=c)
    for sw in ((1.0,), (1.0, -1.0), (1.0, float("inf")), 1.0, (True, 1.0)):
        with pytest.raises(ValueError, match="score_weights"):
            DDPTrainer(on, score_coef=0.5, score_weights=sw)
    buf = _cpu_buffer(bs)
    seen = []
    inner = rvz.differentiable_score(SR.as_kernel)

    def score_fn(*a):
        seen.append((a, inner(*a)))
        return seen[-1][1]
    tr = DDPTrainer(on, batch_size=16, score_coef=0.5, score_weights=(1.0, 2.0),
                    score_loss_fn=score_fn)
    w0 = on.score_fc.weight.detach().clone()
    # one step by hand: the step's loss is base + score_coef * L, exactly
    states, policy, value, _, _, own, margin = buf.sample(16, 3, 0)
    assert margin.shape == (16,) and bool((margin == margin.round()).all())
    loss, pl, vl = tr.train_step(states, policy, value, margin=margin)
    (args, (L, stats)), = seen
    assert args[1] is margin and args[2] is None and args[3:] == (1.0, 2.0, bs)
    assert args[0].shape == (16, 73) and L.dtype == torch.float32
    assert torch.equal(loss, (1.0 * pl + 1.0 * vl) + 0.5 * L.detach())
    assert L.item() == np.float32(stats["pdf_loss"].item() + 2.0 * stats["cdf_loss"].item())
    # a fresh head's output layer is zero: the uniform distribution
    assert abs(stats["pdf_loss"].item() - math.log(73)) <= 1e-12 and tr.last_score[1] is stats
    assert not torch.equal(w0, on.score_fc.weight)           # the head is trained
    out = tr.train_replay(buf, 3, seed=1)
    assert out["steps"] == 3
    keys = ("train/score_loss", "train/score_pdf", "train/score_cdf", "train/score_abs_error",
            "train/score_agreement")
    for k in ("train/loss", "train/policy_loss", "train/value_loss") + keys:
        assert np.isfinite(out[k]), k
    assert list(out)[-5:] == list(keys) and "train/ownership_loss" not in out
    assert 0.0 <= out["train/score_agreement"] <= 1.0 and out["train/score_abs_error"] >= 0
    assert abs(out["train/score_loss"] - (out["train/score_pdf"] + 2 * out["train/score_cdf"])) \
        < 1e-5
    assert abs(out["train/loss"] - (out["train/policy_loss"] + out["train/value_loss"] +
                                    0.5 * out["train/score_loss"])) < 1e-5
    with pytest.raises(ValueError, match="train_replay"):
        tr.train_epoch({"states": torch.zeros(1, 3, bs, bs)})
    with pytest.raises(ValueError, match="margin"):
        tr.train_step(states, policy, value)
    with pytest.raises(ValueError, match="margin"):
        DDPTrainer(off).train_step(states, policy, value, margin=margin)
    with pytest.raises(ValueError, match="ReplayBuffer"):
        tr.train_replay(_cpu_buffer(bs, ownership=False), 1)
    with pytest.raises(ValueError, match="ReplayBuffer"):
        DDPTrainer(off).train_replay(buf, 1)
    # both heads, both coefficients: the 4-tuple, both terms, the keys in order
    torch.manual_seed(2)
    both = rvz.AlphaZeroNetwork(bs, 1, 64, ownership_head=True, score_head=True)
    for kw in (dict(score_coef=0.5), dict(ownership_coef=0.5)):
        with pytest.raises(ValueError, match="head"):
            DDPTrainer(both, **kw)
    tb = DDPTrainer(both, batch_size=16, ownership_coef=0.25, score_coef=0.5,
                    ownership_loss_fn=differentiable_ownership(OR.as_kernel), score_loss_fn=inner)
    out = tb.train_replay(buf, 2, seed=4)
    assert list(out)[-7:] == ["train/ownership_loss", "train/ownership_agreement"] + list(keys)
    assert abs(out["train/loss"] - (out["train/policy_loss"] + out["train/value_loss"] +
                                    0.25 * out["train/ownership_loss"] +
                                    0.5 * out["train/score_loss"])) < 1e-5


def test_selfplay_trainer_score_rules():
    """The option's rules are checked before the model or the device is touched."""
    from rvz.pipeline import SelfPlayTrainer
    for kw, says in ((dict(), "replay_iterations"), (dict(replay_iterations=0), "replay_iter"),
                     (dict(replay_iterations=2, merge_positions=True), "merge_positions"),
                     (dict(replay_iterations=2, adjudicate_empties=4), "adjudicate_empties"),
                     (dict(replay_iterations=2, continuous_plies=8, merge_positions=True),
                      "merge_positions")):
        with pytest.raises(ValueError, match=says):
            SelfPlayTrainer(None, 4, score_coef=0.5, **kw)
    for c in (-0.5, True, float("inf")):
        with pytest.raises(ValueError, match="score_coef"):
            SelfPlayTrainer(None, 4, score_coef=c, replay_iterations=2)
