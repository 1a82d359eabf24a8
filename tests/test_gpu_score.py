"""rvz_score_loss on the device against the NumPy float64 reference (tests/score_ref.py), its
write discipline, the Python surface, replay_ownership -> score_loss in one HIP graph, and
SelfPlayTrainer(score_coef=...) end to end.

Bounds. Every out_loss / out_row entry within 1e-12 * max(1, |ref|), the project's float64
tolerance (tests/test_score_cpu.py holds the reference itself within it of a longdouble
evaluation: the reference alone stays some 50 times inside). W, the malformed count and the zero
entry are exact. A float32 gradient g is the float64 value rounded once, so
|g - ref64| <= 2^-23 |ref64| + 1e-12: one float32 rounding (2^-24, relative) plus the float64
bound on the value before it. Adjacency in float32 is not demanded: p_k (R_k - Qr) cancels, so
two correct float64 evaluations need not round to the same or to adjacent float32 numbers.
Outputs and the scratch are pre-filled (NaN, 0xFF) before every raw call, so a comparison also
shows which elements were written."""
import functools
import math

import numpy as np
import pytest
import torch

import score_ref as SR

pytestmark = pytest.mark.gpu


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64) \
        if t.dtype.is_floating_point else t


@functools.lru_cache(maxsize=None)
def _reference(bs, n, weighted):
    return SR.batch(*SR.inputs(bs, n, weighted), 1.0, 1.0)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(bs, dev, pdf=1.0, cdf=1.0, rows=True, grads=True):
    """rvz_score_loss through the C-ABI on NaN-filled outputs and a scratch of 0xFF bytes."""
    import rvz
    from rvz._lib import ptr
    lib = rvz.load()
    z, t, w = dev
    n, K = z.shape
    out = (torch.full((8,), float("nan"), dtype=torch.float64, device="cuda"),
           torch.full((n, 4), float("nan"), dtype=torch.float64, device="cuda"),
           torch.full((n, K), float("nan"), device="cuda"))
    scratch = torch.full((lib.rvz_score_loss_scratch_size(bs, n),), 0xFF, dtype=torch.uint8,
                         device="cuda")
    rc = lib.rvz_score_loss(bs, n, z.data_ptr(), t.data_ptr(),
                            None if w is None else w.data_ptr(), pdf, cdf, ptr(scratch),
                            out[0].data_ptr(), out[1].data_ptr() if rows else None,
                            out[2].data_ptr() if grads else None,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def _compare(got, ref, what):
    out_loss, rows, grad = (x.cpu().numpy() for x in got)
    assert np.isfinite(out_loss).all() and np.isfinite(rows).all() and np.isfinite(grad).all()
    e_loss = np.abs(out_loss - ref["out_loss"]) / np.maximum(1, np.abs(ref["out_loss"]))
    e_rows = np.abs(rows - ref["rows"]) / np.maximum(1, np.abs(ref["rows"]))
    g64 = ref["grad64"]
    e_grad = np.abs(grad.astype(np.float64) - g64)
    slack = e_grad - (2.0 ** -23 * np.abs(g64) + 1e-12)
    rel = (e_grad / np.maximum(np.abs(g64), 1e-300))[np.abs(g64) > 1e-6]
    print(what, "out_loss err", e_loss.max(), "rows err", e_rows.max(), "grad abs err",
          e_grad.max(), "grad rel err (|g| > 1e-6)", rel.max() if rel.size else 0.0,
          "float32 mismatches", int((grad != ref["grad_logits"]).sum()), "of", grad.size)
    assert (e_loss <= 1e-12).all(), (what, e_loss)
    assert (e_rows <= 1e-12).all(), (what, e_rows.max())
    for k in (4, 6, 7):                                      # W on integer weights, count, zero
        assert out_loss[k] == ref["out_loss"][k], (what, k)
    assert (slack <= 0).all(), (what, slack.max())


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [1, 65, 4097])
@pytest.mark.parametrize("bs", [8, 6])
def test_score_loss_against_the_reference(bs, n, weighted):
    host = SR.inputs(bs, n, weighted)
    ref = _reference(bs, n, weighted)
    if n >= 65:
        assert ref["out_loss"][6] == (SR.MALFORMED if weighted else SR.MALFORMED - 3)
        assert ref["grad_logits"].any() and not ref["grad_logits"][10:14].any()
    dev = [_dev(a) for a in host]
    got = _raw(bs, dev)
    _compare(got, ref, (bs, n, weighted))
    if n >= 65:                                              # the edge rows, as the CPU test has them
        rows, K = got[1].cpu().numpy(), 2 * bs * bs + 1
        assert abs(rows[2, 0] - math.log(K)) <= 1e-12 and abs(rows[2, 2]) <= 1e-12
        assert rows[3, 0] == 0.0 and rows[3, 1] == 0.0 and not got[2][3].any()
        assert abs(rows[4, 1] - (K - 4) / (K - 1)) <= 1e-12
        bad = [10, 11, 12, 13] + ([14, 15, 16] if weighted else [])
        assert not got[1][bad].any() and not got[2][bad].any()
    again = _raw(bs, dev)
    for x, y in zip(got, again):                             # the same bytes on every call
        assert torch.equal(_bits(x), _bits(y))
    off = _raw(bs, dev, rows=False, grads=False)
    assert torch.isnan(off[1]).all() and torch.isnan(off[2]).all()
    assert torch.equal(_bits(off[0]), _bits(got[0]))


def test_score_loss_weights_zero_weights_and_autograd():
    import rvz
    bs, n = 6, 65
    host = SR.inputs(bs, n, True)
    z, t, w = (_dev(a) for a in host)
    zero = _raw(bs, (z, t, torch.zeros_like(w)))
    assert not zero[0][:6].any() and not zero[1][:, :2].isnan().any() and not zero[2].any()
    assert zero[0][6].item() == SR.MALFORMED - 3
    ref = SR.batch(*host, 0.75, 1.5)                         # the two loss weights
    plain = rvz.score_loss(z, t, w, 0.75, 1.5, bs, rows=True)
    _compare((plain["out_loss"], plain["rows"], plain["grad_logits"]), ref, "python surface")
    for i, k in enumerate(SR.NAMES):
        assert plain[k].dim() == 0 and plain[k].item() == plain["out_loss"][i].item()
    assert set(rvz.score_loss(z, t, None, board_size=bs, grads=False)) == \
        {"out_loss", *SR.NAMES}
    none = rvz.score_loss(z[:0], t[:0], None, board_size=bs, rows=True)
    assert not none["out_loss"].any() and none["rows"].shape == (0, 4)
    assert none["grad_logits"].shape == (0, 73)
    zg = z.clone().requires_grad_(True)
    loss, stats = rvz.full_score_loss(zg, t, w, 0.75, 1.5, bs)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    assert loss.item() == plain["loss"].float().item()
    assert set(stats) == {"pdf_loss", "cdf_loss", "abs_error", "agreement", "weight_sum",
                          "malformed"}
    (loss * 3.0).backward()
    assert torch.equal(zg.grad, plain["grad_logits"] * 3.0)


def test_replay_ownership_and_score_loss_in_one_graph():
    """replay_ownership -> score_loss captured in one HIP graph and replayed twice: the eager
    bytes."""
    import rvz
    bs, nsq = 6, 36
    g = np.random.default_rng(3)
    pick = g.integers(0, 3, (50, nsq))
    fm = np.array([sum(1 << s for s in range(nsq) if pick[r, s] == 1) for r in range(50)],
                  np.uint64)
    fo = np.array([sum(1 << s for s in range(nsq) if pick[r, s] == 2) for r in range(50)],
                  np.uint64)
    fm, fo = _dev(fm.view(np.int64)), _dev(fo.view(np.int64))
    slot = torch.arange(256, dtype=torch.int32, device="cuda") % 50
    sym = torch.arange(256, dtype=torch.int32, device="cuda") % 8
    logits = _dev(SR.inputs(bs, 4097, False)[0])[100:356].contiguous()

    def calls():
        own, margin = rvz.replay_ownership(fm, fo, slot, sym, bs)
        loss = rvz.score_loss(logits, margin, None, 1.0, 1.0, bs, rows=True)
        return own, margin, loss["out_loss"], loss["rows"], loss["grad_logits"]

    eager = [x.clone() for x in calls()]
    assert eager[1].any() and eager[4].any() and eager[2][4].item() == 256
    ref = SR.batch(logits.cpu().numpy(), eager[1].cpu().numpy(), None, 1.0, 1.0)
    _compare(eager[2:], ref, "graph inputs")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = calls()
    for _ in range(2):
        for x in out:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, (x, y) in enumerate(zip(out, eager)):
            assert torch.equal(_bits(x), _bits(y)), k


def test_selfplay_trainer_with_the_score_target():
    """6x6, 64 games, 16 simulations, one 64-filter block, replay_iterations=2, score_coef=0.5:
    the metrics are there and finite, a fresh head starts at log 73, the first iteration's
    self-play records are those of a head-less copy of the net, and both coefficients work
    together."""
    import rvz
    from rvz.pipeline import SelfPlayTrainer
    kw = dict(num_simulations=16, batch_size=8, seed=5, train_steps=1, train_batch=32,
              replay_iterations=2, policy_target="full")
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(6, 1, 64, score_head=True).cuda()
    torch.manual_seed(0)
    bare = rvz.AlphaZeroNetwork(6, 1, 64).cuda()
    for k, v in bare.state_dict().items():
        assert torch.equal(v, net.state_dict()[k]), k
    with pytest.raises(ValueError, match="score"):
        SelfPlayTrainer(bare, 64, score_coef=0.5, **kw)
    spt = SelfPlayTrainer(net, 64, score_coef=0.5, **kw)
    ref = SelfPlayTrainer(bare, 64, **kw)
    ref.generate()
    want = [t.clone() for t in (ref.runner.rec_black, ref.runner.rec_white, ref.runner.rec_side,
                                ref.runner.rec_idx, ref.runner.rec_p)]
    keys = ("train/score_loss", "train/score_pdf", "train/score_cdf", "train/score_abs_error",
            "train/score_agreement")
    for it in range(2):
        out = spt.run_iteration()
        if it == 0:
            run = spt.runner
            got = (run.rec_black, run.rec_white, run.rec_side, run.rec_idx, run.rec_p)
            for a, b in zip(got, want):
                assert torch.equal(a, b)
            # one step in the iteration: its pdf is the first step's, a fresh head's
            assert abs(out["train/score_pdf"] - math.log(73)) <= 0.5, out["train/score_pdf"]
        print(it, {k: v for k, v in out.items() if "score" in k or k == "steps"})
        assert out["ownership_dropped"] == 0 and out["samples"] > 0 and out["steps"] == 1
        for k in ("train/loss", "train/policy_loss", "train/value_loss") + keys:
            assert k in out and np.isfinite(out[k]), k
        assert "train/ownership_loss" not in out
        assert out["train/score_loss"] > 0 and 0 <= out["train/score_agreement"] <= 1
        assert 0 <= out["train/score_abs_error"] <= 72
    assert spt.buffer.ownership and len(spt.buffer) > 0
    torch.manual_seed(0)
    both = rvz.AlphaZeroNetwork(6, 1, 64, ownership_head=True, score_head=True).cuda()
    two = SelfPlayTrainer(both, 64, ownership_coef=0.25, score_coef=0.5, **kw)
    out = two.run_iteration()
    for k in ("train/ownership_loss", "train/ownership_agreement") + keys:
        assert k in out and np.isfinite(out[k]), k
    assert abs(out["train/loss"] - (out["train/policy_loss"] + out["train/value_loss"] +
                                    0.25 * out["train/ownership_loss"] +
                                    0.5 * out["train/score_loss"])) <= 1e-4
