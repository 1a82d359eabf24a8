"""The loss on the full policy target without a GPU: the NumPy reference (tests/loss_ref.py)
against torch's float64 autograd, its edge rows, the argument rules of rvz_policy_value_loss
through the built library (checked before any HIP call), and DDPTrainer / SelfPlayTrainer's new
arguments with the reference as the injected loss_fn."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref as LR

EINVAL = -22


def _inputs(n, A=65, seed=0):
    g = np.random.default_rng(seed)
    z = (g.standard_normal((n, A)) * 3).astype(np.float32)
    y = np.tanh(g.standard_normal(n)).astype(np.float32)
    visits = g.integers(0, 30, (n, A)) * (g.random((n, A)) < 0.4)
    visits[:, 0] += 1
    pi = (visits / visits.sum(1, keepdims=True)).astype(np.float32)
    t = g.choice([-1.0, 0.0, 1.0, 0.25], n).astype(np.float32)
    return z, y, pi, t


def _torch_loss(z, y, pi, t, w, wp, wv):
    """sum_r w (wp Lp + wv Lv) / W in torch float64, differentiable in z and y."""
    logp = torch.log_softmax(z, dim=1)
    lp = -(torch.where(pi > 0, pi * logp, torch.zeros_like(logp))).sum(1)
    lv = (y - t) ** 2
    return (w * (wp * lp + wv * lv)).sum() / w.sum()


def test_one_hot_unweighted_is_cross_entropy_plus_mse():
    z, y, _, t = _inputs(37)
    arg = np.random.default_rng(1).integers(0, 65, 37)
    arg[0] = 64                                             # the pass index
    pi = np.eye(65, dtype=np.float32)[arg]
    ref = LR.batch(z, y, pi, t)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(y, dtype=torch.float64, requires_grad=True)
    pl = F.cross_entropy(zt, torch.from_numpy(arg))
    vl = F.mse_loss(yt, torch.tensor(t, dtype=torch.float64))
    (pl + vl).backward()
    assert abs(ref["out_loss"][1] - pl.item()) <= 1e-13 * max(1.0, pl.item())
    assert abs(ref["out_loss"][2] - vl.item()) <= 1e-13
    assert abs(ref["out_loss"][0] - (pl + vl).item()) <= 1e-13 * max(1.0, pl.item())
    assert ref["out_loss"][3] == 0.0 and ref["out_loss"][4] == 37 and ref["out_loss"][6] == 0
    assert np.allclose(ref["grad_logits"], zt.grad.numpy(), rtol=1e-6, atol=1e-9)
    assert np.allclose(ref["grad_value"], yt.grad.numpy(), rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("A", [65, 37])
def test_soft_weighted_gradients_are_float64_autograd(A):
    z, y, pi, t = _inputs(50, A, seed=2)
    w = np.random.default_rng(3).integers(0, 4097, 50).astype(np.float32)
    w[:3] = 0
    wp, wv = 0.7, 1.9
    ref = LR.batch(z, y, pi, t, w, wp, wv)
    f64 = [torch.tensor(a, dtype=torch.float64) for a in (z, y, pi, t, w)]
    f64[0].requires_grad_(True)
    f64[1].requires_grad_(True)
    loss = _torch_loss(*f64, wp, wv)
    loss.backward()
    assert abs(ref["out_loss"][0] - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
    assert ref["out_loss"][4] == float(w.astype(np.float64).sum())
    # float32 rounding of the reference's float64 gradient: half an ulp
    gz, gy = f64[0].grad.numpy(), f64[1].grad.numpy()
    assert np.all(np.abs(ref["grad_logits"] - gz) <= 2.0 ** -23 * np.abs(gz) + 1e-300)
    assert np.all(np.abs(ref["grad_value"] - gy) <= 2.0 ** -23 * np.abs(gy) + 1e-300)
    assert not ref["grad_logits"][:3].any() and not ref["grad_value"][:3].any()


def test_edge_rows():
    z, y, pi, t = _inputs(8, seed=4)
    pi[2] = 0.0                                             # an all-zero target row
    ref = LR.batch(z, y, pi, t)
    assert ref["rows"][2, 0] == 0.0 and ref["rows"][2, 2] == 0.0
    assert not ref["grad_logits"][2].any()
    assert ref["out_loss"][6] == 0 and ref["out_loss"][4] == 8
    # zeros of pi contribute nothing to H: H over the positive entries alone, and finite
    pos = pi[0] > 0
    assert 0 < pos.sum() < 65
    h = -(pi[0][pos].astype(np.float64) * np.log(pi[0][pos].astype(np.float64))).sum()
    assert ref["rows"][0, 2] == h and np.isfinite(ref["rows"]).all()
    # all weights 0: zeros, no NaN
    zero = LR.batch(z, y, pi, t, np.zeros(8, np.float32))
    assert not zero["out_loss"].any() and not zero["grad_logits"].any()
    assert not zero["grad_value"].any() and np.isfinite(zero["rows"]).all()


def test_each_malformed_kind_is_counted_and_zeroed():
    z, y, pi, t = _inputs(12, seed=5)
    w = np.ones(12, np.float32)
    clean = LR.batch(z, y, pi, t, w)
    z[0, 3] = np.nan
    z[1, 64] = np.inf
    y[2] = np.nan
    pi[3, 5] = -1e-3
    pi[4, 0] = 1.5
    pi[5, 7] = np.nan
    t[6] = 1.5
    t[7] = np.nan
    w[8] = -1.0
    w[9] = np.inf
    w[10] = np.nan
    ref = LR.batch(z, y, pi, t, w)
    assert ref["out_loss"][6] == 11 and ref["out_loss"][4] == 1.0
    assert not ref["rows"][:11].any() and not ref["grad_logits"][:11].any()
    assert not ref["grad_value"][:11].any()
    assert np.isfinite(ref["out_loss"]).all() and np.isfinite(ref["grad_logits"]).all()
    # the one well-formed row carries the whole mean
    assert ref["out_loss"][1] == clean["rows"][11, 0] and ref["out_loss"][2] == clean["rows"][11, 1]
    assert np.array_equal(ref["rows"][11], clean["rows"][11])


def test_argument_rules_through_the_library():
    """RVZ_EINVAL before any HIP call, so no device is needed; addresses are never dereferenced."""
    import rvz
    lib = rvz.load()
    p = 0x10000
    ok = dict(bs=8, n=4, logits=p, value=p, pt=p, vt=p, w=None, wp=1.0, wv=1.0, scratch=p,
              out=p, rows=None, gl=p, gv=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.rvz_policy_value_loss(a["bs"], a["n"], a["logits"], a["value"], a["pt"],
                                         a["vt"], a["w"], a["wp"], a["wv"], a["scratch"],
                                         a["out"], a["rows"], a["gl"], a["gv"], None)
    for bad in (dict(bs=7), dict(bs=0), dict(n=-1), dict(n=(2 ** 31) // 65 + 1),
                dict(bs=6, n=(2 ** 31) // 37 + 1), dict(wp=-1.0), dict(wp=float("inf")),
                dict(wp=float("nan")), dict(wv=-0.5), dict(wv=float("nan")),
                dict(logits=None), dict(value=None), dict(pt=None), dict(vt=None),
                dict(scratch=None), dict(out=None), dict(gl=None), dict(gv=None),
                dict(scratch=p + 8), dict(scratch=p + 4)):
        assert call(**bad) == EINVAL, bad
    # n = 0: nothing is launched or written, whatever the pointers
    assert call(n=0, logits=None, value=None, pt=None, vt=None, scratch=None, out=None,
                gl=None, gv=None) == 0
    assert call(n=0, wp=-1.0) == EINVAL
    size = lib.rvz_loss_scratch_size
    for bs in (8, 6):
        last = -1
        for n in (0, 1, 2, 63, 64, 65, 257, 4096, 4097, 10 ** 5, 2 ** 24, 2 ** 24 + 1,
                  (2 ** 31 - 1) // (bs * bs + 1)):
            s = size(bs, n)
            assert s >= last and s >= 64 * n, (bs, n, s)
            last = s
    assert size(8, -1) < 0 and size(7, 4) < 0 and size(8, (2 ** 31) // 65 + 1) < 0
    assert size(6, (2 ** 31) // 37 + 1) < 0


def test_python_surface_refuses_bad_shapes_and_dtypes():
    import rvz
    z, y = torch.zeros(4, 65), torch.zeros(4)
    pi, t = torch.zeros(4, 65), torch.zeros(4, 1)
    for bad in (dict(logits=torch.zeros(4, 64)), dict(logits=z.double()),
                dict(policy_targets=torch.zeros(3, 65)), dict(value=torch.zeros(5)),
                dict(value_targets=torch.zeros(4, 2)), dict(weights=torch.zeros(4, 1)),
                dict(weights=torch.zeros(4, dtype=torch.int32)), dict(board_size=7),
                dict(board_size=6), dict(policy_weight=-1.0), dict(value_weight=float("nan"))):
        a = dict(dict(logits=z, value=y, policy_targets=pi, value_targets=t), **bad)
        with pytest.raises(rvz.RvzError):
            rvz.policy_value_loss(**a)
    if not torch.cuda.is_available():                       # no host fallback
        with pytest.raises(rvz.RvzError):
            rvz.policy_value_loss(z, y, pi, t)


# ---- DDPTrainer / SelfPlayTrainer -----------------------------------------------------------

def _data(n=160, seed=0):
    g = torch.Generator().manual_seed(seed)
    states = (torch.rand(n, 3, 8, 8, generator=g) > 0.6).float()
    policy = torch.rand(n, 65, generator=g) * (torch.rand(n, 65, generator=g) < 0.3)
    policy[:, 0] += 0.01
    policy = policy / policy.sum(1, keepdim=True)
    values = torch.randint(-1, 2, (n, 1), generator=g).float()
    return {"states": states, "policy_targets": policy, "value_targets": values}


def _model():
    import rvz
    torch.manual_seed(0)
    return rvz.AlphaZeroNetwork(8, 1, 16)


def _ref_loss_fn():
    from rvz.loss import differentiable
    return differentiable(LR.as_kernel)


def _params_equal(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return all(torch.equal(sa[k], sb[k]) for k in sa)


def test_trainer_defaults_reproduce_a_run_without_the_new_arguments():
    from rvz.trainer import DDPTrainer
    data = _data()
    a, b = _model(), _model()
    out_a = DDPTrainer(a).train_epoch(data, seed=3)
    out_b = DDPTrainer(b, policy_target="argmax", count_weights=False,
                       loss_fn=_ref_loss_fn()).train_epoch(data, seed=3)
    assert _params_equal(a, b) and out_a == out_b
    assert set(out_a) == {"train/loss", "train/policy_loss", "train/value_loss", "train/lr",
                          "steps"}


def test_trainer_full_differs_from_argmax_and_reports_its_keys():
    from rvz.trainer import DDPTrainer
    data = _data()
    a, b = _model(), _model()
    start = copy.deepcopy(a.state_dict())
    DDPTrainer(a).train_epoch(data, seed=3, max_steps=1)
    tr = DDPTrainer(b, policy_target="full", loss_fn=_ref_loss_fn())
    out = tr.train_epoch(data, seed=3, max_steps=1)
    assert not _params_equal(a, b)
    assert any(not torch.equal(v, start[k]) for k, v in b.state_dict().items())
    assert {"train/policy_kl", "train/policy_agreement"} <= set(out) and out["steps"] == 1
    # one step: the dict is that step's reference loss on the model before the step
    m = _model().train()
    g = torch.Generator().manual_seed(3)
    torch.empty((), dtype=torch.int64).random_(generator=g)
    idx = torch.randperm(160, generator=g)[:64]
    with torch.no_grad():
        logits, v = m(data["states"][idx])
    ref = LR.batch(logits.numpy(), v.numpy(), data["policy_targets"][idx].numpy(),
                   data["value_targets"][idx].numpy())
    assert abs(out["train/policy_loss"] - ref["out_loss"][1]) <= 1e-12
    assert abs(out["train/value_loss"] - ref["out_loss"][2]) <= 1e-12
    assert abs(out["train/policy_kl"] - (ref["out_loss"][1] - ref["out_loss"][3])) <= 1e-12
    assert out["train/policy_kl"] > 0 and 0 <= out["train/policy_agreement"] <= 1
    assert out["train/policy_agreement"] == ref["out_loss"][5]


def test_trainer_count_weights():
    from rvz.trainer import DDPTrainer
    data = _data()
    tr = DDPTrainer(_model(), policy_target="full", count_weights=True, loss_fn=_ref_loss_fn())
    with pytest.raises(ValueError):
        tr.train_epoch(data, seed=1)
    with pytest.raises(ValueError):
        DDPTrainer(_model(), count_weights=True)            # argmax has no row weights
    with pytest.raises(ValueError):
        DDPTrainer(_model(), policy_target="mean")
    with pytest.raises(ValueError):
        DDPTrainer(_model()).train_step(data["states"][:8], data["policy_targets"][:8],
                                        data["value_targets"][:8], torch.ones(8))
    # counts of 1 are the unweighted run; other counts are another run
    a, b, c = _model(), _model(), _model()
    DDPTrainer(a, policy_target="full", loss_fn=_ref_loss_fn()).train_epoch(data, seed=1,
                                                                          max_steps=2)
    ones = dict(data, position_counts=torch.ones(160, dtype=torch.int32))
    DDPTrainer(b, policy_target="full", count_weights=True,
               loss_fn=_ref_loss_fn()).train_epoch(ones, seed=1, max_steps=2)
    assert _params_equal(a, b)
    many = dict(data, position_counts=torch.arange(1, 161, dtype=torch.int32))
    DDPTrainer(c, policy_target="full", count_weights=True,
               loss_fn=_ref_loss_fn()).train_epoch(many, seed=1, max_steps=2)
    assert not _params_equal(a, c)


def test_train_replay_full_mode_on_cpu():
    """train_replay in "full" mode, unweighted, through a stand-in buffer."""
    from rvz.trainer import DDPTrainer
    data = _data(64)

    class Buffer:
        def sample(self, nb, seed, step, symmetries):
            return data["states"], data["policy_targets"], data["value_targets"], None, None
    tr = DDPTrainer(_model(), policy_target="full", loss_fn=_ref_loss_fn())
    out = tr.train_replay(Buffer(), 2, seed=0)
    assert out["steps"] == 2 and np.isfinite(out["train/policy_kl"])
    assert "train/policy_kl" not in DDPTrainer(_model()).train_replay(Buffer(), 1)


def test_selfplay_trainer_refuses_forbidden_combinations():
    from rvz.pipeline import SelfPlayTrainer
    m = _model()
    for bad in (dict(policy_target="full", count_weights=True),                # no merging
                dict(policy_target="full", count_weights=True, merge_positions=True,
                     replay_iterations=2),                                     # a replay buffer
                dict(policy_target="argmax", count_weights=True, merge_positions=True),
                dict(count_weights=True, merge_positions=True),
                dict(policy_target="soft")):
        with pytest.raises(ValueError):
            SelfPlayTrainer(m, games=4, **bad)
