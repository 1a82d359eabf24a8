"""The bound that tests/test_gpu_policy_softmax.py holds the device softmax to, checked without a
GPU against two float32 softmaxes that are not the project's.

Per element, with ref the float64 softmax of the float32 logits and d = max(z) - z:

    |p - ref| <= max((d + 8) * 2^-23 * ref, 2^-148)

Derivation, for p computed in float32 as max, subtract, expf, sum, divide:
  * the subtraction z - m is rounded once: an absolute error <= d * 2^-24 of the exponent, which
    is that relative error of the exponential;
  * expf is within 1 ulp, a relative 2^-23 (the HIP math API's documented bound for expf);
  * the sum of <= 65 non-negative terms through a log-depth reduction (6 levels) plus the pass
    add takes <= 7 roundings of 2^-24 each, and no cancellation: a relative 7 * 2^-24;
  * the division is correctly rounded: 2^-24;
  * together <= (d/2 + 1 + 3.5 + 0.5) * 2^-23 = (d/2 + 5) * 2^-23; (d + 8) * 2^-23 leaves a
    margin of 1.6 (d = 0) to 2 (large d);
  * the absolute floor is two roundings to a float32 denormal (spacing 2^-149): the
    exponential's and the quotient's. With one (2^-149) torch's CPU softmax reaches 1.26 on
    denormal results, so the floor is 2^-148.
A -inf logit gives exactly 0 (exp(-inf) is 0 in every format), so there the bound is 0.

Row sum, in float64: |sum(p) - 1| <= 16 * 2^-24. Every p_i is e_i / s rounded once, and s is the
rounded sum of the e_i: one division rounding plus <= 7 sum roundings is 8 * 2^-24, and 16
leaves a margin of 2.

Neither figure is taken from what the kernel returns. Fractions of the bound reached here
(257-row pools and 20,000 rows per board, scale and outlier setting): printed by the tests."""
import numpy as np
import pytest
import torch

import softmax_ref as S

BOARDS = (8, 6)


def numpy_f32_softmax(z):
    """The float32 restatement, every step rounded on its own: the maximum, the subtraction,
    exp, a log-depth sum of the squares (halving, 6 levels) plus the pass, the division."""
    z = np.asarray(z, np.float32)
    n, npol = z.shape
    m = z.max(axis=1, keepdims=True)
    with np.errstate(under="ignore"):
        e = np.exp((z - m).astype(np.float32)).astype(np.float32)
        t = np.zeros((n, 64), np.float32)
        t[:, :npol - 1] = e[:, :npol - 1]
        while t.shape[1] > 1:
            h = t.shape[1] // 2
            t = (t[:, :h] + t[:, h:]).astype(np.float32)
        s = (t + e[:, npol - 1:]).astype(np.float32)
        return (e / s).astype(np.float32)


def torch_f32_softmax(z):
    return torch.softmax(torch.from_numpy(np.array(z, np.float32)), 1).numpy()


IMPLS = {"numpy-f32": numpy_f32_softmax, "torch-f32": torch_f32_softmax}


@pytest.mark.parametrize("bs", BOARDS)
@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_float32_softmax_within_bound_on_pool(bs, impl):
    """The rows the GPU test uses: both float32 references pass every check the kernel has to
    pass (bound, row sum, monotonicity, the exact expectations of the structured rows)."""
    z, fam = S.pool(bs)
    worst = S.check_rows(z, fam, IMPLS[impl](z), (impl, bs), S.pool_ref(bs))
    print(f"{bs}x{bs} {impl} pool: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("bs", BOARDS)
def test_float32_softmax_within_bound_statistics(bs):
    """20,000 rows per scale, with and without a +60 outlier: the largest fraction of the bound
    each float32 reference reaches, overall and on normal-range results, and the largest row-sum
    error in units of 2^-24."""
    for scale in S.SCALES:
        for outlier in (False, True):
            z = S.random_rows(bs, scale, 20000, 3, outlier)
            ref, d = S.softmax_ref(z)
            line = []
            for name in sorted(IMPLS):
                p = IMPLS[name](z)
                f = S.fraction(p, ref, d)
                normal = ref >= 2.0 ** -126
                rs = np.abs(p.astype(np.float64).sum(1) - 1.0).max() / 2.0 ** -24
                line.append(f"{name} {f.max():.2f} (normal range {f[normal].max():.2f}, "
                            f"row sum {rs:.1f} * 2^-24)")
                assert f.max() <= 1.0, (bs, scale, outlier, name, float(f.max()))
                assert rs <= 16, (bs, scale, outlier, name, float(rs))
            print(f"{bs}x{bs} scale {scale}{' +60 outlier' if outlier else ''}: "
                  + "; ".join(line))


@pytest.mark.parametrize("bs", BOARDS)
def test_reference_equals_torch_float64(bs):
    """softmax_ref against torch.softmax of the same logits in float64: within 1e-15, -inf
    entries exactly 0, rows summing to 1."""
    z, _ = S.pool(bs)
    ref, d = S.pool_ref(bs)
    t = torch.softmax(torch.from_numpy(z.copy()).double(), 1).numpy()
    assert np.abs(ref - t).max() <= 1e-15, float(np.abs(ref - t).max())
    assert (ref[np.isneginf(z)] == 0).all() and np.isinf(d[np.isneginf(z)]).all()
    assert np.abs(ref.sum(1) - 1.0).max() <= 1e-15
    assert (d >= 0).all() and (d.min(axis=1) == 0).all()


@pytest.mark.parametrize("bs", BOARDS)
def test_pool_is_what_the_gpu_test_needs(bs):
    """The pool's shape, its families, and that its cases are the ones named: a maximum at the
    pass, at square 0 and at the last square; float32 denormal results in the ladders, some of
    them at or above the floor; rows are read-only."""
    z, fam = S.pool(bs)
    ref, _ = S.pool_ref(bs)
    nsq = bs * bs
    assert z.shape == (S.POOL_ROWS, nsq + 1) and z.dtype == np.float32
    assert not z.flags.writeable and not ref.flags.writeable
    for k, idx in (("a_max_pass", nsq), ("b_max_sq0", 0), ("b_max_last", nsq - 1)):
        assert (z[fam == k].argmax(1) == idx).all()
    for s in S.SCALES:
        assert (fam == f"random_{s}").sum() >= 40
    lad = ref[fam == "e_ladder"]
    den = (lad > 0) & (lad < 2.0 ** -126)
    assert den.sum() >= 20 and (lad[den] >= S.FLOOR).sum() >= 10 and (lad[den] < S.FLOOR).any()
    assert np.isneginf(z[fam == "f_neg_inf"]).any(1).all()
    assert not np.isnan(z).any() and np.isfinite(z.max(1)).all()
