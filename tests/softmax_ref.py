"""Float64 reference of the policy softmax (F.softmax(policy_logits, dim=1), mcts.py:596), the
error bound a float32 implementation is held to, and the input rows the CPU and the GPU tests
share. NumPy only: nothing here comes from rvz, so the device function policy_softmax<NSQ>
(csrc/rvz_search.hip.h) is compared with arithmetic it has no part in.

softmax_ref(z)      (p, d) float64 of float32 rows z [n, S*S+1]: m = max(z), e = exp(z - m),
                    p = e / sum(e) over all S*S+1 entries (the pass included), d = m - z. A -inf
                    entry gives p == 0 exactly (and d == inf).
bound(ref, d)       max((d + 8) * 2^-23 * ref, 2^-148) per element, 0 where d is inf; derived in
                    tests/test_softmax_ref_cpu.py.
ROW_SUM_TOL         16 * 2^-24 for |sum(p) - 1| (same place).
pool(bs)            (rows float32 [257, S*S+1], family [257]): the rows of both tests, read-only.
random_rows(...)    more rows of the random families, for the CPU test's statistics.
check_rows(...)     every assertion a softmax result has to pass on these rows; returns the
                    largest fraction of the bound reached per family.
"""
import functools

import numpy as np

EPS = 2.0 ** -23
FLOOR = 2.0 ** -148
ROW_SUM_TOL = 16 * 2.0 ** -24
SCALES = (1, 3, 10, 30)
POOL_ROWS = 257


def softmax_ref(z):
    z = np.asarray(z)
    assert z.dtype == np.float32 and z.ndim == 2
    z64 = z.astype(np.float64)
    m = z64.max(axis=1, keepdims=True)
    assert np.isfinite(m).all(), "a row needs one finite entry"
    d = m - z64
    e = np.exp(-d)
    return e / e.sum(axis=1, keepdims=True), d


def bound(ref, d):
    with np.errstate(invalid="ignore"):
        b = np.maximum((d + 8.0) * EPS * ref, FLOOR)
    return np.where(np.isinf(d), 0.0, b)


def fraction(p, ref, d):
    """|p - ref| / bound per element (0 where the bound is 0 and p is exactly ref, inf where it
    is not, inf for a NaN)."""
    err = np.abs(np.asarray(p, np.float64) - ref)
    b = bound(ref, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(f), np.inf, f)


def random_rows(bs, scale, n, seed, outlier=False):
    """n rows of N(0, scale^2) logits; with outlier, one entry of each row (any index, the pass
    included) raised by 60."""
    npol = bs * bs + 1
    rng = np.random.default_rng([bs, int(scale), seed, int(outlier)])
    z = (rng.standard_normal((n, npol)) * scale).astype(np.float32)
    if outlier:
        z[np.arange(n), rng.integers(0, npol, n)] += np.float32(60)
    return z


def _structured(bs):
    """[(family, row)]: the structured rows; the family's letter is the case of the docstring of
    tests/test_gpu_policy_softmax.py."""
    nsq = bs * bs
    npol = nsq + 1
    rng = np.random.default_rng([bs, 77])
    out = []

    def base(scale=3.0):
        return (rng.standard_normal(npol) * scale).astype(np.float32)

    def add(fam, row):
        row = np.asarray(row, np.float32)
        assert row.shape == (npol,)
        out.append((fam, row))

    # (a) the maximum at the pass, by 0.5, 5 and 50; (b) at square 0 and at the last square
    for idx, fam in ((nsq, "a_max_pass"), (0, "b_max_sq0"), (nsq - 1, "b_max_last")):
        for margin in (0.5, 5.0, 50.0):
            z = base()
            z[idx] = np.delete(z, idx).max() + np.float32(margin)
            add(fam, z)
    # (c) all entries equal
    for v in (0.0, -1e30, 3e38):
        add("c_equal", np.full(npol, v, np.float32))
    # (d) one entry 1e4 above the rest
    for idx in (0, nsq // 2 + 1, nsq - 1, nsq):
        z = base(1.0)
        z[idx] += np.float32(1e4)
        add("d_one_hot", z)
    # (e) ladders: d = 0, 10, .., 100 in a cycle from square 0, the same backwards from the pass,
    # one maximum with the cycle 10 .. 100 under it (d = 100 gives e^-100 = 3.7e-44), and two
    # fine ladders d = 80 .. 112 through the denormal range (e^-87.3 = 2^-126, e^-103.3 = 2^-149)
    i = np.arange(npol)
    add("e_ladder", -10.0 * (i % 11))
    add("e_ladder", -10.0 * ((npol - 1 - i) % 11))
    z = -10.0 * (1 + (i % 10))
    z[nsq // 3] = 0.0
    add("e_ladder", z)
    z = -(80.0 + 32.0 * i / (npol - 1))
    z[0] = 0.0
    add("e_ladder", z)
    z = -(80.0 + 32.0 * (npol - 1 - i) / (npol - 1))
    z[nsq] = 0.0
    add("e_ladder", z)
    # (f) -inf entries: one square, the pass, and every other square
    for idx in (0, nsq // 2, nsq - 1, nsq):
        z = base()
        z[idx] = -np.inf
        add("f_neg_inf", z)
    z = base()
    z[0:nsq:2] = -np.inf
    add("f_neg_inf", z)
    # (g) consecutive rows at offsets 0 and +1e4 in turn: what follows a row's S*S+1 floats in
    # memory is far larger than (or far below) anything in the row
    for k in range(8):
        add("g_alternate", base(1.0) + np.float32(1e4 * (k & 1)))
    # (h) the whole row far from 0: the result may not depend on where 0 is
    for off in (-87.0, -200.0, -1e4, 200.0):
        add("h_shifted", base(1.0) + np.float32(off))
    return out


@functools.lru_cache(maxsize=None)
def pool(bs):
    """The 257 rows: the structured ones, then 16 rows of N(0, 3^2) with a +60 outlier, then the
    random scales in turn. Both arrays are read-only."""
    st = _structured(bs)
    fam = [f for f, _ in st]
    rows = [r for _, r in st]
    rows += list(random_rows(bs, 3, 16, 5, outlier=True))
    fam += ["outlier"] * 16
    rest = POOL_ROWS - len(rows)
    per = {s: random_rows(bs, s, -(-rest // len(SCALES)), 11) for s in SCALES}
    for k in range(rest):
        s = SCALES[k % len(SCALES)]
        rows.append(per[s][k // len(SCALES)])
        fam.append(f"random_{s}")
    z = np.stack(rows).astype(np.float32)
    fam = np.array(fam)
    assert z.shape == (POOL_ROWS, bs * bs + 1)
    z.setflags(write=False)
    fam.setflags(write=False)
    return z, fam


@functools.lru_cache(maxsize=None)
def pool_ref(bs):
    """softmax_ref of pool(bs), computed once and read-only."""
    ref, d = softmax_ref(pool(bs)[0])
    ref.setflags(write=False)
    d.setflags(write=False)
    return ref, d


def check_rows(z, fam, p, what, ref_d=None):
    """Everything a float32 softmax p of the rows z has to satisfy: float32 without a NaN, the
    bound at every element, the row sum, monotonicity within a row (z_i > z_j => p_i >= p_j, and
    equal logits give equal bits), and the structured families' exact expectations. Returns
    {family: largest fraction of the bound}."""
    p = np.asarray(p)
    assert p.dtype == np.float32 and p.shape == z.shape, (what, p.dtype, p.shape)
    assert not np.isnan(p).any(), (what, "unwritten or NaN at rows", np.flatnonzero(np.isnan(p).any(1)))
    ref, d = softmax_ref(z) if ref_d is None else ref_d
    f = fraction(p, ref, d)
    worst = {k: float(f[fam == k].max()) for k in sorted(set(fam.tolist()))}
    bad = np.argwhere(f > 1.0)
    assert bad.size == 0, (what, "beyond the bound at (row, entry)", bad[:8].tolist(),
                           "fractions", f[f > 1.0][:8].tolist(), worst)
    s = p.astype(np.float64).sum(axis=1)
    assert (np.abs(s - 1.0) <= ROW_SUM_TOL).all(), \
        (what, "row sums", np.flatnonzero(np.abs(s - 1.0) > ROW_SUM_TOL)[:8].tolist(),
         float(np.abs(s - 1.0).max() / 2.0 ** -24))
    # monotonicity: along the stable order of the logits the probabilities never fall, and over
    # a run of equal logits their bits do not change
    order = np.argsort(z, axis=1, kind="stable")
    zs, ps = np.take_along_axis(z, order, 1), np.take_along_axis(p, order, 1)
    assert (np.diff(ps, axis=1) >= 0).all(), \
        (what, "not monotone in rows", np.flatnonzero((np.diff(ps, axis=1) < 0).any(1))[:8].tolist())
    with np.errstate(invalid="ignore"):       # -inf next to -inf: checked to be 0 below
        same = np.diff(zs, axis=1) == 0
    assert (np.diff(ps.view(np.int32), axis=1)[same] == 0).all(), (what, "equal logits differ")
    # exact expectations
    assert (p[np.isneginf(z)].view(np.int32) == 0).all(), (what, "-inf entry not exactly 0")
    for r in np.flatnonzero(fam == "c_equal"):
        assert np.isfinite(p[r]).all() and (p[r].view(np.int32) == p[r, :1].view(np.int32)).all(), \
            (what, "equal logits", r, p[r])
    for r in np.flatnonzero(fam == "d_one_hot"):
        top = int(np.argmax(z[r]))
        assert p[r, top] == 1.0 and not np.delete(p[r], top).any(), (what, "one-hot", r, p[r])
    lad = fam == "e_ladder"
    assert (p[lad][ref[lad] >= FLOOR] != 0).all(), (what, "a denormal result flushed to 0")
    return worst
