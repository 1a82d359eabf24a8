"""The Dirichlet sampler of the root noise (csrc/rvz_dirichlet.hip.h) through rvz.dirichlet_noise,
the stateless entry point that runs the search's own device function: the raw Philox4x32-10
blocks against a NumPy restatement of the published algorithm, the distribution against
np.random's Dirichlet, the shape of the rows, independence of the launch geometry, and the
argument errors of both entry points."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OPENING = (1 << 19) | (1 << 26) | (1 << 37) | (1 << 44)       # black's four moves at the start
K11 = sum(1 << s for s in (0, 7, 9, 18, 20, 27, 33, 42, 45, 56, 63))
EINVAL = -22


def _i64(masks):
    return torch.from_numpy(np.array(masks, np.uint64).view(np.int64)).cuda()


def _draw(masks, seeds, tags, salt, alpha, bs=8, bits=False):
    import rvz
    return rvz.dirichlet_noise(_i64(masks), torch.as_tensor(seeds, dtype=torch.int64).cuda(),
                               torch.as_tensor(tags, dtype=torch.int64).cuda().to(torch.int32),
                               salt, alpha, board_size=bs, bits=bits)


def philox4x32_10(key, ctr):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
    SC'11), restated from the paper on Python integers: 10 rounds of two 32x32 -> 64 multiplies
    and the key bumped by the Weyl constants between rounds."""
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    k0, k1 = key
    c0, c1, c2, c3 = ctr
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, \
            p0 & 0xFFFFFFFF
    return c0, c1, c2, c3


def test_philox_known_answers():
    """The restatement itself against the known-answer vectors published with the algorithm
    (Random123's kat_vectors: zeros, all ones, and the digits of pi)."""
    assert philox4x32_10((0, 0), (0, 0, 0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    f = 0xFFFFFFFF
    assert philox4x32_10((f, f), (f, f, f, f)) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert philox4x32_10((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e,
                                                    0x03707344)) == \
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


def test_raw_bits_match_philox():
    """out_bits = the attempt-0 block: key (seed32, salt), counter (0, square, tag, 0). Seeds,
    salts and tags include 0 and 0xffffffff; squares run over the whole board, 0 and S*S - 1
    included (a square is a lane index, so 0xffffffff does not exist there)."""
    rng = np.random.RandomState(5)
    seeds = [0, 0xFFFFFFFF, 1, 0x12345678] + [int(x) for x in rng.randint(0, 2 ** 32, 4, np.int64)]
    tags = [0, 0xFFFFFFFF, 4, 60] + [int(x) for x in rng.randint(0, 2 ** 32, 4, np.int64)]
    rows = [(s, t) for s in seeds for t in tags]
    sd = [s for s, _ in rows]
    tg = [t - (1 << 32) if t >> 31 else t for _, t in rows]      # the int32 bit pattern
    for bs in (8, 6):
        nsq = bs * bs
        for salt in (0, 0xFFFFFFFF, 0xDEADBEEF):
            _, bits = _draw([OPENING] * len(rows), sd, tg, salt, 0.3, bs=bs, bits=True)
            bits = bits.cpu().numpy().view(np.uint32)
            assert bits.shape == (len(rows), nsq, 4)
            for r, (s, t) in enumerate(rows):
                for sq in (0, 1, 17, nsq - 1) if r % 3 else range(nsq):
                    want = philox4x32_10((s, salt), (0, sq, t, 0))
                    assert tuple(int(x) for x in bits[r, sq]) == want, (bs, salt, s, t, sq)


def _ks(a, b):
    a, b = np.sort(a), np.sort(b)
    pts = np.concatenate([a, b])
    return np.abs(np.searchsorted(a, pts, "right") / a.size
                  - np.searchsorted(b, pts, "right") / b.size).max()


@pytest.mark.parametrize("mask", [OPENING, K11], ids=["k4", "k11"])
@pytest.mark.parametrize("alpha", [0.03, 0.3, 1.0, 3.0])
def test_distribution(alpha, mask):
    """N = 65,536 rows. Component 0 against np.random.RandomState(...).dirichlet by a two-sample
    Kolmogorov-Smirnov test, D < 1.95 sqrt(2 / N) (Smirnov's asymptotic bound at 1e-3), the
    reference rounded to float32 as the sampler's output is (at alpha = 0.03 a quarter of the
    rows has one component that is 1.0 to float32: both samples must sit on one grid, or the ties
    at 1.0 alone would make D ~ 0.25). Every component's mean within 5 standard errors of 1 / k,
    from the exact Dirichlet variance (1/k)(1 - 1/k) / (k alpha + 1)."""
    N = 65536
    k = bin(mask).count("1")
    eta = _draw([mask] * N, np.arange(N), [4] * N, 99, alpha).cpu().numpy()
    sq = [s for s in range(64) if mask >> s & 1]
    comp = eta[:, sq].astype(np.float64)
    ref = np.random.RandomState(1234).dirichlet([alpha] * k, N)[:, 0].astype(np.float32)
    ref = ref[np.isfinite(ref)]
    d = _ks(eta[:, sq[0]], ref)
    bound = 1.95 * np.sqrt(2.0 / N)
    se = np.sqrt((1 / k) * (1 - 1 / k) / (k * alpha + 1) / N)
    dev = np.abs(comp.mean(0) - 1 / k).max() / se
    print(f"alpha {alpha} k {k}: KS D = {d:.5f} (bound {bound:.5f}), worst mean {dev:.2f} SE")
    assert d < bound
    assert dev < 5.0


def test_row_shape():
    import rvz
    rng = np.random.RandomState(2)
    masks = [OPENING, K11, 0xFFFFFFFFFFFFFFFF, 1 << 63, 1, 0, 1 << 20, 0] + \
        [int(x) for x in rng.randint(0, 2 ** 62, 56, np.int64)]
    n = len(masks)
    for alpha in (0.03, 0.3, 1.0, 3.0):
        eta = _draw(masks, np.arange(n) + 7, [10] * n, 3, alpha).cpu().numpy()
        assert eta.shape == (n, 65) and np.isfinite(eta).all() and (eta >= 0).all()
        for r, m in enumerate(masks):
            legal = np.array([(m >> s) & 1 for s in range(64)], bool)
            assert not eta[r, :64][~legal].any() and eta[r, 64] == 0.0
            k = int(legal.sum())
            if k == 0:
                assert not eta[r].any()
            elif k == 1:
                assert eta[r, :64][legal][0] == 1.0
            else:
                assert abs(eta[r].astype(np.float64).sum() - 1.0) <= 1e-5
    # board 6: bits >= 36 of the mask are ignored
    eta6 = _draw([0xFFFFFFFFFFFFFFFF, 1 << 40], [1, 2], [4, 4], 0, 0.3, bs=6).cpu().numpy()
    assert eta6.shape == (2, 37) and abs(eta6[0].astype(np.float64).sum() - 1.0) <= 1e-5
    assert not eta6[1].any()
    # 2^20 rows at the reference's alpha: finite, and no rejection loop ran out of attempts
    N = 1 << 20
    lg = torch.full((N,), OPENING, dtype=torch.int64, device="cuda")
    lg[1::2] = torch.from_numpy(np.array([K11], np.uint64).view(np.int64)).cuda()
    big = rvz.dirichlet_noise(lg, torch.arange(N, device="cuda"), torch.full((N,), 4).cuda(), 11,
                              0.03)
    assert bool(torch.isfinite(big).all())
    assert float((big.double().sum(1) - 1.0).abs().max()) <= 1e-5
    rvz.Engine(1, 8, 8).check()          # the device's exhaustion bit (32) is clear


@pytest.mark.parametrize("bs", [8, 6])
def test_geometry_independence(bs):
    """Row r bitwise the same sampled alone, inside a batch of 4,097 and at another position."""
    rng = np.random.RandomState(bs)
    n = 4097
    masks = [int(x) for x in rng.randint(1, 2 ** (bs * bs - 1), n, np.int64)]
    seeds = rng.randint(0, 2 ** 32, n, np.int64)
    tags = rng.randint(4, bs * bs, n)
    full = _draw(masks, seeds, tags, 21, 0.3, bs=bs).cpu().numpy().view(np.int32)
    for r in (0, 1, 2048, 4095, 4096):
        alone = _draw(masks[r:r + 1], seeds[r:r + 1], tags[r:r + 1], 21, 0.3, bs=bs)
        assert np.array_equal(alone.cpu().numpy().view(np.int32)[0], full[r])
    perm = rng.permutation(n)
    moved = _draw([masks[i] for i in perm], seeds[perm], tags[perm], 21, 0.3, bs=bs)
    assert np.array_equal(moved.cpu().numpy().view(np.int32), full[perm])


def test_argument_errors():
    import rvz
    lib = rvz.load()
    lg, sd, tg = _i64([OPENING]), torch.zeros(1, dtype=torch.int32).cuda(), \
        torch.full((1,), 4, dtype=torch.int32).cuda()
    out = torch.zeros(65).cuda()
    args = (lg.data_ptr(), sd.data_ptr(), tg.data_ptr())
    for alpha in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        assert lib.rvz_dirichlet_noise(8, 1, *args, 0, alpha, out.data_ptr(), None,
                                       None) == EINVAL
        with pytest.raises(rvz.RvzError):
            rvz.dirichlet_noise(lg, sd, tg, 0, alpha)
    assert lib.rvz_dirichlet_noise(8, 1, *args, 0, 0.3, None, None, None) == EINVAL   # null out
    assert lib.rvz_dirichlet_noise(7, 1, *args, 0, 0.3, out.data_ptr(), None, None) == EINVAL
    assert lib.rvz_dirichlet_noise(8, -1, *args, 0, 0.3, out.data_ptr(), None, None) == EINVAL
    assert lib.rvz_dirichlet_noise(8, 0, None, None, None, 0, 0.3, None, None, None) == 0
    eng = rvz.Engine(4, 16, 8)
    h = eng._h
    for alpha, eps in ((0.0, 0.25), (-0.3, 0.25), (float("nan"), 0.25), (float("inf"), 0.25),
                       (0.3, -0.01), (0.3, 1.01), (0.3, float("nan"))):
        assert lib.rvz_search_root_noise(h, alpha, eps, 0) == EINVAL
        with pytest.raises(rvz.RvzError):
            eng.root_noise(alpha, eps)
    assert lib.rvz_search_root_noise(None, 0.3, 0.25, 0) == EINVAL
    eng.root_noise(0.3, 0.25)
    eng.root_noise(0.3, 1.0)
    eng.root_noise(0.3, 0.0)
    eng.search_begin()
    eng.root_noise(0.3, 0.25)               # before the first batch: not yet inside the search
    assert eng.search_step()
    assert lib.rvz_search_root_noise(h, 0.3, 0.25, 0) == EINVAL     # inside a search
    with pytest.raises(rvz.RvzError):
        eng.root_noise(0.3, 0.25)
    eng.check()
