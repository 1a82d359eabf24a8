"""rvz_merge_positions on the GPU, bit for bit against the NumPy reference (tests/merge_ref.py):
sizes across wave, workgroup and scan-block edges, one group under maximal contention, the
identity on distinct rows, long probe chains, determinism across runs and streams, malformed
rows, graph capture, and SelfPlayTrainer(merge_positions=True) end to end. The four per-position
outputs are pre-filled with a sentinel before every raw call, so a comparison also shows that the
rows below m were written and the rows from m on were not."""
import numpy as np
import pytest
import torch

import merge_ref as M

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 1023, 1025, 4097, 70001)
SENTINEL = -77


def _dev(rows):
    """Device (black, white, status, policy, value) of the reference's (b, w, side, pol, val)."""
    b, w, s, pol, val = rows
    status = np.zeros((len(b), 4), np.int32)
    status[:, 0], status[:, 2] = s, -1
    return (torch.from_numpy(np.ascontiguousarray(b).view(np.int64)).cuda(),
            torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).cuda(),
            torch.from_numpy(status).cuda(), torch.from_numpy(np.ascontiguousarray(pol)).cuda(),
            torch.from_numpy(np.ascontiguousarray(val)).cuda())


def _outputs(bs, n):
    return {"m": torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda"),
            "first": torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda"),
            "count": torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda"),
            "policy": torch.full((n, bs * bs + 1), float(SENTINEL), device="cuda"),
            "value": torch.full((n,), float(SENTINEL), device="cuda"),
            "group": torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")}


def _raw(bs, dev, table_log2=0, stream=None, out=None, scratch=None):
    """rvz_merge_positions through the C-ABI on pre-filled outputs and a scratch full of junk."""
    import rvz
    from rvz._lib import ptr
    lib = rvz.load()
    n = dev[0].numel()
    if out is None:
        out = _outputs(bs, n)
    if scratch is None:
        size = lib.rvz_merge_scratch_size(bs, n, table_log2)
        assert size > 0
        scratch = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    rc = lib.rvz_merge_positions(bs, n, *[ptr(t) for t in dev], table_log2, ptr(scratch),
                                 *[ptr(out[k]) for k in ("m", "first", "count", "policy", "value",
                                                         "group")], stream)
    assert rc == 0, rc
    return out


def _assert_equal(got, want, n):
    """Every output against the reference's: bit for bit below m, untouched from m on."""
    m = int(got["m"][0])
    assert m == want["m"]
    for k in ("first", "count", "policy", "value"):
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype, k
        assert g[:m].tobytes() == want[k].tobytes(), k
        assert (g[m:] == SENTINEL).all(), k
    assert np.array_equal(got["group"].cpu().numpy(), want["group"])
    first, group = want["first"], want["group"]
    assert (np.diff(first) > 0).all() and np.array_equal(group[first], np.arange(m))
    assert int(got["count"][:m].sum()) == int((group >= 0).sum())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bs", [8, 6])
def test_mixed_rows_against_reference(bs, n):
    """Playout positions whose early plies repeat, with planted colour-swapped twins."""
    rows = M.mixed_rows(bs, n) if n != 2 else tuple(
        np.repeat(a[:1], 2, axis=0) if i < 3 else a[:2] for i, a in enumerate(M.mixed_rows(bs, 2)))
    want = M.merge(*rows, bs)
    if n == 2:
        assert want["m"] == 1 and want["count"].tolist() == [2]
    elif n > 64:
        assert want["m"] < n and want["count"].max() > 2 and (want["count"] == 1).any()
    _assert_equal(_raw(bs, _dev(rows)), want, n)


@pytest.mark.parametrize("bs", [8, 6])
def test_all_rows_identical(bs):
    """One group of 4,096 members: every adder on one row."""
    n = 4096
    b, w, s, pol, val = M.mixed_rows(bs, n, seed=3)
    b, w, s = np.repeat(b[:1], n), np.repeat(w[:1], n), np.repeat(s[:1], n)
    twin = np.arange(n) % 3 == 1                   # a third of them as the colour-swapped twin
    b[twin], w[twin], s[twin] = w[0], b[0], 3 - s[0]
    want = M.merge(b, w, s, pol, val, bs)
    assert want["m"] == 1 and want["count"].tolist() == [n]
    got = _raw(bs, _dev((b, w, s, pol, val)))
    _assert_equal(got, want, n)
    import os
    os.environ["RVZ_MERGE_HOT"] = "0"              # the same bytes without the LDS pre-reduction
    try:
        _assert_equal(_raw(bs, _dev((b, w, s, pol, val))), want, n)
    finally:
        del os.environ["RVZ_MERGE_HOT"]


@pytest.mark.parametrize("bs", [8, 6])
def test_distinct_rows_are_the_identity(bs):
    n = 4097
    rows = M.distinct_rows(bs, n)
    rows[3][5, 7] = np.float32(1e-30)              # copied, not recomputed (q would round to 0)
    dev = _dev(rows)
    got = _raw(bs, dev)
    assert int(got["m"][0]) == n
    assert torch.equal(got["policy"].view(torch.int32), dev[3].view(torch.int32))
    assert torch.equal(got["value"].view(torch.int32), dev[4].view(torch.int32))
    ar = torch.arange(n, dtype=torch.int32, device="cuda")
    assert torch.equal(got["first"], ar) and torch.equal(got["group"], ar)
    assert bool((got["count"] == 1).all())
    _assert_equal(got, M.merge(*rows, bs), n)


def test_distinct_rows_past_one_block_sum_per_thread():
    """The identity again at n = 2^20 + 1025 on 6x6: more than 1,024 scan blocks, so each thread of
    k_scan_blocks carries two block sums. The rows are made on the device, a counter split over
    the two bitboards under disjoint masks (distinct, disjoint, on the board, black to move), and
    the expectation needs no reference run."""
    bs, n = 6, 1024 * 1024 + 1025
    i = torch.arange(n, dtype=torch.int64, device="cuda")
    status = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    status[:, 0], status[:, 2] = 1, -1
    gen = torch.Generator(device="cuda").manual_seed(5)
    dev = (i & 0x3FF, i & ~0x3FF, status,
           torch.rand((n, bs * bs + 1), device="cuda", generator=gen),
           torch.rand((n,), device="cuda", generator=gen) * 2 - 1)
    assert int((i & ~0x3FF).max()) < 1 << (bs * bs)
    got = _raw(bs, dev)
    assert int(got["m"][0]) == n
    assert torch.equal(got["policy"].view(torch.int32), dev[3].view(torch.int32))
    assert torch.equal(got["value"].view(torch.int32), dev[4].view(torch.int32))
    ar = torch.arange(n, dtype=torch.int32, device="cuda")
    assert torch.equal(got["first"], ar) and torch.equal(got["group"], ar)
    assert bool((got["count"] == 1).all())


@pytest.mark.parametrize("bs", [8, 6])
def test_probe_chains(bs):
    """1,000 distinct rows in 1,024 slots (load 0.98) and in the default table: equal bytes; so
    too for a mix with duplicates."""
    for rows in (M.distinct_rows(bs, 1000, seed=1), M.mixed_rows(bs, 1000, seed=1)):
        dev = _dev(rows)
        tight, loose = _raw(bs, dev, table_log2=10), _raw(bs, dev),
        for k in tight:
            assert tight[k].cpu().numpy().tobytes() == loose[k].cpu().numpy().tobytes(), k
        _assert_equal(tight, M.merge(*rows, bs), 1000)


def test_determinism_across_runs_and_streams():
    bs, n = 8, 4097
    dev = _dev(M.mixed_rows(bs, n, seed=2))
    base = _raw(bs, dev)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = []
    for st in (streams[0], streams[1], streams[0]):
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            outs.append(_raw(bs, dev, stream=st.cuda_stream))
    torch.cuda.synchronize()
    for out in outs:
        for k in base:
            assert out[k].cpu().numpy().tobytes() == base[k].cpu().numpy().tobytes(), k


@pytest.mark.parametrize("defect", ["overlap", "off_board", "side", "policy_high", "policy_nan",
                                    "value_low"])
def test_malformed_rows(defect):
    """Every third row carries the defect; the good rows' results are the reference's without
    the bad ones."""
    bs, n = 6, 257
    b, w, s, pol, val = (a.copy() for a in M.mixed_rows(bs, n, seed=5))
    bad = np.arange(n) % 3 == 1
    if defect == "overlap":
        b[bad] |= np.uint64(1)
        w[bad] |= np.uint64(1)
    elif defect == "off_board":
        b[bad] |= np.uint64(1 << 36)
        w[bad & (np.arange(n) % 2 == 0)] |= np.uint64(1 << 63)
    elif defect == "side":
        s[bad] = np.where(np.arange(n)[bad] % 2 == 0, 0, 3)
    elif defect == "policy_high":
        pol[bad, np.arange(n)[bad] % 37] = 1.5
    elif defect == "policy_nan":
        pol[bad, np.arange(n)[bad] % 37] = np.nan
    else:
        val[bad] = -2.0
    want = M.merge(b, w, s, pol, val, bs)
    assert np.array_equal(want["group"] == -1, bad)
    got = _raw(bs, _dev((b, w, s, pol, val)))
    _assert_equal(got, want, n)
    good = M.merge(b[~bad], w[~bad], s[~bad], pol[~bad], val[~bad], bs)
    m = good["m"]
    assert int(got["m"][0]) == m
    assert got["policy"][:m].cpu().numpy().tobytes() == good["policy"].tobytes()
    assert got["value"][:m].cpu().numpy().tobytes() == good["value"].tobytes()
    assert np.array_equal(got["count"][:m].cpu().numpy(), good["count"])
    assert np.array_equal(got["first"][:m].cpu().numpy(), np.flatnonzero(~bad)[good["first"]])


def test_python_surface():
    import rvz
    bs, n = 8, 1025
    rows = M.mixed_rows(bs, n, seed=7)
    want = M.merge(*rows, bs)
    dev = _dev(rows)
    out = rvz.merge_positions(*dev, board_size=bs)
    assert out["m"] == want["m"] and isinstance(out["m"], int)
    for k in ("first", "count", "policy", "value", "group"):
        assert out[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    pad = rvz.merge_positions(dev[0], dev[1], dev[2], dev[3], dev[4].reshape(n, 1), bs,
                              table_log2=11, trim=False)
    assert pad["m"].is_cuda and pad["m"].dim() == 0 and int(pad["m"]) == want["m"]
    for k in ("first", "count", "policy", "value"):
        assert pad[k].shape[0] == n and torch.equal(pad[k][:want["m"]], out[k]), k
    assert torch.equal(pad["group"], out["group"])
    e64 = torch.empty(0, dtype=torch.int64, device="cuda")
    none = rvz.merge_positions(e64, e64, torch.empty(0, 4, dtype=torch.int32, device="cuda"),
                               torch.empty(0, 65, device="cuda"), torch.empty(0, device="cuda"))
    assert none["m"] == 0 and none["policy"].shape == (0, 65) and none["group"].shape == (0,)
    with pytest.raises(rvz.RvzError):
        rvz.merge_positions(*dev, board_size=bs, table_log2=10)      # 1,024 slots for 1,025 rows


def test_graph_capture():
    """The call captured at n = 4,097 and replayed twice on changed inputs."""
    import rvz
    bs, n = 8, 4097
    sets = [M.mixed_rows(bs, n, seed=k) for k in (11, 12)]
    ins = [t.clone() for t in _dev(sets[0])]
    eager = _raw(bs, ins)                                            # warm
    torch.cuda.synchronize()
    out = _outputs(bs, n)
    size = rvz.load().rvz_merge_scratch_size(bs, n, 0)
    scratch = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _raw(bs, ins, stream=torch.cuda.current_stream().cuda_stream, out=out, scratch=scratch)
    for rows in (sets[1], sets[0]):
        for t, x in zip(ins, _dev(rows)):
            t.copy_(x)
        for k, t in out.items():
            t.fill_(SENTINEL)
        graph.replay()
        _assert_equal(out, M.merge(*rows, bs), n)
    for k in out:
        assert torch.equal(out[k], eager[k]), k


# ---------------------------------------------------------------- end to end
def test_selfplay_trainer_with_merging():
    import rvz
    from rvz.pipeline import SelfPlayTrainer
    torch.manual_seed(0)
    G, sims = 64, 64      # in four leaf batches of 16: a one-batch search never leaves its root
    net = rvz.AlphaZeroNetwork(8, 1, 64).cuda()
    spt = SelfPlayTrainer(net, G, num_simulations=sims, batch_size=16, seed=7, train_steps=2,
                          train_batch=64, merge_positions=True)
    out = spt.run_iteration()
    assert 0 < out["merge_rows"] < out["merge_input_rows"] and out["samples"] == out["merge_rows"]
    for k in ("train/loss", "train/policy_loss", "train/value_loss"):
        assert np.isfinite(out[k]), k
    data = spt.generate()
    m = int(data["merge_rows"])
    assert data["states"].shape == (m, 3, 8, 8) and data["position_counts"].shape == (m,)
    assert int(data["position_counts"].sum()) == int(data["merge_input_rows"])
    from oracle import oracle as O
    start = torch.from_numpy(np.asarray(O.canonical(O.new_game(8), 8), np.float32)).cuda()
    at =(data["states"] == start).flatten(1).all(dim=1).nonzero().flatten()
    assert at.tolist() == [0]                                         # the first record of game 0
    assert int(data["position_counts"][0]) == G
    assert abs(float(data["policy_targets"][0].double().sum()) - 1.0) < 1e-6
    assert bool((data["policy_targets"].sum(dim=1) - 1).abs().max() < 1e-5)
    assert bool(data["value_targets"].abs().max() <= 1)
