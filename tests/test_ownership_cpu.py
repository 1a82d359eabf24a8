"""The final-ownership targets without a GPU: what the three entry points refuse before any HIP
call, the scratch size, the NumPy restatements' own invariants (tests/ownership_ref.py), the
option through records_to_training / games_to_training / ReplayBuffer / DDPTrainer on CPU tensors
with the restatements in the kernels' places, the network's training-only head, and every
ValueError of the option."""
import numpy as np
import pytest
import torch

import ownership_ref as OR
import records_games_ref as RG
import replay_ref as RR
from test_pipeline_cpu import synthetic_records

EINVAL = -22


# ---------------------------------------------------------------- the entry points' refusals
def test_records_final_refuses_bad_arguments_without_a_gpu():
    import rvz
    lib = rvz.load()
    q = 0x10000
    #       bs  P   G  black white side idx n  src count fm fo ok stats stream
    good = [8, 70, 65, q, q, q, q, 9, q, None, q, q, q, q, None]
    for k, v in ((0, 7), (0, 4), (1, 0), (1, -1), (2, 0), (2, -5), (7, -1),
                 (1, 2 ** 31 // (65 * 65) + 1), (2, 2 ** 31 // (65 * 70) + 1)):
        args = list(good)
        args[k] = v
        assert lib.rvz_records_final(*args) == EINVAL, (k, v)
    args = list(good)
    args[0], args[1], args[2] = 6, 2 ** 16, 2 ** 31 // (37 * 2 ** 16) + 1
    assert lib.rvz_records_final(*args) == EINVAL                 # 6x6: * 37 reaches 2^31
    for k in (3, 4, 5, 6, 8, 10, 11, 12, 13):                     # count (9) may be null
        bad = list(good)
        bad[k] = None
        assert lib.rvz_records_final(*bad) == EINVAL, k
    none = list(good)
    none[7] = 0
    for k in (8, 10, 11, 12):                                     # n = 0: no row array is needed
        none[k] = None
    assert lib.rvz_records_final(*none) == 0


def test_replay_ownership_refuses_bad_arguments_without_a_gpu():
    import rvz
    lib = rvz.load()
    q = 0x10000
    #       bs cap fm fo nb slot sym own margin stream
    good = [8, 7, q, q, 5, q, q, q, q, None]
    for k, v in ((0, 7), (1, 0), (1, -3), (4, -1), (4, 2 ** 31 // 65 + 1)):
        args = list(good)
        args[k] = v
        assert lib.rvz_replay_ownership(*args) == EINVAL, (k, v)
    args = list(good)
    args[0], args[4] = 6, 2 ** 31 // 37 + 1
    assert lib.rvz_replay_ownership(*args) == EINVAL
    for k in (2, 3, 5, 6, 7, 8):
        bad = list(good)
        bad[k] = None
        assert lib.rvz_replay_ownership(*bad) == EINVAL, k
    assert lib.rvz_replay_ownership(8, 7, None, None, 0, None, None, None, None, None) == 0
    assert lib.rvz_replay_ownership(8, 0, None, None, 0, None, None, None, None, None) == EINVAL


def test_ownership_loss_refuses_bad_arguments_and_sizes_its_scratch_without_a_gpu():
    import rvz
    lib = rvz.load()
    q = 0x10000
    #       bs  n  logits target weight scratch out_loss out_row grad stream
    good = [8, 65, q, q, None, q, q, None, None, None]
    for k, v in ((0, 7), (1, -1), (1, 2 ** 31 // 65 + 1), (5, q + 8), (2, None), (3, None),
                 (5, None), (6, None)):
        args = list(good)
        args[k] = v
        assert lib.rvz_ownership_loss(*args) == EINVAL, (k, v)
    assert lib.rvz_ownership_loss(6, 2 ** 31 // 37 + 1, q, q, None, q, q, None, None, None) == EINVAL
    assert lib.rvz_ownership_loss(8, 0, None, None, None, None, None, None, None, None) == 0
    size = lib.rvz_ownership_loss_scratch_size
    for bs in (8, 6):
        last = -1
        for n in (0, 1, 2, 63, 64, 65, 257, 4096, 4097, 10 ** 5, 2 ** 24, 2 ** 24 + 1):
            now = size(bs, n)
            assert now >= last and now % 8 == 0 and now == lib.rvz_loss_scratch_size(bs, n), n
            last = now
        assert size(bs, -1) < 0 and size(bs, 2 ** 31 - 1) < 0
    assert size(7, 4) < 0


def test_python_wrappers_refuse_before_any_device_call():
    import rvz
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    win = dict(rec_black=i64(5, 3), rec_white=i64(5, 3), rec_side=i32(5, 3), rec_idx=i32(5, 3),
               src=i32(0))
    out = rvz.records_final(**win)
    assert out["ok"].shape == (0,) and out["stats"].tolist() == [0, 0, 0, 0]
    for mut in (dict(board_size=7), dict(rec_black=i32(5, 3)), dict(rec_white=i64(5, 4)),
                dict(rec_side=torch.zeros(5, 3)), dict(src=torch.zeros(0)), dict(src=i32(0, 1)),
                dict(count=i64(1)), dict(count=i32(2)), dict(count=3)):
        with pytest.raises(rvz.RvzError):
            rvz.records_final(**{**win, **mut})
    ring = dict(final_mover=i64(7), final_opponent=i64(7), slot=i32(0), sym=i32(0))
    own, margin = rvz.replay_ownership(**ring, board_size=6)
    assert own.shape == (0, 36) and margin.shape == (0,)
    for mut in (dict(board_size=5), dict(final_mover=i32(7)), dict(final_opponent=i64(8)),
                dict(slot=torch.zeros(0)), dict(sym=i32(1)), dict(final_mover=i64(0),
                                                                 final_opponent=i64(0))):
        with pytest.raises(rvz.RvzError):
            rvz.replay_ownership(**{**ring, **mut})
    z = torch.zeros(0, 64)
    empty = rvz.ownership_loss(z, z)
    assert not empty["out_loss"].any() and empty["grad_logits"].shape == (0, 64)
    for a, kw in (((torch.zeros(2, 65), torch.zeros(2, 65)), {}),
                  ((torch.zeros(2, 64), torch.zeros(2, 36)), {}),
                  ((torch.zeros(2, 64, dtype=torch.float64), torch.zeros(2, 64)), {}),
                  ((torch.zeros(2, 64), torch.zeros(2, 64)), dict(weights=torch.zeros(3))),
                  ((torch.zeros(2, 64), torch.zeros(2, 64)), dict(board_size=6))):
        with pytest.raises(rvz.RvzError):
            rvz.ownership_loss(*a, **kw)
    for name in ("records_final", "replay_ownership", "ownership_loss", "full_ownership_loss"):
        assert callable(getattr(rvz, name)), name


# ---------------------------------------------------------------- the restatements' invariants
@pytest.mark.parametrize("bs", [6, 8])
def test_reference_final_boards_are_the_oracles(oracle, bs):
    """A whole game recorded from the start position: every record's final boards are the boards
    the oracle holds after the game's moves, seen from the record's mover; a record of the next,
    unfinished game is open."""
    P = bs * bs + 4
    rng = np.random.default_rng(bs)
    black, white = np.zeros((P, 1), np.uint64), np.zeros((P, 1), np.uint64)
    side, idx = np.zeros((P, 1), np.int32), np.full((P, 1), -2, np.int32)
    col = RG.stream(oracle, bs, rng, P)
    game, length = oracle.new_game(bs), None
    for k, (b, w, s, sq) in enumerate(col):
        black[k, 0], white[k, 0], side[k, 0], idx[k, 0] = b, w, s, sq
        if length is None:
            assert oracle.make_move(game, sq, bs)
            if game.over:
                length = k + 1
    assert length is not None and length < P
    fm, fo, ok, stats, handled, _ = OR.final(oracle, bs, black, white, side, idx,
                                                np.arange(P))
    assert handled == P and ok[:length].all() and not ok[length:].any()
    B, W = int(game.black), int(game.white)
    for k in range(length):
        assert (int(fm[k]), int(fo[k])) == ((B, W) if side[k, 0] == 1 else (W, B)), k
    assert stats.tolist() == [P, length, P - length, 0]
    # count below n: the rows beyond it are not handled
    fm2, _, ok2, stats2, handled2, _ = OR.final(oracle, bs, black, white, side, idx,
                                                np.arange(P), 3)
    assert handled2 == 3 and stats2.tolist() == [3, 3, 0, 0] and not fm2[3:].any()


@pytest.mark.parametrize("bs", [6, 8])
def test_reference_ownership_sums_to_the_margin(bs):
    rng = np.random.default_rng(7 + bs)
    nsq = bs * bs
    cap = 40
    pick = rng.integers(0, 3, (cap, nsq))
    fm = np.array([sum(1 << s for s in range(nsq) if pick[r, s] == 1) for r in range(cap)],
                  np.uint64)
    fo = np.array([sum(1 << s for s in range(nsq) if pick[r, s] == 2) for r in range(cap)],
                  np.uint64)
    fo[5] |= fm[5] & (~fm[5] + np.uint64(1))                  # an overlap: a zero row
    slot = np.concatenate([np.repeat(np.arange(cap), 8), [-1, cap, 3, 3]])
    sym = np.concatenate([np.tile(np.arange(8), cap), [0, 0, 8, -1]])
    own, margin = OR.ownership(bs, fm, fo, slot, sym)
    assert np.array_equal(own.sum(1), margin)
    assert not own[-4:].any() and not own[40:48].any() and not margin[40:48].any()
    # k = 0 is the identity, and every image holds the same discs
    assert np.array_equal(own[0].reshape(bs, bs), OR.bits(fm[0], bs) - OR.bits(fo[0], bs))
    for r in range(8):
        assert sorted(own[r]) == sorted(own[0])
    # the direction is symmetry_ref's: the mover's discs of the state planes
    import symmetry_ref as S
    st8, _, _ = S.training_rows(fm[:4], fo[:4], np.ones(4, np.int32),
                                np.zeros((4, nsq + 1), np.float32), None, bs, all_images=True)
    assert np.array_equal(st8[:, 0].reshape(32, nsq) - st8[:, 1].reshape(32, nsq), own[:32])


def test_reference_loss_is_the_torch_expression():
    g = torch.Generator().manual_seed(3)
    o = torch.randn(9, 36, generator=g) * 3
    t = torch.randint(-1, 2, (9, 36), generator=g).float()
    w = torch.rand(9, generator=g)
    ref = OR.loss(o.numpy(), t.numpy(), w.numpy())
    od = o.double().requires_grad_(True)
    per_row = ((torch.tanh(od) - t.double()) ** 2).mean(1)
    L = (w.double() * per_row).sum() / w.double().sum()
    L.backward()
    assert abs(ref["out_loss"][0] - L.item()) < 1e-14
    assert np.allclose(ref["grad_logits"], od.grad.float().numpy(), rtol=1e-6, atol=1e-12)
    bad = t.clone()
    bad[4, 7] = 0.5
    assert OR.loss(o.numpy(), bad.numpy())["out_loss"][6] == 1


# ---------------------------------------------------------------- the option on CPU tensors
def _oracle_canonical(black, white, status, board_size):
    raise AssertionError("compact rows do not call canonical")


def test_records_to_training_ownership(oracle):
    from rvz.trainer import records_to_training
    t, games = synthetic_records(G=6, seed=2)
    plain = records_to_training(**t, canonical=_oracle_canonical, compact=True)
    own = records_to_training(**t, canonical=_oracle_canonical, compact=True, ownership=True,
                              finaler=OR.as_finaler(oracle))
    assert set(own) - set(plain) == {"final_mover", "final_opponent", "ownership_dropped"}
    assert int(own["ownership_dropped"]) == 0
    for k in plain:
        assert torch.equal(plain[k], own[k]), k
    n = plain["mover"].numel()
    assert own["final_mover"].shape == (n,) and own["final_mover"].dtype == torch.int64
    # the margin's sign is the value target: the final position decides the winner
    fm, fo = (own[k].numpy().view(np.uint64) for k in ("final_mover", "final_opponent"))
    margin = np.array([bin(int(a)).count("1") - bin(int(b)).count("1") for a, b in zip(fm, fo)])
    assert np.array_equal(np.sign(margin), plain["value_targets"].reshape(-1).numpy())
    # a game cut short: its rows are dropped from every key and counted
    cut = dict(t)
    cut["rec_idx"] = t["rec_idx"].clone()
    length = int((t["rec_idx"][:, 2] >= 0).sum())
    cut["rec_idx"][length - 1, 2] = -2
    part = records_to_training(**cut, canonical=_oracle_canonical, compact=True, ownership=True,
                               finaler=OR.as_finaler(oracle))
    assert int(part["ownership_dropped"]) == length - 1
    assert part["mover"].numel() == n - length == part["final_mover"].numel()
    for bad in (dict(merge_positions=True), dict(compact=False)):
        with pytest.raises(ValueError, match="ownership"):
            records_to_training(**t, canonical=_oracle_canonical,
                                **{**dict(compact=True, ownership=True), **bad})


def test_games_to_training_ownership(oracle):
    from rvz.trainer import games_to_training
    bs, P, G = 6, 60, 5
    win = RG.window(oracle, bs, P, G, 4)
    rows = RG.games(oracle, bs, *win)
    tw = RG.tensors(*win)
    trows = {k: torch.from_numpy(np.ascontiguousarray(
        v.view(np.int64) if v.dtype == np.uint64 else v)) for k, v in rows.items()
        if k in ("mover", "opponent", "policy", "value", "src")}
    trows["m"] = rows["m"]
    plain = games_to_training(trows, bs)
    own = games_to_training(trows, bs, ownership=True, window=tw[:4],
                            finaler=OR.as_finaler(oracle))
    assert int(own["ownership_dropped"]) == 0 and own["final_mover"].numel() == rows["m"]
    for k in plain:
        assert torch.equal(plain[k], own[k]), k
    for bad in (dict(window=None), dict(merge_positions=True), dict(compact=False)):
        with pytest.raises(ValueError, match="ownership|window"):
            games_to_training(trows, bs, **{**dict(ownership=True, window=tw[:4]), **bad})


def test_replay_buffer_ownership_columns_follow_the_ring():
    import rvz
    bs, cap = 6, 10
    mover, opponent, policy, value = RR.ring(bs, 64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int64) if a.dtype == np.uint64
                                                        else a))
    buf = rvz.ReplayBuffer(cap, bs, "cpu", window_iterations=2, batcher=RR.batcher,
                           ownership=True, ownership_batcher=OR.as_batcher)
    plain = rvz.ReplayBuffer(cap, bs, "cpu", window_iterations=2, batcher=RR.batcher)
    at = 0
    for it, n in ((0, 4), (1, 5), (2, 4), (3, 3)):            # wraps, overwrites, drops
        rows = slice(at, at + n)
        args = (t(mover[rows]), t(opponent[rows]), t(policy[rows]), t(value[rows]), it)
        with pytest.raises(ValueError, match="final_mover"):
            buf.append(*args)
        with pytest.raises(ValueError, match="ownership=True"):
            plain.append(*args, final_mover=t(mover[rows]), final_opponent=t(opponent[rows]))
        # the row's own bitboards stand in for its final position: the columns must stay aligned
        buf.append(*args, final_mover=t(mover[rows]), final_opponent=t(opponent[rows]))
        plain.append(*args)
        at += n
        assert torch.equal(buf.final_mover, buf.mover) and (buf.start, len(buf)) == (
            plain.start, len(plain))
        got = buf.sample(17, 5, it)
        want = plain.sample(17, 5, it)
        assert len(got) == 7 and len(want) == 5
        for a, b in zip(got[:5], want):
            assert torch.equal(a, b)
        own, margin = got[5], got[6]
        assert own.shape == (17, bs * bs) and torch.equal(own.sum(1), margin)
        # the ownership of a row's own position is its state planes' difference
        st = got[0]
        assert torch.equal(own, (st[:, 0] - st[:, 1]).reshape(17, -1))
    with pytest.raises(ValueError, match="ownership_batcher"):
        rvz.ReplayBuffer(cap, bs, "cpu", ownership_batcher=OR.as_batcher)


# ---------------------------------------------------------------- the network and the trainers
def test_network_head_is_training_only():
    import rvz
    from rvz.network import h2_covers, pack_resnet_params
    torch.manual_seed(0)
    off = rvz.AlphaZeroNetwork(6, 2, 64)
    torch.manual_seed(0)
    on = rvz.AlphaZeroNetwork(6, 2, 64, ownership_head=True)
    torch.manual_seed(0)
    before = rvz.AlphaZeroNetwork(6, 2, 64, False)
    assert list(off.state_dict()) == list(before.state_dict())
    assert not any("own" in k for k in off.state_dict())
    assert set(on.state_dict()) - set(off.state_dict()) == {"own_conv.weight", "own_conv.bias"}
    for k, v in off.state_dict().items():
        assert torch.equal(v, on.state_dict()[k]), k
    assert pack_resnet_params(on).numpy().tobytes() == pack_resnet_params(off).numpy().tobytes()
    assert h2_covers(on, device="cuda") == h2_covers(off, device="cuda")
    x = (torch.rand(5, 3, 6, 6) > 0.5).float()
    on.eval(), off.eval()
    with torch.no_grad():
        p0, v0 = off(x)
        p1, v1 = on(x)
        p2, v2, own = on.forward_aux(x)
    assert torch.equal(p0, p1) and torch.equal(v0, v1) and torch.equal(p1, p2)
    assert torch.equal(v1, v2) and own.shape == (5, 36)
    with pytest.raises(ValueError, match="ownership_head"):
        off.forward_aux(x)


def test_trainer_ownership_coef_rules_and_a_step():
    import rvz
    from rvz.loss import differentiable_ownership
    from rvz.trainer import DDPTrainer
    bs = 6
    torch.manual_seed(1)
    on = rvz.AlphaZeroNetwork(bs, 1, 64, ownership_head=True)
    off = rvz.AlphaZeroNetwork(bs, 1, 64)
    for model, c in ((on, 0.0), (off, 0.5)):
        with pytest.raises(ValueError, match="ownership"):
            DDPTrainer(model, ownership_coef=c)
    for c in (-1.0, True, float("nan"), "x"):
        with pytest.raises(ValueError, match="ownership_coef"):
            DDPTrainer(on, ownership_coef=c)
    mover, opponent, policy, value = RR.ring(bs, 40)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int64) if a.dtype == np.uint64
                                                        else a))
    buf = rvz.ReplayBuffer(64, bs, "cpu", batcher=RR.batcher, ownership=True,
                           ownership_batcher=OR.as_batcher)
    buf.append(t(mover), t(opponent), t(policy), t(value), 0, final_mover=t(mover),
               final_opponent=t(opponent))
    tr = DDPTrainer(on, batch_size=16, ownership_coef=0.5,
                    ownership_loss_fn=differentiable_ownership(OR.as_kernel))
    w0 = on.own_conv.weight.detach().clone()
    out = tr.train_replay(buf, 3, seed=1)
    assert out["steps"] == 3
    for k in ("train/loss", "train/policy_loss", "train/value_loss", "train/ownership_loss",
              "train/ownership_agreement"):
        assert np.isfinite(out[k]), k
    assert 0.0 <= out["train/ownership_agreement"] <= 1.0 and out["train/ownership_loss"] > 0
    assert abs(out["train/loss"] - (out["train/policy_loss"] + out["train/value_loss"] +
                                    0.5 * out["train/ownership_loss"])) < 1e-5
    assert not torch.equal(w0, on.own_conv.weight)             # the head is trained
    with pytest.raises(ValueError, match="train_replay"):
        tr.train_epoch({"states": torch.zeros(1, 3, bs, bs)})
    plain = rvz.ReplayBuffer(64, bs, "cpu", batcher=RR.batcher)
    with pytest.raises(ValueError, match="ownership"):
        tr.train_replay(plain, 1)
    with pytest.raises(ValueError, match="ownership"):
        DDPTrainer(off).train_replay(buf, 1)


def test_selfplay_trainer_ownership_rules():
    """The option's rules are checked before the model or the device is touched."""
    from rvz.pipeline import SelfPlayTrainer
    for kw, says in ((dict(), "replay_iterations"), (dict(replay_iterations=0), "replay_iter"),
                     (dict(replay_iterations=2, merge_positions=True), "merge_positions"),
                     (dict(replay_iterations=2, adjudicate_empties=4), "adjudicate_empties"),
                     (dict(replay_iterations=2, continuous_plies=8, merge_positions=True),
                      "merge_positions")):
        with pytest.raises(ValueError, match=says):
            SelfPlayTrainer(None, 4, ownership_coef=0.5, **kw)
    for c in (-0.5, True, float("inf")):
        with pytest.raises(ValueError, match="ownership_coef"):
            SelfPlayTrainer(None, 4, ownership_coef=c, replay_iterations=2)
