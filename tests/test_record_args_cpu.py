"""What the training-record wrappers (rvz.training_rows, rvz.merge_positions, rvz.replay_batch,
rvz.replay_batch_weighted) accept and refuse, without a GPU: a good call on CPU tensors with no
rows (no pointer is taken, nothing launches) and a table of single mutations of it, each refused
with an RvzError that names the function. And the names rvz exports."""
import pytest
import torch

CAP, START, LIVE = 7, 5, 3


def _good(fn, bs=8):
    """(callable, keyword arguments) of a call of rvz.<fn> that goes through with no rows."""
    import rvz
    npol = bs * bs + 1
    i64 = lambda n: torch.zeros(n, dtype=torch.int64)
    if fn in ("training_rows", "merge_positions"):
        kw = dict(black=i64(0), white=i64(0), status=torch.zeros(0, 4, dtype=torch.int32),
                  policy=torch.zeros(0, npol), board_size=bs)
        if fn == "training_rows":
            kw.update(sym=torch.zeros(0, dtype=torch.int32))
        else:
            kw.update(value=torch.zeros(0), table_log2=0)
        return getattr(rvz, fn), kw
    kw = dict(mover=i64(CAP), opponent=i64(CAP), policy=torch.zeros(CAP, npol),
              value=torch.zeros(CAP), start=START, live=LIVE, nb=0, seed=11, step=2 ** 64 + 3,
              idx=torch.zeros(0, dtype=torch.int64), sym=torch.zeros(0, dtype=torch.int32),
              board_size=bs)
    if fn == "replay_batch_weighted":
        kw.update(cdf=i64(4 + LIVE), word=i64(0))
    return getattr(rvz, fn), kw


@pytest.mark.parametrize("bs", (8, 6))
def test_calls_without_rows_go_through(bs):
    npol = bs * bs + 1
    call, kw = _good("training_rows", bs)
    for more, n_out in ((dict(), 2), (dict(quirk=True), 3), (dict(all_images=True, sym=None), 2)):
        out = call(**{**kw, **more})
        assert len(out) == n_out
        assert out[0].shape == (0, 3, bs, bs) and out[0].dtype == torch.float32
        assert out[1].shape == (0, npol) and out[1].dtype == torch.float32
        assert n_out == 2 or (out[2].shape == (0,) and out[2].dtype == torch.int32)

    call, kw = _good("merge_positions", bs)
    for trim in (True, False):
        for value in (kw["value"], kw["value"].reshape(0, 1)):
            out = call(**{**kw, "trim": trim, "value": value})
            assert sorted(out) == ["count", "first", "group", "m", "policy", "value"]
            if trim:
                assert out["m"] == 0 and isinstance(out["m"], int)
            else:
                assert out["m"].shape == () and out["m"].dtype == torch.int32
                assert int(out["m"]) == 0
            for name in ("first", "count", "group"):
                assert out[name].shape == (0,) and out[name].dtype == torch.int32
            assert out["policy"].shape == (0, npol) and out["policy"].dtype == torch.float32
            assert out["value"].shape == (0,) and out["value"].dtype == torch.float32

    for fn in ("replay_batch", "replay_batch_weighted"):
        call, kw = _good(fn, bs)
        for more in (dict(), dict(idx=None, sym=None, random_sym=False),
                     dict(value=kw["value"].reshape(CAP, 1), live=CAP, start=CAP - 1)):
            if fn == "replay_batch_weighted" and "live" in more:
                more = dict(more, cdf=torch.zeros(4 + CAP, dtype=torch.int64), word=None)
            out = call(**{**kw, **more})
            assert len(out) == (6 if fn == "replay_batch_weighted" else 5)
            assert out[0].shape == (0, 3, bs, bs) and out[1].shape == (0, npol)
            assert out[2].shape == (0, 1) and out[3].shape == (0,) and out[4].shape == (0,)
            assert [t.dtype for t in out[:5]] == [torch.float32] * 3 + [torch.int32] * 2
            assert len(out) == 5 or (out[5].shape == (0,) and out[5].dtype == torch.float32)


def _rows_mutations(fn):
    """Single mutations of the good call of training_rows / merge_positions."""
    i32 = torch.zeros(0, dtype=torch.int32)
    m = [dict(board_size=7), dict(black=i32), dict(white=i32),
         dict(black=torch.zeros(0, 1, dtype=torch.int64)),
         dict(white=torch.zeros(1, dtype=torch.int64)),
         dict(status=torch.zeros(0, 3, dtype=torch.int32)),
         dict(policy=torch.zeros(0, 65, dtype=torch.float64)), dict(policy=torch.zeros(0, 64))]
    if fn == "training_rows":
        m += [dict(sym=None), dict(sym=torch.zeros(0)), dict(sym=torch.zeros(0, dtype=torch.bool)),
              dict(sym=torch.zeros(1, dtype=torch.int32))]
    else:
        m += [dict(value=torch.zeros(0, 2)), dict(value=torch.zeros(0, dtype=torch.float64)),
              dict(table_log2=True), dict(table_log2=4.0), dict(table_log2=31),
              dict(table_log2=-1)]
    return m


def _ring_mutations(fn):
    """Single mutations of the good call of replay_batch / replay_batch_weighted."""
    i64 = lambda *shape: torch.zeros(*shape, dtype=torch.int64)
    m = [dict(board_size=7)]
    for name in ("start", "live", "nb", "seed", "step"):
        m += [{name: True}, {name: 1.0}]
    m += [dict(mover=torch.zeros(CAP, dtype=torch.int32)),
          dict(opponent=torch.zeros(CAP, dtype=torch.int32)), dict(mover=i64(CAP, 1)),
          dict(opponent=i64(CAP + 1)), dict(policy=torch.zeros(CAP, 65, dtype=torch.float64)),
          dict(policy=torch.zeros(CAP, 64)), dict(value=torch.zeros(CAP, 2)),
          dict(value=torch.zeros(CAP, dtype=torch.float64)),
          dict(live=0), dict(live=CAP + 1), dict(start=CAP), dict(start=-1), dict(nb=-1),
          dict(nb=2 ** 31 // 65 + 1, idx=None, sym=None, word=None),
          dict(idx=torch.zeros(0)), dict(sym=torch.zeros(0, dtype=torch.bool)),
          dict(idx=i64(1)), dict(sym=i64(0, 1))]
    if fn == "replay_batch_weighted":
        m += [dict(word=torch.zeros(0, dtype=torch.int32)), dict(word=i64(1)),
              dict(cdf=torch.zeros(4 + LIVE, dtype=torch.int32)), dict(cdf=i64(3 + LIVE)),
              dict(cdf=i64(2 * (4 + LIVE))[::2]), dict(cdf=i64(4 + LIVE, 1))]
    else:
        for x in m:
            x.pop("word", None)
    return m


CASES = [(fn, 8, mut) for fn in ("training_rows", "merge_positions") for mut in _rows_mutations(fn)]
CASES += [(fn, 8, mut) for fn in ("replay_batch", "replay_batch_weighted")
          for mut in _ring_mutations(fn)]
CASES += [(fn, 6, dict(nb=2 ** 31 // 37 + 1, idx=None, sym=None))
          for fn in ("replay_batch", "replay_batch_weighted")]
CASES += [(fn, 6, dict(policy=torch.zeros(n, 65)))
          for fn, n in (("training_rows", 0), ("merge_positions", 0), ("replay_batch", CAP),
                        ("replay_batch_weighted", CAP))]


def _case_id(case):
    fn, bs, mut = case
    what = ",".join(f"{k}={tuple(v.shape)}:{str(v.dtype)[6:]}" if isinstance(v, torch.Tensor)
                    else f"{k}={v!r}" for k, v in mut.items())
    return f"{fn}-{bs}-{what}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_single_mutations_are_refused(case):
    import rvz
    fn, bs, mut = case
    call, kw = _good(fn, bs)
    with pytest.raises(rvz.RvzError) as err:
        call(**{**kw, **mut})
    if mut.keys() == {"board_size"}:              # the one rule whose message names no function
        assert str(err.value) == "board_size must be 8 or 6"
    else:
        assert str(err.value).startswith(fn + ":"), str(err.value)


def test_replay_cdf_keeps_its_own_rules():
    """live = 0 is a table of no rows for replay_cdf and a refusal for the two batch calls."""
    import rvz
    w = torch.ones(CAP)
    for bad in (dict(live=-1), dict(live=CAP + 1), dict(start=CAP), dict(start=True),
                dict(live=2.0), dict(tile_log2=False), dict(tile_log2=5)):
        with pytest.raises(rvz.RvzError) as err:
            rvz.replay_cdf(w, **{**dict(start=START, live=0), **bad})
        assert str(err.value).startswith("replay_cdf:"), str(err.value)


# what rvz/__init__.py imported from .engine before the record wrappers moved to rvz.records
ENGINE_NAMES = """AB_HEUR_MAX AB_MAX_DEPTH AB_WIN SOLVE_ABANDONED SOLVE_NOT_A_MOVE Engine
action_probs alphabeta alphabeta_weights best_moves board_apply board_canonical board_legal
board_symmetry dirichlet_noise merge_positions policy_softmax replay_batch replay_batch_weighted
replay_cdf solve solve_moves solve_moves_wld solve_window solve_wld symmetry_compose
symmetry_inverse training_rows""".split()


def test_rvz_still_exports_every_name():
    import rvz
    assert len(ENGINE_NAMES) == 28
    missing = [name for name in ENGINE_NAMES if not hasattr(rvz, name)]
    assert not missing, missing
    for name in ("board_symmetry", "training_rows", "merge_positions", "replay_batch",
                 "replay_cdf", "replay_batch_weighted", "symmetry_compose", "symmetry_inverse"):
        assert callable(getattr(rvz, name)), name
    assert rvz.symmetry_compose(1, 3) == 0 and rvz.symmetry_inverse(1) == 3
