"""The move-number temperature schedule without a GPU: sequential_draw_passes with a first-guess
draw count (a game under a schedule with late temperature 0 draws one value per move for its
first N moves only), the host-side argument rules, and the header / ctypes declarations of
rvz_act_schedule and rvz_action_probs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MOVES = 6


class _FakeGames:
    """A fake player: a game's length (3 .. 12 moves, or `floor` .. 12) is a function of the first
    value of its piece, and it draws one value per move for its first N_MOVES moves only. The
    payload of a game is the values it drew."""

    def __init__(self, floor=3):
        self.floor, self.calls = floor, []

    def length(self, first):
        return self.floor + int(first * (13 - self.floor))

    def game(self, draw):
        first = draw()
        n = min(self.length(first), N_MOVES)
        return [first] + [draw() for _ in range(n - 1)]

    def play(self, U):
        self.calls.append(len(U))
        out, used = [], []
        for row in U:
            it = iter(row)
            g = self.game(lambda: float(next(it)))
            out.append(g)
            used.append(len(g))
        return out, np.asarray(used)

    def sequential(self, rng, n):
        return [self.game(lambda: float(rng.random_sample())) for _ in range(n)]


def _run(fake, seed, n, **kw):
    from rvz.selfplay import sequential_draw_passes
    rng = np.random.RandomState(seed)
    payloads, where, used = sequential_draw_passes(n, 12, 16, True, rng, fake.play, **kw)
    return [payloads[p][j] for p, j in where], list(used), rng


@pytest.mark.parametrize("floor,one_pass", [(N_MOVES, True), (3, False)],
                         ids=["none-shorter", "some-shorter"])
def test_first_guess_passes(floor, one_pass):
    """Games in order, the shared stream where a sequential loop leaves it; one pass when no game
    is shorter than N (the first guess is exact), more than one, with the same result, when one
    is."""
    n, seed = 10, 5
    fake = _FakeGames(floor)
    seq_rng = np.random.RandomState(seed)
    want = fake.sequential(seq_rng, n)
    lens = [len(g) for g in want]
    assert all(x == N_MOVES for x in lens) if one_pass else min(lens[:-1]) < N_MOVES, lens
    got, used, rng = _run(fake, seed, n, first_guess=N_MOVES)
    assert got == want and used == lens
    nxt = seq_rng.random_sample()
    assert rng.random_sample() == nxt
    if one_pass:
        assert fake.calls == [n]
    else:
        assert len(fake.calls) > 1 and fake.calls[0] == n
    # any first guess gives the same games and leaves the same stream
    for guess in (0, 12):
        got2, used2, rng2 = _run(_FakeGames(floor), seed, n, first_guess=guess)
        assert got2 == want and used2 == lens
        assert rng2.random_sample() == nxt
    with pytest.raises(ValueError):
        _run(_FakeGames(floor), seed, n, first_guess=13)


def test_without_the_keyword_nothing_changes():
    """No keyword == the keyword at its default == first_guess = max_draws (today's first guess):
    same payloads per pass, same pass structure, same stream."""
    outs = []
    for kw in ({}, {"first_guess": None}, {"first_guess": 12}):
        fake = _FakeGames(3)
        got, used, rng = _run(fake, 9, 8, **kw)
        outs.append((got, used, fake.calls, rng.random_sample()))
    assert outs[0] == outs[1] == outs[2]
    assert len(outs[0][2]) > 1           # several passes: 12 is a wrong guess for every game


def test_schedule_draws():
    """Which moves draw: one value per move unless the move is chosen at temperature 0."""
    from rvz.selfplay import schedule_draws
    assert schedule_draws(1.0, None, 60) == (True, None)
    assert schedule_draws(0.0, None, 60) == (False, None)
    assert schedule_draws(1.0, (6, 0.0), 60) == (True, 6)
    assert schedule_draws(1.0, (80, 0.0), 60) == (True, 60)
    assert schedule_draws(1.0, (6, 0.1), 60) == (True, None)
    assert schedule_draws(0.0, (6, 1.0), 60) == (True, 54)     # draws from move 7 on
    assert schedule_draws(0.0, (80, 1.0), 60) == (True, 0)
    assert schedule_draws(0.0, (6, 0.0), 60) == (False, None)


def test_argument_helpers():
    import rvz
    from rvz._lib import check_schedule_args
    from rvz.selfplay import temperature_schedule_args
    assert check_schedule_args(None) is None
    assert check_schedule_args(None, float("nan")) is None       # off: late is not looked at
    assert check_schedule_args(6) == (6, 0.0)
    assert check_schedule_args(0, 0.25) == (0, 0.25)
    assert check_schedule_args(np.int64(30), 1) == (30, 1.0)
    for moves, late in ((-1, 0.0), (2.5, 0.0), ("6", 0.0), (True, 0.0), (2 ** 40, 0.0),
                        (6, -0.1), (6, float("nan")), (6, float("inf")), (6, None), (6, "x")):
        with pytest.raises(rvz.RvzError):
            check_schedule_args(moves, late)
    assert temperature_schedule_args({}) is None
    assert temperature_schedule_args({"temperature_late": 0.5}) is None
    assert temperature_schedule_args({"temperature_moves": None}) is None
    assert temperature_schedule_args({"temperature_moves": 6}) == (6, 0.0)
    assert temperature_schedule_args({"temperature_moves": 6, "temperature_late": 0.1}) == (6, 0.1)
    for bad in ({"temperature_moves": -2}, {"temperature_moves": 1.5},
                {"temperature_moves": 6, "temperature_late": -1.0},
                {"temperature_moves": 6, "temperature_late": float("nan")},
                {"temperature_moves": 6, "temperature_late": float("inf")}):
        with pytest.raises(rvz.RvzError):
            temperature_schedule_args(bad)


def test_python_refuses_before_any_device_call():
    import rvz
    import torch

    class NoDevice:          # Engine.temperature_schedule must raise before it touches the handle
        pass

    for moves, late in ((-1, 0.0), (1.5, 0.0), (6, -1.0), (6, float("nan")), (6, float("inf"))):
        with pytest.raises(rvz.RvzError):
            rvz.Engine.temperature_schedule(NoDevice(), moves, late)
    with pytest.raises(AttributeError):     # valid arguments reach the (absent) device call
        rvz.Engine.temperature_schedule(NoDevice(), 6, 0.0)
    with pytest.raises(AttributeError):
        rvz.Engine.temperature_schedule(NoDevice(), None)
    host = torch.zeros(2, 65, dtype=torch.int32)
    with pytest.raises(rvz.RvzError, match="board_size"):
        rvz.action_probs(host, 1.0, board_size=7)
    with pytest.raises(rvz.RvzError, match="visits"):
        rvz.action_probs(host, 1.0, board_size=6)


def _header_arg_count(name):
    text = open(os.path.join(ROOT, "include", "rvz.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"include/rvz.h does not declare {name}"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_and_binding():
    import rvz
    sig = rvz._lib.SIGNATURES
    assert sig["rvz_act_schedule"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_double])
    assert sig["rvz_action_probs"][0] is C.c_int
    for name in ("rvz_act_schedule", "rvz_action_probs"):
        assert _header_arg_count(name) == len(sig[name][1]), name
    assert _header_arg_count("rvz_action_probs") == 9
    # the library exports both, and they refuse bad arguments before any HIP call
    lib = rvz.load()
    p = 0x10000                                   # never dereferenced
    assert lib.rvz_act_schedule(None, 10, 0.0) == EINVAL
    assert lib.rvz_action_probs(7, 4, p, p, p, p, p, None, None) == EINVAL
    assert lib.rvz_action_probs(8, -1, p, p, p, p, p, None, None) == EINVAL
    for k in range(2, 7):                         # a null array with n > 0
        args = [8, 4, p, p, p, p, p, None, None]
        args[k] = None
        assert lib.rvz_action_probs(*args) == EINVAL
    assert lib.rvz_action_probs(8, 0, None, None, None, None, None, None, None) == 0
    assert callable(rvz.action_probs) and callable(rvz.Engine.temperature_schedule)
