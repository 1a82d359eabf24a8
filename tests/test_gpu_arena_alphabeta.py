"""rvz.arena.AlphaBetaPlayer on the GPU: its games against host games played with
tests/alphabeta_ref.py (and tests/solve_ref.py below solve_empties) on the CPU oracle, and a
tournament with all three kinds of player."""
import random

import numpy as np
import pytest
import torch

import alphabeta_ref as A
import solve_ref as R

pytestmark = pytest.mark.gpu


def host_game(bs, black, white):
    """One game on the oracle; black / white are (depth, solve_empties). Returns (the result for
    Black, the moves): each mover plays alphabeta_ref.alphabeta's move at its depth with the
    default table, or, with at most solve_empties empty squares, solve_ref.alphabeta's."""
    wt = A.default_table(bs)
    g = R.O.new_game(bs)
    moves = []
    while not g.over:
        depth, solve_empties = black if g.side == 1 else white
        if 0 < solve_empties and R.empties(g, bs) <= solve_empties:
            sq = R.alphabeta(g, bs)[1]
        else:
            sq = A.alphabeta(g, depth, wt, bs)[1]
        assert R.O.make_move(g, sq, bs)
        moves.append(sq)
    nb, nw = bin(g.black).count("1"), bin(g.white).count("1")
    return (1.0 if nb > nw else (0.0 if nw > nb else 0.5)), moves


def _arena(bs, seed, players):
    from rvz.arena import AlphaBetaPlayer, Arena
    arena = Arena(seed=seed)
    for pid, (depth, solve_empties) in players.items():
        arena.add_player(AlphaBetaPlayer(pid, depth=depth, board_size=bs,
                                         solve_empties=solve_empties))
    return arena


@pytest.mark.parametrize("bs", [6, 8])
def test_deterministic_games_against_the_host(bs):
    """depth 2 against depth 1, both colours: the results are the host games', and the player
    draws from neither generator. In the batched order the arena itself draws one uniform per
    game per ply whoever moves; the alpha-beta players add nothing to that."""
    players = {"d2": (2, 0), "d1": (1, 0)}
    black, white = ["d2", "d1", "d2"], ["d1", "d2", "d2"]
    hosts = [host_game(bs, players[b], players[w]) for b, w in zip(black, white)]
    want = [h[0] for h in hosts]
    plies = max(len(h[1]) for h in hosts)
    for order in ("reference", "batched"):
        arena = _arena(bs, 11, players)
        assert arena.play_games(black, white, draw_order=order) == want, order
        np_rng, py_rng = np.random.RandomState(11), random.Random(11)
        if order == "batched":
            for _ in range(plies):
                np_rng.random_sample(len(black))
        else:
            assert arena.reference_order_passes == 1
        assert arena.np_rng.random_sample() == np_rng.random_sample(), order
        assert arena.py_rng.random() == py_rng.random(), order


# (depth of the solving player, depth of its opponent, the solving player is Black): found on the
# CPU oracle: the host game with the exact endgame differs from the one without in a move
SOLVE_CASE = (2, 1, True)


def test_solve_empties_switches_to_the_solver():
    bs = 6
    depth, other, is_black = SOLVE_CASE
    plain = {"s": (depth, 0), "o": (other, 0)}
    exact = {"s": (depth, 6), "o": (other, 0)}
    black, white = (["s"], ["o"]) if is_black else (["o"], ["s"])
    h_plain = host_game(bs, plain[black[0]], plain[white[0]])
    h_exact = host_game(bs, exact[black[0]], exact[white[0]])
    assert h_plain[1] != h_exact[1]                  # the switch is seen
    first = next(i for i, (a, b) in enumerate(zip(h_plain[1], h_exact[1])) if a != b)
    assert bs * bs - 4 - first <= 6                  # and it happens in the solved endgame
    assert _arena(bs, 0, exact).play_games(black, white) == [h_exact[0]]
    assert _arena(bs, 0, plain).play_games(black, white) == [h_plain[0]]
    # the board after every ply, not only the result: one lockstep batch of both games' plies
    from rvz.arena import AlphaBetaPlayer
    pl = AlphaBetaPlayer("s", depth=depth, board_size=bs, solve_empties=6)
    g = R.O.new_game(bs)
    rows, want = [], []
    for sq in h_exact[1]:
        if (g.side == 1) == is_black:
            rows.append(g.copy())
            want.append(sq)
        assert R.O.make_move(g, sq, bs)
    got = pl.moves(*R.to_device(rows))
    assert list(got) == want


def test_an_abandoned_row_raises():
    from rvz.arena import AlphaBetaPlayer
    pl = AlphaBetaPlayer("x", depth=4, board_size=8, node_limit=10)
    with pytest.raises(RuntimeError):
        pl.moves(*R.to_device([R.O.new_game(8)]))
    # a row the solver abandons keeps the alpha-beta move
    g = R.position(1, 9, 8)[0]
    k_ab = A.negamax(g, 1, A.default_table(8), 8)[2]
    pl = AlphaBetaPlayer("x", depth=1, board_size=8, solve_empties=9, node_limit=k_ab)
    assert R.solved(1, 9, 8)[2] > k_ab
    assert list(pl.moves(*R.to_device([g]))) == [A.alphabeta(g, 1, A.default_table(8), 8)[1]]


def _tournament(seed):
    import rvz
    from rvz.arena import AlphaBetaPlayer, Arena, ELOPlayer
    torch.manual_seed(0)
    net = rvz.AlphaZeroNetwork(8, 6, 64)
    arena = Arena(seed=seed)
    # 64 simulations in four leaf batches: a one-batch search only expands the root
    arena.add_player(ELOPlayer("net", net, {"num_simulations": 64, "batch_size": 16}))
    arena.add_player(ELOPlayer("random", None))
    arena.add_player(AlphaBetaPlayer("ab2", depth=2))
    res = arena.run_tournament(rounds=4)
    return arena, res


def test_tournament_with_all_three_player_kinds(capsys):
    arena, res = _tournament(4)
    assert res["games_played"] == 4 * 3
    for m in res["matchups"].values():
        assert m["games_played"] == 4 and m["wins1"] + m["wins2"] + m["draws"] == 4
    assert sum(r["games_played"] for r in res["leaderboard"]) == 2 * 12
    assert all(r["games_played"] == 8 for r in res["leaderboard"])
    assert len(arena.elo.history) == 12
    assert abs(sum(r["rating"] for r in res["leaderboard"]) - 3 * 1500.0) < 1e-6
    # only the 8 games with the random player take a pass each
    assert arena.reference_order_passes <= 8 + 3
    again, res2 = _tournament(4)
    strip = lambda h: [{k: v for k, v in r.items() if k != "timestamp"} for r in h]
    assert strip(again.elo.history) == strip(arena.elo.history)
    assert res2["leaderboard"] == res["leaderboard"]
    assert again.np_rng.random_sample() == arena.np_rng.random_sample()
    assert again.py_rng.random() == arena.py_rng.random()
