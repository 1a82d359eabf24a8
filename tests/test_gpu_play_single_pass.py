"""The one-board pass of the fused self-play kernel (k_play<64, 2, 2, 4, 8, 2>, C2): a trunk pass
whose second board does not exist runs that board alone at the one-board tile shape
(h2_pass_single: half the pixel tiles, no interleave) instead of the pair shape over a zero board.
A row's outputs must be bitwise the pair shape's, so the games stay those of the pull-style runner
(k_resnet_h2's pair passes; it never takes the new path): every ply's moves, the boards, statuses,
counters, seeds and f64 policies are compared bit for bit. RVZ_PLAY_SINGLE_PASS=0 (read by the
library in rvz_play) runs the pair shape everywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# S = 320: five batches, so the visits depend on the net and the games diverge (with two batches
# every slot plays one game, mcts.py:96-97)
G, S, PLIES = 37, 320, 12


def _net(board, blocks, filters, seed=0):
    import rvz
    torch.manual_seed(seed)
    return rvz.AlphaZeroNetwork(board, blocks, filters).cuda().eval()


def _plain(net, G, S, plies, memo, skip, seed_base=42):
    import rvz
    run = rvz.SelfPlayRunner(rvz.Engine(G, S, 64, board_size=net.board_size, compact_leaves=True,
                                        memo=memo),
                             rvz.LeafEvaluator(net), autoreset=True, seed_base=seed_base,
                             skip_last_eval=skip)
    run.start()
    moves = []
    for _ in range(plies):
        run.ply()
        moves.append(run.eng.idx_buf.clone())
    return run, torch.stack(moves)


def _fused(net, G, S, plies, memo, skip, seed_base=42, gpw=0):
    import rvz
    eng = rvz.Engine(G, S, 64, board_size=net.board_size, memo=memo)
    run = rvz.SelfPlayRunner(eng, rvz.LeafEvaluator(net), autoreset=True, seed_base=seed_base,
                             skip_last_eval=skip, fused=True)
    run.start()
    hist = torch.full((plies, G), -9, dtype=torch.int32, device="cuda")
    eng.play(run.evaluator, plies, 1.0, run.seeds, run.seed_stride, run._plies, run._done,
             reset=True, skip_last_eval=skip, hist=hist, games_per_workgroup=gpw)
    return run, hist


def _same(a, b):
    (ra, ma), (rb, mb) = a, b
    assert ma.shape == mb.shape
    for k in range(ma.shape[0]):
        assert torch.equal(ma[k], mb[k]), f"ply {k}: {int((ma[k] != mb[k]).sum())} games differ"
    for x, y in zip(ra.eng.get_state(), rb.eng.get_state()):
        assert torch.equal(x, y)
    assert torch.equal(ra._plies, rb._plies) and torch.equal(ra._done, rb._done)
    assert torch.equal(ra.seeds, rb.seeds)
    assert torch.equal(ra.eng.p_buf, rb.eng.p_buf)
    ra.eng.check()
    rb.eng.check()


@pytest.fixture(scope="module")
def runner_games():
    """The pull-style runner's games of the 2x64 net: computed once, only read by the tests."""
    net = _net(8, 2, 64, seed=3)
    ref = _plain(net, G, S, PLIES, True, True)
    assert len(set(ref[1][3].tolist())) > 1                # distinct games by the fourth ply
    return net, ref


@pytest.mark.parametrize("gpw", [1, -1], ids=["static1", "queue1"])
def test_every_pass_single(runner_games, gpw):
    """One game per workgroup (static) or per queue group: every cycle queues at most one row,
    so every trunk pass has one live board and runs the one-board shape."""
    net, ref = runner_games
    a = _fused(net, G, S, PLIES, True, True, gpw=gpw)
    assert len(set(a[1][3].tolist())) > 1
    _same(a, ref)


@pytest.mark.parametrize("gpw", [3, -3, -6], ids=["static3", "queue3", "queue6"])
def test_mixed_passes(runner_games, gpw):
    """Groups of 3 (static, queue) and 6 games (bench.py's): a cycle queues 0..3 or 0..6 rows, so
    pair passes, one-board passes and rows held one cycle mix."""
    net, ref = runner_games
    a = _fused(net, G, S, PLIES, True, True, gpw=gpw)
    assert len(set(a[1][3].tolist())) > 1
    _same(a, ref)


_CHILD = r"""
import os, sys
import numpy as np
import torch
root, out, gpw = sys.argv[1], sys.argv[2], int(sys.argv[3])
sys.path.insert(0, os.path.join(root, "alphazero-reversi_amd"))
sys.path.insert(0, os.path.join(root, "tests"))
import test_gpu_play_single_pass as T
net = T._net(8, 2, 64, seed=3)
run, hist = T._fused(net, T.G, T.S, T.PLIES, True, True, gpw=gpw)
run.eng.check()
bl, wh, st = run.eng.get_state()
torch.cuda.synchronize()
np.savez(out, moves=hist.cpu().numpy(), black=bl.cpu().numpy(), white=wh.cpu().numpy(),
         status=st.cpu().numpy(), plies=run._plies.cpu().numpy(), done=run._done.cpu().numpy(),
         seeds=run.seeds.cpu().numpy(), policy=run.eng.p_buf.cpu().numpy().view(np.int64))
"""


def test_single_pass_knob(runner_games, tmp_path):
    """RVZ_PLAY_SINGLE_PASS=0 (the pair shape everywhere) and the default (on) leave the same
    arrays, and the runner's moves. Each setting in a fresh process: the library reads the
    variable, and the environment is a process's."""
    _, ref = runner_games
    dumps = []
    for knob in ("0", "1"):
        out = str(tmp_path / f"knob{knob}.npz")
        env = dict(os.environ, RVZ_PLAY_SINGLE_PASS=knob)
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out, "-6"], env=env,
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        dumps.append(np.load(out))
    off, on = dumps
    assert sorted(off.files) == sorted(on.files)
    for k in off.files:
        assert np.array_equal(off[k], on[k]), k
    assert np.array_equal(on["moves"], ref[1].cpu().numpy())
    assert len(set(on["moves"][3].tolist())) > 1


def test_ranged_rerun_on_a_single_pass():
    """The loud-stem net of test_fused_ranged_rerun_is_per_board (stem channels 0-7 at 2e5, past
    f16's 65520, where the mover has >= 7 discs in a 3x3 window; they feed only the skip path)
    with one game per workgroup: every pass is a one-board pass, and a board that overflows is
    re-run with its image scaled inside the one-board function. The runner's games, no overflow
    left."""
    import rvz
    net = _net(8, 2, 64, seed=2)
    W = 2e5
    with torch.no_grad():
        net.conv.weight[:8].zero_()
        net.conv.weight[:8, 0] = W
        if net.conv.bias is not None:
            net.conv.bias[:8].zero_()
        net.bn.running_mean[:8] = 0.0
        net.bn.running_var[:8] = 1.0 - net.bn.eps
        net.bn.weight[:8] = 1.0
        net.bn.bias[:8] = -6.5 * W
        for blk in net.res_blocks:
            blk.conv1.weight[:, :8] = 0.0
        for m in (net.policy_conv, net.value_conv):
            m.weight[:, :8] = 0.0
    Gr, Sr, plies = 48, 320, 40
    bits = np.arange(64, dtype=np.uint64)

    def loud_boards(eng):      # boards whose mover has a window of >= 7 discs (stem past 65520)
        state = eng.get_state()
        torch.cuda.synchronize()
        bl, wh, st = (t.cpu().numpy() for t in state)
        mover = np.where((st[:, 0] == 1)[:, None], bl.view(np.uint64)[:, None],
                         wh.view(np.uint64)[:, None])
        grid = ((mover >> bits) & np.uint64(1)).astype(np.int32).reshape(Gr, 8, 8)
        pad = np.pad(grid, ((0, 0), (1, 1), (1, 1)))
        win = sum(pad[:, 1 + dr:1 + dr + 8, 1 + dc:1 + dc + 8]
                  for dr in (-1, 0, 1) for dc in (-1, 0, 1))
        return int((win >= 7).any(axis=(1, 2)).sum())

    run = rvz.SelfPlayRunner(rvz.Engine(Gr, Sr, 64, compact_leaves=True, memo=True),
                             rvz.LeafEvaluator(net), autoreset=True, seed_base=42,
                             skip_last_eval=True)
    run.start()
    moves, counts = [], []
    for _ in range(plies):
        run.ply()
        moves.append(run.eng.idx_buf.clone())
        counts.append(loud_boards(run.eng))
    assert any(c > 0 for c in counts), str(counts)   # some searches start from a loud root
    a = _fused(net, Gr, Sr, plies, True, True, gpw=1)
    assert len(set(a[1][3].tolist())) > 1
    _same(a, (run, torch.stack(moves)))
    for r in (a[0], run):
        assert not r.evaluator.overflowed()
