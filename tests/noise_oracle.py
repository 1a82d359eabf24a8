"""The literal CPU oracle (oracle/) driven with Dirichlet noise at the search roots, the checker of
tests/test_gpu_root_noise.py. The oracle takes probabilities per leaf (rvzo_search_submit), so
the noise is mixed here, in NumPy float32, into the softmaxed row of each search's FIRST submit
(whose leaf is the root for every live game):

    P'(s) = fl32(fl32((1 - eps) * P(s)) + fl32(eps * eta(s)))   over the root's legal squares,

eps = float32(epsilon), 1 - eps = float32(1) - eps, eta from rvz.dirichlet_noise (the engine's own
device function) for the root's legal mask, the game's seed and the root's disc count.
The softmaxed row is rvz.policy_softmax's by default: borrowing it is licensed by
tests/test_gpu_policy_softmax.py, which holds it to a float64 reference at every output.
Test infrastructure only (the pattern of tests/oracle_play.py)."""
from __future__ import annotations

import numpy as np
import torch


def root_eta(O, games, seeds, salt, alpha, bs=8, device="cuda"):
    """eta rows float32 [n, npol] of the given root positions (oracle Game structs)."""
    import rvz
    legal, tags = [], []
    for g in games:
        P, Opp = (g.black, g.white) if g.side == 1 else (g.white, g.black)
        legal.append(0 if g.over else O.legal(int(P), int(Opp), bs))
        tags.append(bin(int(g.black) | int(g.white)).count("1"))
    lg = torch.from_numpy(np.array(legal, np.uint64).view(np.int64)).to(device)
    sd = torch.tensor([int(s) & 0xFFFFFFFF for s in seeds], dtype=torch.int64, device=device)
    tg = torch.tensor(tags, dtype=torch.int32, device=device)
    eta = rvz.dirichlet_noise(lg, sd, tg, salt, alpha, board_size=bs).cpu().numpy()
    return eta, np.array(legal, np.uint64)


def mix(probs, eta, legal, eps, bs=8):
    """The formula above on rows float32 [n, npol], at the legal squares only."""
    e = np.float32(eps)
    om = np.float32(1.0) - e
    out = probs.astype(np.float32).copy()
    nsq = bs * bs
    mixed = (om * out[:, :nsq]).astype(np.float32) + (e * eta[:, :nsq]).astype(np.float32)
    mask = ((legal[:, None] >> np.arange(nsq, dtype=np.uint64)[None, :]) & np.uint64(1)) != 0
    out[:, :nsq] = np.where(mask, mixed.astype(np.float32), out[:, :nsq])
    return out


class NoisyOracleGames:
    def __init__(self, O, seeds, sims, batch, alpha, eps, salt=0, temperature=1.0, bs=8,
                 softmax=None):
        import rvz
        self.O, self.bs, self.S, self.B, self.T = O, bs, int(sims), int(batch), float(temperature)
        self.alpha, self.eps, self.salt = alpha, eps, salt
        self.seeds = [int(s) for s in seeds]
        self.games = [O.new_game(bs) for _ in seeds]
        self.mts = [O.MT(s) for s in self.seeds]
        self.softmax = softmax or (lambda lg: rvz.policy_softmax(lg, bs))

    def ply(self, ev):
        """One ply of every game: (visits int32 [n, npol], idx [n], p f64 [n, npol])."""
        O, bs = self.O, self.bs
        srch = O.Search(len(self.games), self.S, self.B, 1.0, bs=bs)
        srch.begin(self.games)
        first = True
        while (r := srch.step()) is not None:
            x = torch.from_numpy(O.leaf_planes(r[0], bs)).to(ev.device)
            logits, value = ev(x)
            probs = self.softmax(logits).cpu().numpy()
            if first and self.eps > 0:      # every queued leaf of the first batch is a root
                eta, legal = root_eta(O, self.games, self.seeds, self.salt, self.alpha, bs,
                                      ev.device)
                probs = mix(probs, eta, legal, self.eps, bs)
            first = False
            srch.submit(probs, value.cpu().numpy())
        vis = srch.visits()
        idx, ps = [], []
        for j, g in enumerate(self.games):
            if g.over:
                idx.append(-2)
                ps.append(np.zeros(bs * bs + 1))
                continue
            u = self.mts[j].random_sample() if O.action_needs_draw(vis[j], self.T) else 0.0
            a, p, _ = O.action(vis[j], self.T, u)
            assert O.make_move(g, -1 if a == bs * bs else a, bs)
            idx.append(a)
            ps.append(p)
        return vis, np.array(idx), np.stack(ps)
