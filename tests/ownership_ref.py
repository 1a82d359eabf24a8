"""Plain Python / NumPy restatements of the three final-ownership calls (include/rvz.h has the
definitions): rvz_records_final (`final`, its rules the oracle's make_move, as
tests/records_games_ref.py takes them), rvz_replay_ownership (`ownership`, NumPy's rot90 / fliplr
being the definition of the symmetries) and rvz_ownership_loss (`loss`, float64), and the same
through torch tensors in the result layouts of the rvz functions (`as_finaler`, `as_batcher`,
`as_kernel`) for the tests on a host without a GPU."""
import numpy as np


def final(O, bs, black, white, side, idx, src, count=None):
    """rvz_records_final. black / white uint64, side / idx int32, all [P, G]; src int [n]; count
    None or an int. Returns (final_mover uint64 [n], final_opponent uint64 [n], ok int32 [n],
    stats int64 [4], handled: the number of rows written, code int32 [n]: 1 ok, 2 open, 3 any
    other handled row, 0 a row beyond the bound)."""
    P, G = idx.shape
    nsq = bs * bs
    full = (1 << nsq) - 1
    n = len(src)
    bound = n if count is None else max(0, min(n, int(count)))
    fm, fo = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    ok = np.zeros(n, np.int32)
    stats = np.zeros(4, np.int64)
    codes = np.zeros(n, np.int32)
    for j in range(bound):
        stats[0] += 1
        s = int(src[j])
        if not 0 <= s < P * G or idx.reshape(-1)[s] < 0:
            stats[3] += 1
            codes[j] = 3
            continue
        p0, g = divmod(s, G)
        cur, mover, code = None, 0, 2                       # 2: the game is still open
        for p in range(p0, P):
            i = int(idx[p, g])
            if i < 0:
                continue
            b, w, sd = int(black[p, g]), int(white[p, g]), int(side[p, g])
            good = not (b & w) and not ((b | w) & ~full) and sd in (1, 2) and i <= nsq
            if good and cur is not None:
                good = (b, w, sd) == (int(cur.black), int(cur.white), int(cur.side))
            if good:
                if cur is None:
                    cur, mover = O.Game(b, w, sd, 0, -1, 0), sd
                good = O.make_move(cur, -1 if i == nsq else i, bs)
            if not good:
                code = 3
                break
            if cur.over:
                code = 1
                break
        stats[code] += 1
        codes[j] = code
        if code == 1:
            B, W = int(cur.black), int(cur.white)
            fm[j], fo[j], ok[j] = (B, W, 1) if mover == 1 else (W, B, 1)
    return fm, fo, ok, stats, bound, codes


def bits(x, bs):
    """A bitboard as an S x S 0/1 array, bit r * S + c at [r, c]."""
    return np.array([(int(x) >> s) & 1 for s in range(bs * bs)], np.int64).reshape(bs, bs)


def image(x, k):
    """T_k(x) = fliplr^f(rot90^r(x)), k = 4f + r (include/rvz.h)."""
    y = np.rot90(x, k & 3)
    return np.fliplr(y) if k & 4 else y


def ownership(bs, final_mover, final_opponent, slot, sym):
    """rvz_replay_ownership. final_mover / final_opponent uint64 [capacity], slot / sym int [nb].
    Returns (own float32 [nb, S*S], margin float32 [nb])."""
    nsq = bs * bs
    full = (1 << nsq) - 1
    nb = len(slot)
    own, margin = np.zeros((nb, nsq), np.float32), np.zeros(nb, np.float32)
    for r in range(nb):
        s, k = int(slot[r]), int(sym[r])
        if not (0 <= s < len(final_mover) and 0 <= k < 8):
            continue
        P, Q = int(final_mover[s]), int(final_opponent[s])
        if (P & Q) or ((P | Q) & ~full):
            continue
        own[r] = image(bits(P, bs) - bits(Q, bs), k).reshape(-1)
        margin[r] = bin(P).count("1") - bin(Q).count("1")
    return own, margin


def loss(logits, target, weight=None):
    """rvz_ownership_loss. Returns a dict: out_loss float64 [8] (rvz_policy_value_loss's layout:
    {L, L, 0, 0, W, agreement, malformed, 0}), rows float64 [n, 2] ({L, agree}), grad_logits
    float32 [n, S*S]."""
    o32, t32 = np.asarray(logits, np.float32), np.asarray(target, np.float32)
    n, nsq = o32.shape
    wt = np.ones(n, np.float32) if weight is None else np.asarray(weight, np.float32)
    rows, omega = np.zeros((n, 2)), np.zeros(n)
    th = np.zeros((n, nsq))
    bad = 0
    for r in range(n):
        if not np.isfinite(o32[r]).all() or not np.isin(t32[r], (-1.0, 0.0, 1.0)).all() or \
                not (wt[r] >= 0 and np.isfinite(wt[r])):
            bad += 1
            continue
        o, t = o32[r].astype(np.float64), t32[r].astype(np.float64)
        th[r] = np.tanh(o)
        labelled = t != 0
        hits = ((t > 0) & (o > 0)) | ((t < 0) & (o < 0))
        rows[r] = (((th[r] - t) ** 2).sum() / nsq,
                   hits.sum() / labelled.sum() if labelled.any() else 0.0)
        omega[r] = np.float64(wt[r])
    W = omega.sum()
    out = np.zeros(8)
    out[4], out[6] = W, bad
    grad = np.zeros((n, nsq), np.float32)
    if W > 0:
        out[0] = out[1] = (omega * rows[:, 0]).sum() / W
        out[5] = (omega * rows[:, 1]).sum() / W
        for r in range(n):
            if omega[r] > 0:
                t = t32[r].astype(np.float64)
                grad[r] = ((omega[r] / W) * (2.0 / nsq) * (th[r] - t) *
                           (1.0 - th[r] * th[r])).astype(np.float32)
    return {"out_loss": out, "rows": rows, "grad_logits": grad}


# ---------------------------------------------------------------- the rvz functions' layouts
def as_finaler(O):
    """`final` with rvz.records_final's signature and result dict, on CPU tensors."""
    import torch

    def finaler(rec_black, rec_white, rec_side, rec_idx, src, count=None, board_size=8):
        fm, fo, ok, stats = final(O, board_size, rec_black.numpy().view(np.uint64),
                                     rec_white.numpy().view(np.uint64),
                                     rec_side.numpy().astype(np.int32),
                                     rec_idx.numpy().astype(np.int32), src.numpy(),
                                     None if count is None else int(count))[:4]
        return {"final_mover": torch.from_numpy(fm.view(np.int64)),
                "final_opponent": torch.from_numpy(fo.view(np.int64)),
                "ok": torch.from_numpy(ok), "stats": torch.from_numpy(stats)}
    return finaler


def as_batcher(final_mover, final_opponent, slot, sym, board_size=8):
    """`ownership` with rvz.replay_ownership's signature and results, on CPU tensors."""
    import torch
    own, margin = ownership(board_size, final_mover.numpy().view(np.uint64),
                            final_opponent.numpy().view(np.uint64), slot.numpy(), sym.numpy())
    return torch.from_numpy(own), torch.from_numpy(margin)


def as_kernel(logits, targets, weights=None, board_size=8, rows=False, grads=True):
    """`loss` with rvz.ownership_loss's signature and result dict, on CPU tensors."""
    import torch
    assert logits.shape[1] == board_size * board_size
    ref = loss(logits.detach().numpy(), targets.numpy(),
               None if weights is None else weights.numpy())
    out_loss = torch.from_numpy(ref["out_loss"])
    out = {"out_loss": out_loss, "loss": out_loss[0], "weight_sum": out_loss[4],
           "agreement": out_loss[5], "malformed": out_loss[6]}
    if rows:
        out["rows"] = torch.from_numpy(ref["rows"])
    if grads:
        out["grad_logits"] = torch.from_numpy(ref["grad_logits"])
    return out
