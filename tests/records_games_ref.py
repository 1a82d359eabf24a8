"""A plain Python / NumPy restatement of rvz_records_games (include/rvz.h has the walk), its rules
taken from the oracle's make_move, and the synthetic windows the CPU and GPU tests cut: seeded
random playouts laid out as [plies][slots], a slot's games restarting right after they end."""
import numpy as np

STATS = ("rows", "games", "open", "abandoned", "malformed", "headless_games", "earlier", "zero")


def walk(O, bs, black, white, side, idx, emit_from):
    """The walk of every slot. black / white uint64, side / idx int32, all [P, G]. Returns
    (state int32 [P, G], value int32 [P, G] (meaningful where state == 1), rows: the emitted
    records (p, g) slot-major, stats int64 [8])."""
    P, G = idx.shape
    nsq = bs * bs
    full = (1 << nsq) - 1
    first = O.new_game(bs)
    start = (int(first.black), int(first.white), 1)
    state = np.zeros((P, G), np.int32)
    value = np.zeros((P, G), np.int32)
    stats = np.zeros(8, np.int64)
    rows = []
    for g in range(G):
        seg, cur, headless = [], None, False
        for p in range(P):
            i = int(idx[p, g])
            if i < 0:
                state[p, g] = -1
                continue
            b, w, s = int(black[p, g]), int(white[p, g]), int(side[p, g])
            ok = not (b & w) and not ((b | w) & ~full) and s in (1, 2) and i <= nsq
            chained = cur is not None and (b, w, s) == (int(cur.black), int(cur.white),
                                                        int(cur.side))
            if ok and cur is not None and not chained:          # the chain is broken
                state[seg, g] = 3
                stats[3] += len(seg)
                seg, cur = [], None
            t = None
            if ok:
                t = cur.copy() if chained else O.Game(b, w, s, 0, -1, 0)
                ok = O.make_move(t, -1 if i == nsq else i, bs)
            if not ok:
                state[p, g] = -5
                stats[4] += 1
                state[seg, g] = 3
                stats[3] += len(seg)
                seg, cur = [], None
                continue
            if cur is None:
                headless = (b, w, s) != start
            seg.append(p)
            cur = t
            if t.over:
                win = int(t.winner)
                if p >= emit_from:
                    for q in seg:
                        state[q, g] = 1
                        value[q, g] = 0 if win == 0 else (1 if win == int(side[q, g]) else -1)
                        rows.append((q, g))
                    stats[1] += 1
                    stats[5] += int(headless)
                else:
                    state[seg, g] = 2
                    stats[6] += len(seg)
                seg, cur = [], None
        stats[2] += len(seg)                                    # still open: state 0
    stats[0] = len(rows)
    return state, value, rows, stats


def games(O, bs, black, white, side, idx, p, emit_from=0):
    """rvz.records_games' dict as NumPy arrays, the row arrays at length m."""
    P, G = idx.shape
    state, value, rows, stats = walk(O, bs, black, white, side, idx, emit_from)
    q = np.array([r[0] for r in rows], np.int64)
    g = np.array([r[1] for r in rows], np.int64)
    b, w, s = black[q, g], white[q, g], side[q, g]
    return {"m": len(rows), "mover": np.where(s == 1, b, w).astype(np.uint64),
            "opponent": np.where(s == 1, w, b).astype(np.uint64),
            "policy": p[q, g].astype(np.float32).reshape(len(rows), bs * bs + 1),
            "value": value[q, g].astype(np.float32), "src": (q * G + g).astype(np.int32),
            "state": state, "stats": stats}


def stream(O, bs, rng, n, offset=0, gaps=(), pass_record=False):
    """n entries of one slot's column: the records (black, white, side, idx) of consecutive
    random games, the next game starting right after one ends. offset: the first `offset`
    records are dropped (the window opens inside a game). pass_record: after the first auto-pass
    that does not end its game, one extra record of the side that had to pass, with the pass
    index. gaps: plies that hold no record (None); later records move down."""
    out = []
    game = O.new_game(bs)
    while len(out) < n + offset:
        mine, theirs = ((game.black, game.white) if game.side == 1 else
                        (game.white, game.black))
        mask = O.legal(int(mine), int(theirs), bs)
        sq = int(rng.choice([s for s in range(bs * bs) if mask >> s & 1]))
        mover = int(game.side)
        out.append((int(game.black), int(game.white), mover, sq))
        assert O.make_move(game, sq, bs)
        if game.over:
            game = O.new_game(bs)
        elif pass_record and int(game.side) == mover:
            out.append((int(game.black), int(game.white), 3 - mover, bs * bs))
            pass_record = False
    out = out[offset:]
    for ply in sorted(gaps):
        out.insert(ply, None)
    return out[:n]


def window(O, bs, P, G, seed, offsets=None, gaps=None, pass_slots=()):
    """A synthetic window: (black uint64, white uint64, side int32, idx int32, all [P, G], p
    float64 [P, G, S*S+1]). offsets / gaps: {slot: stream()'s argument}; pass_slots: the slots
    that get a pass-index record. A ply without a record holds idx = -2 and stale bytes."""
    rng = np.random.default_rng(seed)
    npol = bs * bs + 1
    black = rng.integers(0, 2 ** 36, (P, G)).astype(np.uint64)   # stale bytes, never read
    white = rng.integers(0, 2 ** 36, (P, G)).astype(np.uint64)
    side = np.zeros((P, G), np.int32)
    idx = np.full((P, G), -2, np.int32)
    p = rng.random((P, G, npol))
    p /= p.sum(axis=2, keepdims=True)
    for g in range(G):
        col = stream(O, bs, rng, P, (offsets or {}).get(g, 0), (gaps or {}).get(g, ()),
                     g in pass_slots)
        for k, rec in enumerate(col):
            if rec is not None:
                black[k, g], white[k, g], side[k, g], idx[k, g] = rec
    return black, white, side, idx, p


def edge_window(O, bs, P, G, seed):
    """The window of the tests' edge cases: slots 3 and 9 open inside a game (headless first
    segments), slot 4 has gaps inside its first game and slot 11 one at the last ply, slots 12 ..
    39 each carry a pass-index record where their games have an auto-pass to hang it on."""
    return window(O, bs, P, G, seed, offsets={3: 5, 9: 17}, gaps={4: (6, 7, 20), 11: (P - 1,)},
                  pass_slots=range(12, 40))


def tensors(black, white, side, idx, p, device="cpu"):
    """The window as rvz.records_games' five tensors."""
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in
                 (black.view(np.int64), white.view(np.int64), side, idx, p))
