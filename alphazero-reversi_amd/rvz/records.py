"""Training records on the device: the stateless wrappers of the C-ABI's record entry points
(include/rvz.h): board symmetries, merge_positions, the replay ring's draws and the cut of autoreset
self-play records into finished games. Every argument rule
is one private helper that raises ``RvzError``, its message beginning with the caller's name,
before any device call; what counts as an int or as a number in a range is ``_lib.is_int`` and
``_lib.is_number``, for the whole package."""
from __future__ import annotations

import numbers
from typing import Optional

import torch

from . import _lib
from ._lib import RvzError, check, check_board_size, is_int, is_number, ptr

_U64 = 2 ** 64 - 1


# ------------------------------------------------------------------ the argument rules
def _ints(who: str, **named) -> None:
    for name, x in named.items():
        if not is_int(x):
            raise RvzError(f"{who}: {name} is an int, not {x!r}")


def _bitboards(who: str, a: torch.Tensor, b: torch.Tensor, names: str, per: str,
               status: Optional[torch.Tensor] = None) -> int:
    """int64 [n] bit patterns (and the rows' status [n, 4], where there is one); returns n."""
    n = a.numel()
    if a.dim() != 1 or b.shape != (n,):
        raise RvzError(f"{who}: {names} hold one entry per {per}")
    if a.dtype != torch.int64 or b.dtype != torch.int64:
        raise RvzError(f"{who}: {names} are int64 bit patterns")
    if status is not None and status.shape != (n, 4):
        raise RvzError(f"{who}: status is [n, 4], one row per entry of {names}")
    return n


def _targets(who: str, n: int, npol: int, policy: torch.Tensor,
             value: Optional[torch.Tensor] = None, rows: str = "n") -> None:
    if policy.shape != (n, npol) or policy.dtype != torch.float32:
        raise RvzError(f"{who}: policy must be float32 [{rows}, {npol}]")
    if value is not None and (value.shape not in ((n,), (n, 1)) or value.dtype != torch.float32):
        raise RvzError(f"{who}: value must be float32 [{rows}] or [{rows}, 1]")


def _fits_int32(who: str, rows: int, npol: int, what: str) -> None:
    if not 0 <= rows * npol < 2 ** 31:
        raise RvzError(f"{who}: {what} must be >= 0 and {what} * (S*S + 1) fit int32")


def _ring(who: str, cap: int, start: int, live: int, min_live: int) -> None:
    if cap < 1 or cap >= 2 ** 31:
        raise RvzError(f"{who}: the ring holds between 1 and 2^31 - 1 slots")
    if not min_live <= live <= cap or not 0 <= start < cap:
        raise RvzError(f"{who}: live = {live} must be in [{min_live}, {cap}] and start = {start} "
                       f"in [0, {cap})")


def _given(who: str, n: int, per: str, optional: bool = True, **named) -> None:
    """Integers given per row (idx, sym): [n], not float or bool; None where optional."""
    for name, x in named.items():
        if (not optional if x is None else
                x.shape != (n,) or x.dtype.is_floating_point or x.dtype == torch.bool):
            raise RvzError(f"{who}: {name} holds one integer per {per}")


def _i32(x: Optional[torch.Tensor], dev) -> Optional[torch.Tensor]:
    return None if x is None else x.to(dev, torch.int32).contiguous()


def _addr(t: Optional[torch.Tensor]):
    """Device address of a contiguous device tensor that a kernel reads and writes in single
    elements (ptr() also asks for the 16-byte alignment of vector accesses)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RvzError("rvz buffers must be device tensors (no host fallback)")
    if not t.is_contiguous():
        raise RvzError("rvz buffers must be contiguous")
    return t.data_ptr()


# ------------------------------------------------------------------ board symmetries
# include/rvz.h: k = 4*f + r, T_k(x) = fliplr(rot90(x, r)) if f else rot90(x, r);
# T_k(x)[i][j] = x[_sym_src(k, i, j, S)]
def _sym_src(k: int, i: int, j: int, S: int):
    if k & 4:
        j = S - 1 - j
    return ((i, j), (j, S - 1 - i), (S - 1 - i, S - 1 - j), (S - 1 - j, i))[k & 3]


# each T_k as the permutation of a 3x3 board's squares (3x3 tells all eight apart)
_SYM_PERMS = [tuple(3 * a + b for a, b in (_sym_src(k, i, j, 3) for i in range(3) for j in range(3)))
              for k in range(8)]


def _sym_index(k, what: str) -> int:
    if not is_int(k) or not 0 <= k < 8:
        raise RvzError(f"{what}: a symmetry is an int in [0, 8), not {k!r}")
    return int(k)


def symmetry_compose(a: int, b: int) -> int:
    """The symmetry c with T_c(x) == T_a(T_b(x)) for every board x (b is applied first)."""
    a, b = _sym_index(a, "symmetry_compose"), _sym_index(b, "symmetry_compose")
    # T_a(T_b(x))[s] = T_b(x)[src_a(s)] = x[src_b(src_a(s))]
    return _SYM_PERMS.index(tuple(_SYM_PERMS[b][s] for s in _SYM_PERMS[a]))


def symmetry_inverse(k: int) -> int:
    """The symmetry c with T_c(T_k(x)) == x for every board x."""
    k = _sym_index(k, "symmetry_inverse")
    return next(c for c in range(8) if symmetry_compose(c, k) == 0)


def board_symmetry(black: torch.Tensor, white: torch.Tensor, sym: torch.Tensor,
                   board_size: int = 8):
    """rvz_board_symmetry: the images of n boards under the eight symmetries of the square board
    (include/rvz.h has the numbering). black / white int64 [n] (bit patterns), sym [n] integers,
    device tensors. Returns (black', white') int64 [n]: row i transformed by T_sym[i]; both 0 for
    a sym[i] outside [0, 8). On 6x6 input bits at or above 36 are ignored."""
    who = "board_symmetry"
    check_board_size(board_size)
    lib = _lib.load()
    n = _bitboards(who, black, white, "black and white", "board")
    _given(who, n, "board", optional=False, sym=sym)
    dev = black.device
    b, w = black.contiguous(), white.to(dev).contiguous()
    sy = _i32(sym, dev)
    ob, ow = torch.empty_like(b), torch.empty_like(w)
    if n:
        check(lib.rvz_board_symmetry(board_size, n, ptr(b), ptr(w), ptr(sy), ptr(ob), ptr(ow),
                                     _lib.stream_handle(dev)), None, "rvz_board_symmetry")
    return ob, ow


def training_rows(black: torch.Tensor, white: torch.Tensor, status: torch.Tensor,
                  policy: torch.Tensor, sym: Optional[torch.Tensor] = None, board_size: int = 8,
                  all_images: bool = False, quirk: bool = False):
    """rvz_training_rows: augmented training rows straight from the bitboards. black / white
    int64 [n], status int32 [n, 4] (only the side is read), policy float32 [n, S*S+1], device
    tensors. all_images=False: sym [n] integers, output row i is row i's image under T_sym[i].
    all_images=True: sym is ignored, output row 8*i + k is the image under T_k (rows [::8] are the
    untransformed rows). Returns (states float32 [m, 3, S, S], policy float32 [m, S*S+1]) with
    m = n or 8*n, and with quirk=True also quirk int32 [m]: 1 where the engine's own legal mask of
    the image position differs from the image of the original's mask (the third plane is always
    the latter), 0 where they agree, -1 for a row whose sym is outside [0, 8) (a zero row)."""
    who = "training_rows"
    check_board_size(board_size)
    npol = board_size * board_size + 1
    lib = _lib.load()
    n = _bitboards(who, black, white, "black and white", "row", status)
    _targets(who, n, npol, policy)
    fan = 8 if all_images else 1
    _fits_int32(who, n * fan, npol, "n * fan")
    dev = black.device
    if not all_images:
        _given(who, n, "row (or pass all_images=True)", optional=False, sym=sym)
    sy = None if all_images else _i32(sym, dev)
    b, w = black.contiguous(), white.to(dev).contiguous()
    st = _i32(status, dev)
    pol = policy.to(dev).contiguous()
    states = torch.empty(n * fan, 3, board_size, board_size, dtype=torch.float32, device=dev)
    out_p = torch.empty(n * fan, npol, dtype=torch.float32, device=dev)
    q = torch.empty(n * fan, dtype=torch.int32, device=dev) if quirk else None
    if n:
        check(lib.rvz_training_rows(board_size, n, ptr(b), ptr(w), ptr(st), ptr(pol), ptr(sy), fan,
                                    ptr(states), ptr(out_p), ptr(q), _lib.stream_handle(dev)),
              None, "rvz_training_rows")
    return (states, out_p, q) if quirk else (states, out_p)


def merge_positions(black: torch.Tensor, white: torch.Tensor, status: torch.Tensor,
                    policy: torch.Tensor, value: torch.Tensor, board_size: int = 8,
                    table_log2: int = 0, trim: bool = True):
    """rvz_merge_positions: one row per distinct position, carrying the mean of the targets of all
    its occurrences. black / white int64 [n], status int32 [n, 4] (only the side is read), policy
    float32 [n, S*S+1] in [0, 1], value float32 [n] or [n, 1] in [-1, 1], device tensors. Two rows
    are the same position iff their (mover, opponent) bitboards are equal, so a row and its
    colour-swapped twin merge. Returns a dict: "m" the number of distinct positions, and for the
    m positions in order of first occurrence "first" int32 (the lowest input row of the group),
    "count" int32 (its members), "policy" float32 [m, S*S+1] and "value" float32 [m] (the means,
    summed in fixed point: bitwise reproducible; a group of one keeps its row's bits); "group"
    int32 [n] maps every input row to its output row, -1 for a malformed row (overlapping discs,
    bits off the board, a side other than 1 or 2, a target out of range or NaN), which joins no
    group. trim=True: m is an int and the four per-position arrays are sliced to m, at the cost of
    the function's one host read. trim=False: they are returned at length n with the rows from m
    on unwritten, m is a 0-d int32 device tensor and nothing synchronises (with n = 0, m is 0).
    table_log2: 0 for the default hash table, else a table of 2^table_log2 > n slots; the
    results do not depend on it."""
    who = "merge_positions"
    check_board_size(board_size)
    npol = board_size * board_size + 1
    lib = _lib.load()
    n = _bitboards(who, black, white, "black and white", "row", status)
    _targets(who, n, npol, policy, value)
    _fits_int32(who, n, npol, "n")
    _ints(who, table_log2=table_log2)
    size = lib.rvz_merge_scratch_size(board_size, n, int(table_log2))
    if size < 0:
        raise RvzError(f"{who}: table_log2 = {table_log2} must be 0 or give more than "
                       f"n = {n} slots (at most 2^30)")
    dev = black.device
    b, w = black.contiguous(), white.to(dev).contiguous()
    st = _i32(status, dev)
    pol = policy.to(dev).contiguous()
    val = value.to(dev).reshape(n).contiguous()
    m = torch.zeros((), dtype=torch.int32, device=dev)
    first, count, group = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    out_p = torch.empty(n, npol, dtype=torch.float32, device=dev)
    out_v = torch.empty(n, dtype=torch.float32, device=dev)
    if n:
        scratch = torch.empty(size, dtype=torch.uint8, device=dev)
        check(lib.rvz_merge_positions(board_size, n, ptr(b), ptr(w), ptr(st), ptr(pol), ptr(val),
                                      int(table_log2), ptr(scratch), ptr(m), ptr(first),
                                      ptr(count), ptr(out_p), ptr(out_v), ptr(group),
                                      _lib.stream_handle(dev)), None, "rvz_merge_positions")
    if trim:
        m = int(m.item())
        first, count, out_p, out_v = first[:m], count[:m], out_p[:m], out_v[:m]
    return {"m": m, "first": first, "count": count, "policy": out_p, "value": out_v,
            "group": group}


# ------------------------------------------------------------------ the replay ring
def _batch(who: str, mover, opponent, policy, value, start, live, nb, seed, step, idx, sym,
           board_size):
    """What replay_batch and replay_batch_weighted share: the argument rules, the ring (mover,
    opponent, policy, value) and the given (idx, sym) prepared, the five common outputs."""
    check_board_size(board_size)
    npol = board_size * board_size + 1
    lib = _lib.load()
    _ints(who, start=start, live=live, nb=nb, seed=seed, step=step)
    cap = _bitboards(who, mover, opponent, "mover and opponent", "slot")
    _targets(who, cap, npol, policy, value, rows="capacity")
    _ring(who, cap, start, live, 1)
    _fits_int32(who, nb, npol, "nb")
    _given(who, nb, "output row", idx=idx, sym=sym)
    dev = mover.device
    ring = (mover.contiguous(), opponent.to(dev).contiguous(), policy.to(dev).contiguous(),
            value.to(dev).reshape(cap).contiguous())
    given = (_i32(idx, dev), _i32(sym, dev))
    out = (torch.empty(nb, 3, board_size, board_size, dtype=torch.float32, device=dev),
           torch.empty(nb, npol, dtype=torch.float32, device=dev),
           torch.empty(nb, 1, dtype=torch.float32, device=dev),
           torch.empty(nb, dtype=torch.int32, device=dev),
           torch.empty(nb, dtype=torch.int32, device=dev))
    return lib, dev, cap, ring, given, out


def replay_batch(mover: torch.Tensor, opponent: torch.Tensor, policy: torch.Tensor,
                 value: torch.Tensor, start: int, live: int, nb: int, seed: int, step: int,
                 random_sym: bool = True, idx: Optional[torch.Tensor] = None,
                 sym: Optional[torch.Tensor] = None, board_size: int = 8):
    """rvz_replay_batch: nb training rows drawn from a ring of compact records (include/rvz.h has
    the draw). mover / opponent int64 [capacity] (bit patterns), policy float32 [capacity, S*S+1],
    value float32 [capacity] or [capacity, 1], device tensors; the ring's `live` rows start at
    slot `start`, oldest first, and wrap. seed and step are integers taken mod 2^64: row r's record
    and symmetry are a pure function of (seed, step, r). idx [nb] integers: the logical rows to
    take instead of the draw; sym [nb] integers: the symmetries instead of the draw
    (random_sym=False: the identity). Returns (states float32 [nb, 3, S, S], policy float32
    [nb, S*S+1], value float32 [nb, 1], slot int32 [nb], sym int32 [nb]); a row whose given idx is
    outside [0, live) or whose given sym is outside [0, 8) is all zero with sym -1 (and slot -1
    for the idx)."""
    lib, dev, cap, ring, given, out = _batch("replay_batch", mover, opponent, policy, value, start,
                                             live, nb, seed, step, idx, sym, board_size)
    if nb:
        check(lib.rvz_replay_batch(board_size, cap, *map(ptr, ring), int(start), int(live),
                                   int(nb), *map(ptr, given), int(bool(random_sym)),
                                   int(seed) & _U64, int(step) & _U64, *map(ptr, out),
                                   _lib.stream_handle(dev)), None, "rvz_replay_batch")
    return out


def replay_cdf(weight: torch.Tensor, start: int, live: int, tile_log2: int = 0,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rvz_replay_cdf: the table rvz.replay_batch_weighted draws from (include/rvz.h has the
    layout). weight float32 [capacity], the ring's per-slot sampling weights, a device tensor; the
    ring's `live` rows start at slot `start`. A weight w counts as rint(w * 2^16); one that is not
    finite or outside [0, 65536] counts as 0 and is reported in word 1. Returns the table, int64
    (the uint64 words' bit patterns, all below 2^63): word 0 the total, 1 the invalid weights,
    2 start, 3 live, 4 + i the inclusive prefix sum up to logical row i; the words behind 4 + live
    are scratch. out: an int64 device tensor of at least rvz_replay_cdf_size(capacity, tile_log2)
    bytes to build into (a buffer kept across calls); None allocates one. tile_log2: 0, or the
    scan's tile as a power of two in [6, 12]; the table does not depend on it. live = 0 writes
    nothing. Asynchronous on the current stream."""
    who = "replay_cdf"
    lib = _lib.load()
    _ints(who, start=start, live=live, tile_log2=tile_log2)
    cap = weight.numel()
    if weight.dim() != 1 or weight.dtype != torch.float32:
        raise RvzError(f"{who}: weight must be float32 [capacity]")
    _ring(who, cap, start, live, 0)                # a ring with no live rows has a table too
    size = lib.rvz_replay_cdf_size(cap, int(tile_log2))
    if size < 0:
        raise RvzError(f"{who}: tile_log2 = {tile_log2} must be 0 or in [6, 12]")
    dev = weight.device
    if out is None:
        out = torch.empty(size // 8, dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or out.dim() != 1 or out.numel() * 8 < size or \
            out.device != dev or not out.is_contiguous():
        raise RvzError(f"{who}: out must be a contiguous int64 tensor of at least {size // 8} "
                       "words on the weights' device")
    w = weight.contiguous()
    check(lib.rvz_replay_cdf(cap, ptr(w), int(start), int(live), int(tile_log2), ptr(out),
                             _lib.stream_handle(dev)), None, "rvz_replay_cdf")
    return out


def replay_batch_weighted(mover: torch.Tensor, opponent: torch.Tensor, policy: torch.Tensor,
                          value: torch.Tensor, cdf: torch.Tensor, start: int, live: int, nb: int,
                          seed: int, step: int, random_sym: bool = True,
                          idx: Optional[torch.Tensor] = None, sym: Optional[torch.Tensor] = None,
                          word: Optional[torch.Tensor] = None, board_size: int = 8):
    """rvz_replay_batch_weighted: rvz.replay_batch with every row drawn in proportion to its
    sampling weight, through the table `cdf` that rvz.replay_cdf built for the same (start, live).
    word [nb] int64 (uint64 bit patterns): the uniform 64-bit words to draw with instead of the
    generator's. The other arguments are replay_batch's. Returns replay_batch's five outputs and
    prob float32 [nb], the probability q_i / total of each row taken. Row r's symmetry is
    replay_batch's for the same (seed, step, r); its record is not, not even for equal weights.
    Every row is a zero row (slot -1, sym -1, prob 0) when the table was built for another start
    or live, and every drawn one when the weights' total is 0."""
    who = "replay_batch_weighted"
    lib, dev, cap, ring, given, out = _batch(who, mover, opponent, policy, value, start, live, nb,
                                             seed, step, idx, sym, board_size)
    if cdf.dtype != torch.int64 or cdf.dim() != 1 or cdf.numel() < 4 + live or \
            cdf.device != dev or not cdf.is_contiguous():
        raise RvzError(f"{who}: cdf is rvz.replay_cdf's table (contiguous int64, at least "
                       "4 + live words, on the ring's device)")
    if word is not None and (word.shape != (nb,) or word.dtype != torch.int64):    # not int32
        raise RvzError(f"{who}: word holds one int64 (a uint64 bit pattern) per output row")
    wd = None if word is None else word.to(dev).contiguous()
    prob = torch.empty(nb, dtype=torch.float32, device=dev)
    if nb:
        check(lib.rvz_replay_batch_weighted(
            board_size, cap, *map(ptr, ring), ptr(cdf), int(start), int(live), int(nb),
            *map(ptr, given), ptr(wd), int(bool(random_sym)), int(seed) & _U64, int(step) & _U64,
            *map(ptr, out), ptr(prob), _lib.stream_handle(dev)), None, "rvz_replay_batch_weighted")
    return (*out, prob)


# ------------------------------------------------------------------ continuous self-play records
def check_records_args(rec_black, rec_white, rec_side, rec_idx, rec_p, board_size, emit_from,
                       who: str = "records_games"):
    """The argument rules of records_games, checked before any device call (the CPU tests'
    NumPy restatement calls it too); returns (plies, n_games)."""
    check_board_size(board_size, who)
    npol = board_size * board_size + 1
    _ints(who, emit_from=emit_from)
    if not all(isinstance(t, torch.Tensor) for t in (rec_black, rec_white, rec_side, rec_idx,
                                                     rec_p)):
        raise RvzError(f"{who}: the five record arrays are tensors")
    if rec_idx.dim() != 2 or any(t.shape != rec_idx.shape for t in (rec_black, rec_white,
                                                                     rec_side)):
        raise RvzError(f"{who}: rec_black, rec_white, rec_side and rec_idx are [plies, n_games]")
    P, G = rec_idx.shape
    _bitboards(who, rec_black.reshape(-1), rec_white.reshape(-1), "rec_black and rec_white",
               "record")
    _given(who, P * G, "record", optional=False, rec_side=rec_side.reshape(-1),
           rec_idx=rec_idx.reshape(-1))
    if rec_p.shape != (P, G, npol) or rec_p.dtype != torch.float64:
        raise RvzError(f"{who}: rec_p must be float64 [plies, n_games, {npol}]")
    _fits_int32(who, P * G, npol, "plies * n_games")
    if not 0 <= emit_from <= P:
        raise RvzError(f"{who}: emit_from = {emit_from} must be in [0, plies = {P}]")
    return P, G


def records_games(rec_black: torch.Tensor, rec_white: torch.Tensor, rec_side: torch.Tensor,
                  rec_idx: torch.Tensor, rec_p: torch.Tensor, board_size: int = 8,
                  emit_from: int = 0, state: bool = False):
    """rvz_records_games: a window of autoreset self-play records cut into finished games
    (include/rvz.h has the walk). rec_black / rec_white int64 [plies, n_games] (bit patterns),
    rec_side / rec_idx [plies, n_games] integers (rec_idx: the moves, negative where a ply holds
    no record), rec_p float64 [plies, n_games, S*S+1]: SelfPlayRunner's record tensors, a slot's
    games one after another down its column; device tensors. A game that ends at a ply >=
    emit_from is emitted: one row per record, slot-major, each with its value target from the
    game's winner by the engine's own rules. Returns a dict: "m" the number of rows, a 0-d int32
    device tensor (reading it is the caller's one host synchronisation); at length plies * n_games
    with the rows from m on unwritten "mover" / "opponent" int64, "policy" float32 [.., S*S+1],
    "value" float32 and "src" int32 (the record's ply * n_games + slot); "stats" int64 [8]:
    emitted rows, emitted games, open records, abandoned records, malformed records, headless
    emitted games, records an earlier window emitted, 0; and with state=True "state" int32
    [plies, n_games]: 1 emitted, 0 open, 2 ended before emit_from, 3 abandoned, -1 no record,
    -5 malformed. Asynchronous on the current stream; nothing synchronises. A window without
    records (plies or n_games 0) gives m = 0 without a launch."""
    P, G = check_records_args(rec_black, rec_white, rec_side, rec_idx, rec_p, board_size,
                              emit_from)
    npol = board_size * board_size + 1
    lib = _lib.load()
    dev = rec_black.device
    n = P * G
    b, w = rec_black.contiguous(), rec_white.to(dev).contiguous()
    sd, ix = _i32(rec_side, dev), _i32(rec_idx, dev)
    pol = rec_p.to(dev).contiguous()
    out = {"m": torch.zeros((), dtype=torch.int32, device=dev),
           "mover": torch.empty(n, dtype=torch.int64, device=dev),
           "opponent": torch.empty(n, dtype=torch.int64, device=dev),
           "policy": torch.empty(n, npol, dtype=torch.float32, device=dev),
           "value": torch.empty(n, dtype=torch.float32, device=dev),
           "src": torch.empty(n, dtype=torch.int32, device=dev),
           "stats": torch.zeros(8, dtype=torch.int64, device=dev)}
    if state:
        out["state"] = torch.empty(P, G, dtype=torch.int32, device=dev)
    if n:
        scratch = torch.empty(lib.rvz_records_scratch_size(P, G), dtype=torch.uint8, device=dev)
        check(lib.rvz_records_games(board_size, P, G, _addr(b), _addr(w), _addr(sd), _addr(ix),
                                    _addr(pol), int(emit_from), ptr(scratch), _addr(out["m"]),
                                    _addr(out["mover"]), _addr(out["opponent"]),
                                    _addr(out["policy"]), _addr(out["value"]), _addr(out["src"]),
                                    _addr(out.get("state")), _addr(out["stats"]),
                                    _lib.stream_handle(dev)), None, "rvz_records_games")
    return out


# ------------------------------------------------------------------ final-ownership targets
def check_final_args(rec_black, rec_white, rec_side, rec_idx, src, count, board_size,
                     who: str = "records_final"):
    """The argument rules of records_final, checked before any device call (the CPU tests' NumPy
    restatement calls it too); returns (plies, n_games, n)."""
    check_board_size(board_size, who)
    npol = board_size * board_size + 1
    if not all(isinstance(t, torch.Tensor) for t in (rec_black, rec_white, rec_side, rec_idx,
                                                     src)):
        raise RvzError(f"{who}: the four record arrays and src are tensors")
    if rec_idx.dim() != 2 or any(t.shape != rec_idx.shape for t in (rec_black, rec_white,
                                                                     rec_side)):
        raise RvzError(f"{who}: rec_black, rec_white, rec_side and rec_idx are [plies, n_games]")
    P, G = rec_idx.shape
    _bitboards(who, rec_black.reshape(-1), rec_white.reshape(-1), "rec_black and rec_white",
               "record")
    _given(who, P * G, "record", optional=False, rec_side=rec_side.reshape(-1),
           rec_idx=rec_idx.reshape(-1))
    if P < 1 or G < 1:
        raise RvzError(f"{who}: the window holds at least one ply and one slot")
    _fits_int32(who, P * G, npol, "plies * n_games")
    if src.dim() != 1:
        raise RvzError(f"{who}: src holds one integer per row")
    _given(who, src.numel(), "row", optional=False, src=src)
    if src.numel() >= 2 ** 31:
        raise RvzError(f"{who}: n must be below 2^31")
    if count is not None and (not isinstance(count, torch.Tensor) or count.numel() != 1 or
                              count.dtype != torch.int32):
        raise RvzError(f"{who}: count is None or one int32 tensor (records_games' m)")
    return P, G, src.numel()


def records_final(rec_black: torch.Tensor, rec_white: torch.Tensor, rec_side: torch.Tensor,
                  rec_idx: torch.Tensor, src: torch.Tensor, count: Optional[torch.Tensor] = None,
                  board_size: int = 8):
    """rvz_records_final: the final position of the game each of n records belongs to, from the
    record's mover's side (include/rvz.h has the walk): the ownership target of a training row.
    rec_black / rec_white int64 [plies, n_games] (bit patterns), rec_side / rec_idx
    [plies, n_games] integers: records_games' window; src [n] integers, each ply * n_games + slot
    (records_games' "src"); count None or one int32 device tensor (records_games' "m"): only the
    rows below min(n, count) are handled, read on the device. Returns a dict: "final_mover" /
    "final_opponent" int64 [n] and "ok" int32 [n] (zeros beyond the bound; ok = 0 and two empty
    boards for a row whose game does not end inside the window, or whose walk meets a malformed
    record, a refused move or a broken chain), "stats" int64 [4]: rows handled, rows with ok = 1,
    rows whose game is still open at the window's end, every other row. Asynchronous on the
    current stream; nothing synchronises. n = 0 launches nothing."""
    P, G, n = check_final_args(rec_black, rec_white, rec_side, rec_idx, src, count, board_size)
    lib = _lib.load()
    dev = rec_black.device
    b, w = rec_black.contiguous(), rec_white.to(dev).contiguous()
    sd, ix, sr = _i32(rec_side, dev), _i32(rec_idx, dev), _i32(src, dev)
    ct = None if count is None else count.to(dev).reshape(1).contiguous()
    out = {"final_mover": torch.zeros(n, dtype=torch.int64, device=dev),
           "final_opponent": torch.zeros(n, dtype=torch.int64, device=dev),
           "ok": torch.zeros(n, dtype=torch.int32, device=dev),
           "stats": torch.zeros(4, dtype=torch.int64, device=dev)}
    if n:
        check(lib.rvz_records_final(board_size, P, G, _addr(b), _addr(w), _addr(sd), _addr(ix), n,
                                    _addr(sr), _addr(ct), _addr(out["final_mover"]),
                                    _addr(out["final_opponent"]), _addr(out["ok"]),
                                    _addr(out["stats"]), _lib.stream_handle(dev)), None,
              "rvz_records_final")
    return out


def check_ownership_args(final_mover, final_opponent, slot, sym, board_size,
                         who: str = "replay_ownership") -> int:
    """The argument rules of replay_ownership, checked before any device call; returns nb."""
    check_board_size(board_size, who)
    if not all(isinstance(t, torch.Tensor) for t in (final_mover, final_opponent, slot, sym)):
        raise RvzError(f"{who}: final_mover, final_opponent, slot and sym are tensors")
    cap = _bitboards(who, final_mover, final_opponent, "final_mover and final_opponent", "slot")
    if not 1 <= cap < 2 ** 31:
        raise RvzError(f"{who}: the ring holds between 1 and 2^31 - 1 slots")
    if slot.dim() != 1:
        raise RvzError(f"{who}: slot holds one integer per output row")
    nb = slot.numel()
    _given(who, nb, "output row", optional=False, slot=slot, sym=sym)
    _fits_int32(who, nb, board_size * board_size + 1, "nb")
    return nb


def replay_ownership(final_mover: torch.Tensor, final_opponent: torch.Tensor, slot: torch.Tensor,
                     sym: torch.Tensor, board_size: int = 8):
    """rvz_replay_ownership: the ownership targets of a drawn batch (include/rvz.h has the
    definition). final_mover / final_opponent int64 [capacity] (bit patterns): the ring's final
    positions; slot / sym [nb] integers: replay_batch's fourth and fifth outputs; device tensors.
    Returns (ownership float32 [nb, S*S]: +1 where the row's mover holds the square at the end of
    its game, -1 where the opponent does, 0 where it stays empty, under the row's own symmetry;
    margin float32 [nb]: the final disc margin, the sum of the row). A row with a slot outside
    [0, capacity), a sym outside [0, 8) or bitboards that overlap or leave the board is all
    zero. Asynchronous on the current stream; nothing synchronises."""
    nb = check_ownership_args(final_mover, final_opponent, slot, sym, board_size)
    lib = _lib.load()
    dev = final_mover.device
    fm, fo = final_mover.contiguous(), final_opponent.to(dev).contiguous()
    sl, sy = _i32(slot, dev), _i32(sym, dev)
    own = torch.empty(nb, board_size * board_size, dtype=torch.float32, device=dev)
    margin = torch.empty(nb, dtype=torch.float32, device=dev)
    if nb:
        check(lib.rvz_replay_ownership(board_size, fm.numel(), _addr(fm), _addr(fo), nb, _addr(sl),
                                       _addr(sy), _addr(own), _addr(margin),
                                       _lib.stream_handle(dev)), None, "rvz_replay_ownership")
    return own, margin


# ------------------------------------------------------------------ opening pools
# The default max_rows of openings(): the bound is the largest level's candidate count, which
# grows with the level, so ply 8's. By the level rule on the CPU oracle (tests/openings_ref.py)
# level 8 has 303,386 candidates on 8x8 and 266,062 on 6x6 (270,319 and 235,673 distinct rows);
# 2^19 = 524,288 holds both (a scratch of 32 MB). Level 9 has 1,703,146 on 6x6: deeper calls pass
# their own max_rows.
OPENINGS_DEFAULT_MAX_ROWS = 1 << 19


def check_openings_args(board_size, plies, max_rows, who: str = "openings") -> int:
    """The argument rules of openings, checked before any device call; returns max_rows."""
    check_board_size(board_size, who)
    _ints(who, plies=plies)
    if not 0 <= plies <= board_size * board_size - 4:
        raise RvzError(f"{who}: plies = {plies} must be in [0, S*S - 4]")
    if max_rows is None:
        if plies > 8:
            raise RvzError(f"{who}: the default max_rows holds plies <= 8; pass max_rows")
        return OPENINGS_DEFAULT_MAX_ROWS
    _ints(who, max_rows=max_rows)
    if not 1 <= max_rows < 2 ** 29:
        raise RvzError(f"{who}: max_rows = {max_rows} must be >= 1 and max_rows * 4 fit int32")
    return int(max_rows)


def openings(board_size: int, plies: int, max_rows: Optional[int] = None, device="cuda"):
    """rvz_openings: the distinct positions after `plies` plies from the start position under the
    engine's own rules (include/rvz.h has the level rule), in order of first occurrence. Returns
    a dict: "black" / "white" int64 [m] (bit patterns), "status" int32 [m, 4], each row
    {side, 0, -1, 0} (what Engine.set_state and Engine.openings take), "stats" int64 [8]: rows, the
    last level's candidates before de-duplication, finished children dropped, duplicates removed,
    the largest level's candidates, 0, 0, 0. max_rows: the rows the scratch holds per level
    (default OPENINGS_DEFAULT_MAX_ROWS = 2^19, enough for plies <= 8 on either board; deeper
    calls pass their own); a level with more candidates raises RvzError, and the result does not
    depend on max_rows otherwise. Reading the row count is the call's one synchronisation."""
    who = "openings"
    R = check_openings_args(board_size, plies, max_rows, who)
    lib = _lib.load()
    dev = torch.device(device)
    m = torch.zeros((), dtype=torch.int32, device=dev)
    b, w = (torch.empty(R, dtype=torch.int64, device=dev) for _ in range(2))
    st = torch.empty(R, 4, dtype=torch.int32, device=dev)
    stats = torch.zeros(8, dtype=torch.int64, device=dev)
    scratch = torch.empty(lib.rvz_openings_scratch_size(board_size, R), dtype=torch.uint8,
                          device=dev)
    check(lib.rvz_openings(board_size, int(plies), R, ptr(scratch), _addr(m), _addr(b), _addr(w),
                           _addr(st), _addr(stats), _lib.stream_handle(dev)), None, "rvz_openings")
    n = int(m.item())
    if n < 0:
        raise RvzError(f"{who}: a level has {int(stats[4].item())} candidates, more than "
                       f"max_rows = {R}")
    return {"black": b[:n].clone(), "white": w[:n].clone(), "status": st[:n].clone(),
            "stats": stats}


def opening_index(n_pool: int, seed32: torch.Tensor, salt: int = 0) -> torch.Tensor:
    """rvz_opening_index: the pool row a game reset with each seed starts from, with a pool of
    n_pool rows set by Engine.openings(..., salt=salt) (the same device function). seed32 [n]
    integers (taken mod 2^32), a device tensor. Returns int32 [n]."""
    who = "opening_index"
    _ints(who, n_pool=n_pool, salt=salt)
    if not 1 <= n_pool < 2 ** 31:
        raise RvzError(f"{who}: n_pool must be in [1, 2^31)")
    if not isinstance(seed32, torch.Tensor) or seed32.dim() != 1 or \
            seed32.dtype.is_floating_point or seed32.dtype == torch.bool:
        raise RvzError(f"{who}: seed32 holds one integer per game")
    lib = _lib.load()
    dev = seed32.device
    n = seed32.numel()
    # the low 32 bits as an int32 bit pattern, as Engine.reset passes its seeds
    s64 = seed32.to(torch.int64).bitwise_and(0xFFFFFFFF)
    sd = torch.where(s64 >= 2 ** 31, s64 - 2 ** 32, s64).to(torch.int32).contiguous()
    out = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        check(lib.rvz_opening_index(int(n_pool), n, _addr(sd), int(salt) & 0xFFFFFFFF, _addr(out),
                                    _lib.stream_handle(dev)), None, "rvz_opening_index")
    return out


def opening_suite(board_size: int, plies: int, depth: Optional[int] = None,
                  max_abs_score: Optional[int] = None, max_rows: Optional[int] = None,
                  device="cuda"):
    """The opening suite of an engine match: openings(board_size, plies), and with depth set only
    the balanced ones: the rows whose rvz.alphabeta score at that depth (default weights, from
    the mover's side) has absolute value at most max_abs_score. There is no default threshold:
    depth and max_abs_score are given together. Returns (black, white, side): int64 [m], int64
    [m], int32 [m], in openings' order."""
    who = "opening_suite"
    if (depth is None) != (max_abs_score is None):
        raise RvzError(f"{who}: depth and max_abs_score are given together (there is no default "
                       "threshold)")
    o = openings(board_size, plies, max_rows, device)
    b, w, st = o["black"], o["white"], o["status"]
    if depth is not None:
        _ints(who, depth=depth, max_abs_score=max_abs_score)
        if max_abs_score < 0:
            raise RvzError(f"{who}: max_abs_score must be >= 0")
        from .engine import alphabeta
        if b.numel():
            score, _, _ = alphabeta(b, w, st, board_size, int(depth))
            keep = score.to(torch.int64).abs() <= int(max_abs_score)
            b, w, st = b[keep], w[keep], st[keep]
    return b, w, st[:, 0].contiguous()


# ------------------------------------------------------------------ prioritized replay
PRIORITY_MIN_FLOOR, PRIORITY_MAX_CAP = 2.0 ** -16, 65536.0


def _number(who: str, name: str, x, lo: float, hi: float, closed_hi: bool = True) -> float:
    """A real number (not a bool) in [lo, hi] (or [lo, hi)); NaN fails."""
    if not is_number(x, lo, hi, hi_open=not closed_hi):
        raise RvzError(f"{who}: {name} must be a number in [{lo}, {hi}{']' if closed_hi else ')'}"
                       f", not {x!r}")
    return float(x)


def check_is_weight_args(prob, slot, beta, who: str = "replay_is_weight") -> int:
    """The argument rules of replay_is_weight, checked before any device call (the CPU tests'
    NumPy restatement calls it too); returns nb."""
    if not isinstance(prob, torch.Tensor) or prob.dim() != 1 or prob.dtype != torch.float32:
        raise RvzError(f"{who}: prob must be float32 [nb]")
    nb = prob.numel()
    if not isinstance(slot, torch.Tensor):
        raise RvzError(f"{who}: slot holds one integer per drawn row")
    _given(who, nb, "drawn row", optional=False, slot=slot)
    _number(who, "beta", beta, 0.0, 1.0)
    return nb


def check_priority_args(weight, slot, rows, policy_coef=1.0, value_coef=1.0,
                        subtract_entropy=True, alpha=0.6, floor=2.0 ** -8, cap=2.0 ** 8,
                        max_priority=None, who: str = "replay_priority") -> int:
    """The argument rules of replay_priority, checked before any device call (the CPU tests'
    NumPy restatement calls it too); returns nb."""
    if not isinstance(weight, torch.Tensor) or weight.dim() != 1 or \
            weight.dtype != torch.float32 or not weight.is_contiguous() or \
            not 1 <= weight.numel() < 2 ** 31:
        raise RvzError(f"{who}: weight must be a contiguous float32 [capacity] (it is written in "
                       "place), 1 <= capacity < 2^31")
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.shape[1] != 3 or \
            rows.dtype != torch.float64:
        raise RvzError(f"{who}: rows must be float64 [nb, 3], the loss's per-row "
                       "{Lp, Lv, H}")
    nb = rows.shape[0]
    if nb > 2 ** 30:
        raise RvzError(f"{who}: nb must be at most 2^30")
    if not isinstance(slot, torch.Tensor):
        raise RvzError(f"{who}: slot holds one integer per row of rows")
    _given(who, nb, "row of rows", optional=False, slot=slot)
    for name, x in (("policy_coef", policy_coef), ("value_coef", value_coef)):
        _number(who, name, x, 0.0, float("inf"), closed_hi=False)
    if not isinstance(subtract_entropy, numbers.Integral):      # a bool is one
        raise RvzError(f"{who}: subtract_entropy is a bool, not {subtract_entropy!r}")
    _number(who, "alpha", alpha, 0.0, 1.0)
    lo = _number(who, "floor", floor, PRIORITY_MIN_FLOOR, PRIORITY_MAX_CAP)
    hi = _number(who, "cap", cap, PRIORITY_MIN_FLOOR, PRIORITY_MAX_CAP)
    if lo > hi:
        raise RvzError(f"{who}: floor = {floor!r} must not exceed cap = {cap!r}")
    if max_priority is not None and (not isinstance(max_priority, torch.Tensor) or
                                     max_priority.numel() != 1 or
                                     max_priority.dtype != torch.float32 or
                                     max_priority.device != weight.device):
        raise RvzError(f"{who}: max_priority is None or one float32 on the weights' device (it "
                       "is updated in place)")
    return nb


def replay_is_weight(prob: torch.Tensor, slot: torch.Tensor, beta: float,
                     with_min: bool = False):
    """rvz_replay_is_weight: the importance-sampling weights of a drawn batch (include/rvz.h has
    the definition). prob float32 [nb] and slot [nb] integers: replay_batch_weighted's prob and
    slot, device tensors; beta in [0, 1]. Returns weight float32 [nb]: (pmin / prob[r]) ** beta in
    float64 with the correctly rounded power, pmin the smallest probability among the valid rows
    (slot >= 0, prob finite and > 0), so every weight is in (0, 1] and the rarest row weighs 1;
    0 for any other row. with_min=True: (weight, min_prob), min_prob float32 [1] holding pmin (0
    with no valid row). Asynchronous on the current stream; nothing synchronises."""
    nb = check_is_weight_args(prob, slot, beta)
    lib = _lib.load()
    dev = prob.device
    pr, sl = prob.contiguous(), _i32(slot, dev)
    out = torch.empty(nb, dtype=torch.float32, device=dev)
    pmin = torch.zeros(1, dtype=torch.float32, device=dev)
    if nb:
        scratch = torch.empty(lib.rvz_replay_is_weight_scratch_size(nb), dtype=torch.uint8,
                              device=dev)
        check(lib.rvz_replay_is_weight(nb, _addr(pr), _addr(sl), float(beta), ptr(scratch),
                                       _addr(out), _addr(pmin), _lib.stream_handle(dev)), None,
              "rvz_replay_is_weight")
    return (out, pmin) if with_min else out


def replay_priority(weight: torch.Tensor, slot: torch.Tensor, rows: torch.Tensor,
                    policy_coef: float = 1.0, value_coef: float = 1.0,
                    subtract_entropy: bool = True, alpha: float = 0.6, floor: float = 2.0 ** -8,
                    cap: float = 2.0 ** 8, max_priority: Optional[torch.Tensor] = None):
    """rvz_replay_priority: a batch's loss rows written into the ring's sampling weights
    (include/rvz.h has the definition). weight float32 [capacity], contiguous, written in place;
    slot [nb] integers, the batch's slots (replay_batch_weighted's); rows float64 [nb, 3],
    policy_value_loss's "rows" {Lp, Lv, H}; device tensors. A valid row's priority is
    min(cap, max(floor, (policy_coef * k + value_coef * Lv) ** alpha)) as float32, k = max(Lp - H,
    0) with subtract_entropy (the policy's KL divergence from its target) or Lp without; where
    several valid rows name one slot the last one's priority is written, and a slot no valid row
    names keeps its bytes. max_priority: None, or one float32 on the device, raised in place to
    the largest priority of the valid rows. Returns (priority float32 [nb], 0 for an invalid row;
    state int32 [nb]: 1 written, 0 superseded by a later row, -1 invalid). No append may have
    overwritten the batch's slots since the draw. The table of prefix sums is not updated: rebuild
    it (replay_cdf) before the next draw. Asynchronous on the current stream; nothing
    synchronises."""
    nb = check_priority_args(weight, slot, rows, policy_coef, value_coef, subtract_entropy, alpha,
                             floor, cap, max_priority)
    lib = _lib.load()
    dev = weight.device
    sl, rw = _i32(slot, dev), rows.to(dev).contiguous()
    pri = torch.zeros(nb, dtype=torch.float32, device=dev)
    state = torch.full((nb,), -1, dtype=torch.int32, device=dev)
    if nb:
        scratch = torch.empty(lib.rvz_replay_priority_scratch_size(nb), dtype=torch.uint8,
                              device=dev)
        check(lib.rvz_replay_priority(weight.numel(), _addr(weight), nb, _addr(sl), _addr(rw),
                                      float(policy_coef), float(value_coef),
                                      int(bool(subtract_entropy)), float(alpha), float(floor),
                                      float(cap), ptr(scratch), _addr(max_priority), _addr(pri),
                                      _addr(state), _lib.stream_handle(dev)), None,
              "rvz_replay_priority")
    return pri, state


# ------------------------------------------------------------------ replay reanalysis
STALE_MAX_CLASSES = 65536


def check_stale_args(stamp, start, live, n, lo, below, who: str = "replay_stale") -> int:
    """The argument rules of replay_stale, checked before any device call (the CPU tests' NumPy
    restatement calls it too); returns the capacity."""
    if not isinstance(stamp, torch.Tensor) or stamp.dim() != 1 or stamp.dtype != torch.int32 or \
            not stamp.is_contiguous():
        raise RvzError(f"{who}: stamp must be a contiguous int32 [capacity]")
    _ints(who, start=start, live=live, n=n, lo=lo, below=below)
    cap = stamp.numel()
    _ring(who, cap, start, live, 1)
    if not 0 <= n < 2 ** 31:
        raise RvzError(f"{who}: n = {n} must be in [0, 2^31)")
    if not (0 <= lo < below < 2 ** 31 and below - lo <= STALE_MAX_CLASSES):
        raise RvzError(f"{who}: (lo, below) = ({lo}, {below}) must have 0 <= lo < below and "
                       f"below - lo <= {STALE_MAX_CLASSES}")
    return cap


def check_roots_args(mover, opponent, slot, board_size, who: str = "replay_roots") -> int:
    """The argument rules of replay_roots, checked before any device call; returns n."""
    check_board_size(board_size, who)
    if not all(isinstance(t, torch.Tensor) for t in (mover, opponent, slot)):
        raise RvzError(f"{who}: mover, opponent and slot are tensors")
    cap = _bitboards(who, mover, opponent, "mover and opponent", "slot")
    if not 1 <= cap < 2 ** 31:
        raise RvzError(f"{who}: the ring holds between 1 and 2^31 - 1 slots")
    if slot.dim() != 1:
        raise RvzError(f"{who}: slot holds one integer per row")
    _given(who, slot.numel(), "row", optional=False, slot=slot)
    return slot.numel()


def check_refresh_args(policy, stamp, slot, p, idx, new_stamp, who: str = "replay_refresh"):
    """The argument rules of replay_refresh, checked before any device call (the CPU tests'
    NumPy restatement calls it too); returns (board_size, n)."""
    if not isinstance(policy, torch.Tensor) or policy.dim() != 2 or \
            policy.dtype != torch.float32 or not policy.is_contiguous() or \
            policy.shape[1] not in (65, 37) or not 1 <= policy.shape[0] < 2 ** 31:
        raise RvzError(f"{who}: policy must be a contiguous float32 [capacity, S*S+1] (it is "
                       "written in place), S 8 or 6")
    cap, npol = policy.shape
    if not isinstance(stamp, torch.Tensor) or stamp.shape != (cap,) or \
            stamp.dtype != torch.int32 or not stamp.is_contiguous() or \
            stamp.device != policy.device:
        raise RvzError(f"{who}: stamp must be a contiguous int32 [capacity] on the policy's device "
                       "(it is written in place)")
    if not isinstance(p, torch.Tensor) or p.dim() != 2 or p.shape[1] != npol or \
            p.dtype != torch.float64:
        raise RvzError(f"{who}: p must be float64 [n, {npol}], the act's probability rows")
    n = p.shape[0]
    if n > 2 ** 30:
        raise RvzError(f"{who}: n must be at most 2^30")
    if not isinstance(slot, torch.Tensor) or not isinstance(idx, torch.Tensor):
        raise RvzError(f"{who}: slot and idx hold one integer per row of p")
    _given(who, n, "row of p", optional=False, slot=slot, idx=idx)
    _ints(who, new_stamp=new_stamp)
    if not 0 <= new_stamp < 2 ** 31:
        raise RvzError(f"{who}: new_stamp = {new_stamp} must be in [0, 2^31)")
    return (8 if npol == 65 else 6), n


def replay_stale(stamp: torch.Tensor, start: int, live: int, n: int, lo: int, below: int):
    """rvz_replay_stale: the stalest rows of a ring, chosen on the device (include/rvz.h has the
    rule). stamp int32 [capacity], contiguous, a device tensor: the iteration whose net produced
    each slot's policy; the ring's `live` rows start at slot `start`, oldest first, and wrap. A
    live row is eligible iff 0 <= stamp < below, its age class is max(stamp - lo, 0), and the
    min(n, eligible) rows of the smallest classes are selected, ties in the last class going to
    the older row. 0 <= lo < below, below - lo <= 65536. Returns (slot int32 [n]: the selected
    slots in logical-row order, oldest first, then -1; count int32 [2]: the rows selected and the
    live rows whose stamp is negative, which are never selected). Asynchronous on the current
    stream; nothing synchronises. n = 0 launches nothing."""
    cap = check_stale_args(stamp, start, live, n, lo, below)
    lib = _lib.load()
    dev = stamp.device
    out = torch.empty(int(n), dtype=torch.int32, device=dev)
    count = torch.zeros(2, dtype=torch.int32, device=dev)
    if n:
        size = lib.rvz_replay_stale_scratch_size(cap, int(below) - int(lo))
        scratch = torch.empty(size, dtype=torch.uint8, device=dev)
        check(lib.rvz_replay_stale(cap, _addr(stamp), int(start), int(live), int(n), int(lo),
                                   int(below), ptr(scratch), size, _addr(out), _addr(count),
                                   _lib.stream_handle(dev)), None, "rvz_replay_stale")
    return out, count


def replay_roots(mover: torch.Tensor, opponent: torch.Tensor, slot: torch.Tensor,
                 board_size: int = 8):
    """rvz_replay_roots: ring rows as the arrays Engine.set_state takes. mover / opponent int64
    [capacity] (bit patterns), slot [n] integers (replay_stale's), device tensors. Returns (black
    int64 [n], white int64 [n], status int32 [n, 4], bad int32 [1]): for a slot in [0, capacity)
    the mover as black, the opponent as white and {1, 0, -1, 0}, a live game with black to move;
    for -1 empty boards and {1, 1, 0, 0}, a game that is over, which the engine does not search;
    for any other slot, or a row whose bitboards overlap or leave the board, the same finished
    row and one count in bad. Asynchronous on the current stream; nothing synchronises."""
    n = check_roots_args(mover, opponent, slot, board_size)
    lib = _lib.load()
    dev = mover.device
    mv, op = mover.contiguous(), opponent.to(dev).contiguous()
    sl = _i32(slot, dev)
    b = torch.empty(n, dtype=torch.int64, device=dev)
    w = torch.empty(n, dtype=torch.int64, device=dev)
    st = torch.empty(n, 4, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    if n:
        check(lib.rvz_replay_roots(board_size, mv.numel(), _addr(mv), _addr(op), n, _addr(sl),
                                   _addr(b), _addr(w), ptr(st), _addr(bad),
                                   _lib.stream_handle(dev)), None, "rvz_replay_roots")
    return b, w, st, bad


def replay_refresh(policy: torch.Tensor, stamp: torch.Tensor, slot: torch.Tensor,
                   p: torch.Tensor, idx: torch.Tensor, new_stamp: int) -> torch.Tensor:
    """rvz_replay_refresh: the act's rows written over a ring's policy targets (include/rvz.h has
    the definition). policy float32 [capacity, S*S+1] and stamp int32 [capacity], contiguous,
    written in place; slot [n] integers (what replay_roots took), p float64 [n, S*S+1] and idx [n]
    integers: Engine.act(1.0, apply=False)'s rows and indices; device tensors. A row is skipped,
    and its slot keeps its bytes, if its slot is outside [0, capacity) (the -1 padding), its idx is
    -2 (the engine treated the game as over), it holds a negative or non-finite entry or its sum
    is off 1 by more than 1e-9; any other row becomes policy[slot] = p.float() and stamp[slot] =
    new_stamp, the last such row where several name one slot. Returns counts int32 [2]: the slots
    written and the rows skipped. The ring's value, mover and opponent are no arguments.
    Asynchronous on the current stream; nothing synchronises."""
    board_size, n = check_refresh_args(policy, stamp, slot, p, idx, new_stamp)
    lib = _lib.load()
    dev = policy.device
    sl, ix, pp = _i32(slot, dev), _i32(idx, dev), p.to(dev).contiguous()
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    if n:
        size = lib.rvz_replay_refresh_scratch_size(n)
        scratch = torch.empty(size, dtype=torch.uint8, device=dev)
        check(lib.rvz_replay_refresh(board_size, policy.shape[0], _addr(policy), _addr(stamp), n,
                                     _addr(sl), _addr(pp), _addr(ix), int(new_stamp),
                                     ptr(scratch), size, _addr(counts),
                                     _lib.stream_handle(dev)), None, "rvz_replay_refresh")
    return counts
