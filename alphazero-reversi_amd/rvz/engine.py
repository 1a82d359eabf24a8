"""Host mirror of the rvz engine: owns one C-ABI engine (include/rvz.h) and its device buffers.

One ``Engine`` = ``n_games`` Reversi games resident in HBM, each with its own MCTS tree.
It is what the reference's per-game ``ReversiGame`` + ``MCTS`` pair becomes when all games of a
self-play batch are advanced in lockstep (self_play.py:80-101, mcts.py:322-694):

    eng.reset(seeds)                      # ReversiGame() x n + np.random.seed per game
    eng.search(evaluator)                 # MCTS.search for every live game
    idx, p = eng.act(temperature)         # get_action_probs tail + game.make_move

Every tensor handed to the library is a device tensor on ``eng.device``; all work is enqueued on
the current torch stream of that device (graph-capturable: no host syncs inside ``search``/``act``).

The stateless wrappers of training records (symmetries, merging, replay) are in ``rvz.records``.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import (RVZ_DONE, RVZ_LEAF_BF16, RVZ_LEAF_F32, RvzError, check, check_board_size,
                   ptr)

U64 = 0xFFFFFFFFFFFFFFFF
SOLVE_MAX_EMPTIES = _lib.RVZ_SOLVE_MAX_EMPTIES
SOLVE_NOT_A_MOVE = _lib.RVZ_SOLVE_NOT_A_MOVE      # solve_moves: not a legal move of the row
SOLVE_ABANDONED = _lib.RVZ_SOLVE_ABANDONED        # solve_moves: the move's search hit node_limit
AB_MAX_DEPTH = _lib.RVZ_AB_MAX_DEPTH              # alphabeta: the deepest search
AB_WIN = _lib.RVZ_AB_WIN                          # alphabeta: |score| of a finished game, at least
AB_HEUR_MAX = _lib.RVZ_AB_HEUR_MAX                # alphabeta: the bound on a weight table


def to_signed64(x: int) -> int:
    x &= U64
    return x - (1 << 64) if x >> 63 else x


def to_unsigned64(x: int) -> int:
    return int(x) & U64


class Engine:
    def __init__(self, n_games: int, num_simulations: int = 800, batch_size: int = 64,
                 c_puct: float = 1.0, board_size: int = 8, device=None,
                 leaf_dtype: torch.dtype = torch.float32, compact_leaves: bool = False,
                 memo: bool = False):
        if not torch.cuda.is_available():
            raise RvzError("rvz needs a HIP device (MI355X); there is no CPU fallback")
        self.lib = _lib.load()
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_games, self.board_size = int(n_games), int(board_size)
        self.num_simulations, self.batch_size = int(num_simulations), int(batch_size)
        self.c_puct = float(c_puct)
        self.nsq = board_size * board_size
        self.npol = self.nsq + 1
        if leaf_dtype not in (torch.float32, torch.bfloat16):
            raise RvzError("leaf_dtype must be torch.float32 or torch.bfloat16")
        self.leaf_dtype = leaf_dtype
        cfg = _lib.Config(board_size, n_games, num_simulations, batch_size, c_puct,
                          self.device.index,
                          RVZ_LEAF_F32 if leaf_dtype == torch.float32 else RVZ_LEAF_BF16)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rvz_create(C.byref(cfg), C.byref(h)), None, "rvz_create")
        self._h = h
        G, dev = self.n_games, self.device
        self.leaf_x = torch.zeros(G, 3, board_size, board_size, dtype=leaf_dtype, device=dev)
        self.need = torch.zeros(G, dtype=torch.int32, device=dev)
        self.visits_buf = torch.zeros(G, self.npol, dtype=torch.int32, device=dev)
        self.p_buf = torch.zeros(G, self.npol, dtype=torch.float64, device=dev)
        self.idx_buf = torch.zeros(G, dtype=torch.int32, device=dev)
        self.black = torch.zeros(G, dtype=torch.int64, device=dev)
        self.white = torch.zeros(G, dtype=torch.int64, device=dev)
        self.status = torch.zeros(G, 4, dtype=torch.int32, device=dev)
        self.n_batches = -(-num_simulations // batch_size)
        self.compact_leaves = False
        if compact_leaves:
            self.compact(True)
        self.memo_on = False
        if memo:
            self.memo(True)

    # ------------------------------------------------------------------ plumbing
    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                torch.cuda.synchronize(self.device)
            except Exception:  # pragma: no cover - interpreter shutdown
                pass
            self.lib.rvz_destroy(h)
            self._h = None

    def _stream(self):
        s = _lib.stream_handle(self.device)
        check(self.lib.rvz_set_stream(self._h, s), self._h, "rvz_set_stream")

    def _call(self, name: str, *args) -> int:
        return check(getattr(self.lib, name)(self._h, *args), self._h, name)

    def check(self) -> None:
        """Synchronise and raise RvzError if a kernel set the device error word (node pool, path
        depth, RNG stream, non-finite NN output) or an evaluator this engine's searches used
        reports an activation overflow (LeafEvaluator.overflowed: h2's sticky device word).
        Both are accumulated on the device and read only here, so graph replays stay sync-free."""
        self._stream()
        err = C.c_int32(0)
        self._call("rvz_check", C.byref(err))
        for ev in getattr(self, "_evaluators", ()):
            of = getattr(ev, "overflowed", None)
            if of is not None and of():
                raise RvzError(f"leaf evaluator ({getattr(ev, 'kernel', type(ev).__name__)}) "
                               "overflowed its f16 activation range (|x| >= 65520) even in the "
                               "ranged re-run: the NN outputs of the searches are not valid")

    def counters(self) -> Tuple[int, int]:
        out = (C.c_int64 * 2)()
        self.lib.rvz_counters(self._h, out)
        return int(out[0]), int(out[1])

    def footprint(self) -> Tuple[int, int]:
        a, b = C.c_int64(), C.c_int64()
        self.lib.rvz_footprint(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def stats_enable(self, on: bool = True):
        self._stream()
        self._call("rvz_stats_enable", int(bool(on)))

    def stats_read(self):
        """Algorithmic bytes moved since stats_enable: (select, expand_backup, act)."""
        self._stream()
        out = (C.c_int64 * 3)()
        self._call("rvz_stats_read", out)
        return int(out[0]), int(out[1]), int(out[2])

    def timing_enable(self, on: bool = True):
        self._call("rvz_timing_enable", int(bool(on)))

    def timing_read(self):
        """Mean ms per launch and launch counts of k_step / k_act since timing_enable."""
        self._stream()
        ms, n = (C.c_double * 2)(), (C.c_int32 * 2)()
        self._call("rvz_timing_read", ms, n)
        return {"step": (ms[0], n[0]), "act": (ms[1], n[1])}

    def tree(self):
        """(nodes int32[G, M, 4] = {N, W, P, C} (W/P/C as float32 bits), meta uint32-as-int32[G, M])."""
        self._stream()
        M = self.lib.rvz_tree_nodes(self._h)
        nodes = torch.empty(self.n_games, M, 4, dtype=torch.int32, device=self.device)
        meta = torch.empty(self.n_games, M, dtype=torch.int32, device=self.device)
        self._call("rvz_tree_export", ptr(nodes), ptr(meta))
        return nodes, meta

    # ------------------------------------------------------------------ env
    def reset(self, seeds: Optional[Sequence[int]] = None, mask: Optional[torch.Tensor] = None):
        """ReversiGame() for every (masked) game + np.random.seed(seeds[g]) per game."""
        self._stream()
        if seeds is None:
            seeds = range(self.n_games)
        if not isinstance(seeds, torch.Tensor):
            seeds = torch.tensor([int(s) & 0xFFFFFFFF for s in seeds], dtype=torch.int64)
        s = seeds.to(self.device).to(torch.int64).bitwise_and(0xFFFFFFFF).to(torch.int32)
        if s.numel() != self.n_games:
            raise RvzError("one seed per game")
        m = None if mask is None else mask.to(self.device, torch.uint8).contiguous()
        self._seeds = s.contiguous()
        self._call("rvz_env_reset", ptr(self._seeds), ptr(m) if m is not None else None)

    def reset_device(self, seeds_i32: torch.Tensor, mask_u8: Optional[torch.Tensor] = None):
        """Graph-capturable reset: persistent int32 seeds / uint8 mask device tensors."""
        self._stream()
        self._call("rvz_env_reset", ptr(seeds_i32), ptr(mask_u8) if mask_u8 is not None else None)

    def autoreset(self, idx: torch.Tensor, seeds: torch.Tensor, stride: int,
                  plies: torch.Tensor, done: torch.Tensor, reset: bool = True):
        """rvz_env_autoreset: count committed plies per game; restart finished games with their
        slot's next seed (seeds int64 [G] advanced in place by stride). Graph-capturable."""
        for t, dt in ((idx, torch.int32), (seeds, torch.int64), (plies, torch.int64),
                      (done, torch.int64)):
            if t.dtype != dt or t.numel() != self.n_games or not t.is_contiguous():
                raise RvzError("autoreset: idx int32, seeds/plies/done int64, [n_games]")
        self._stream()
        self._call("rvz_env_autoreset", ptr(idx), ptr(seeds), int(stride), ptr(plies), ptr(done),
                   int(bool(reset)))

    def set_draws(self, u: torch.Tensor):
        """rvz_env_set_draws: game g's move-sampling draws become u[g] (float64 [G, RVZ_DRAWS],
        the values np.random.random_sample() would return), each game rewound to its first."""
        uu = u.to(self.device, torch.float64).contiguous()
        if uu.shape != (self.n_games, _lib.RVZ_DRAWS):
            raise RvzError(f"set_draws: u must be float64 [{self.n_games}, {_lib.RVZ_DRAWS}]")
        self._stream()
        self._call("rvz_env_set_draws", ptr(uu))
        self._draws_keep = uu          # the copy is stream-ordered: keep the source alive

    def draws(self) -> torch.Tensor:
        """rvz_env_draws: the draws each game consumed since its reset / set_draws (int32 [G])."""
        out = torch.empty(self.n_games, dtype=torch.int32, device=self.device)
        self._stream()
        self._call("rvz_env_draws", ptr(out))
        return out

    def get_state(self):
        """(black int64[G], white int64[G], status int32[G,4]) device tensors (bit patterns)."""
        self._stream()
        self._call("rvz_env_get", ptr(self.black), ptr(self.white), ptr(self.status))
        return self.black, self.white, self.status

    def set_state(self, black: torch.Tensor, white: torch.Tensor, status: torch.Tensor):
        self._stream()
        b = black.to(self.device, torch.int64).contiguous()
        w = white.to(self.device, torch.int64).contiguous()
        st = status.to(self.device, torch.int32).contiguous()
        self._call("rvz_env_set", ptr(b), ptr(w), ptr(st))
        torch.cuda.current_stream(self.device).synchronize()  # b, w, st are temporaries

    def _env_snapshot(self):
        """rvz_env_get into fresh tensors (black, white, status): get_state()'s buffers stay."""
        self._stream()
        b = torch.empty(self.n_games, dtype=torch.int64, device=self.device)
        w = torch.empty_like(b)
        st = torch.empty(self.n_games, 4, dtype=torch.int32, device=self.device)
        self._call("rvz_env_get", ptr(b), ptr(w), ptr(st))
        return b, w, st

    def solve(self, max_empties: int = SOLVE_MAX_EMPTIES, node_limit: int = 2 ** 24):
        """rvz.solve on the engine's current env state (rvz_env_get into fresh tensors, then
        rvz_solve): (score, move, nodes) per game. Reads only: the env, a running search and the
        buffers get_state() returns are left as they are."""
        b, w, st = self._env_snapshot()
        return solve(b, w, st, self.board_size, max_empties, node_limit)

    def solve_wld(self, max_empties: int = SOLVE_MAX_EMPTIES, node_limit: int = 2 ** 24,
                  order_min_empties: Optional[int] = None):
        """rvz.solve_wld on the engine's current env state, as solve(): (outcome, move, nodes) per
        game. order_min_empties None: solve_wld's default."""
        b, w, st = self._env_snapshot()
        if order_min_empties is None:
            order_min_empties = WLD_ORDER_MIN_EMPTIES
        return solve_wld(b, w, st, self.board_size, max_empties, node_limit, order_min_empties)

    def solve_moves(self, max_empties: int = SOLVE_MAX_EMPTIES, node_limit: int = 2 ** 24,
                    alpha: int = -64, beta: int = 64, order_min_empties: int = 0):
        """rvz.solve_moves on the engine's current env state, as solve(): (scores, count, nodes)
        per game, one entry per move."""
        b, w, st = self._env_snapshot()
        return solve_moves(b, w, st, self.board_size, max_empties, node_limit, alpha, beta,
                           order_min_empties)

    def solve_moves_wld(self, max_empties: int = SOLVE_MAX_EMPTIES, node_limit: int = 2 ** 24,
                        order_min_empties: Optional[int] = None):
        """rvz.solve_moves_wld on the engine's current env state, as solve_wld()."""
        b, w, st = self._env_snapshot()
        if order_min_empties is None:
            order_min_empties = WLD_ORDER_MIN_EMPTIES
        return solve_moves_wld(b, w, st, self.board_size, max_empties, node_limit,
                               order_min_empties)

    def alphabeta(self, depth: int = 4, weights: Optional[Sequence[int]] = None,
                  node_limit: int = 2 ** 24):
        """rvz.alphabeta on the engine's current env state, as solve(): (score, move, nodes) per
        game. Reads only."""
        b, w, st = self._env_snapshot()
        return alphabeta(b, w, st, self.board_size, depth, weights, node_limit)

    def legal(self) -> torch.Tensor:
        self._stream()
        out = torch.empty(self.n_games, dtype=torch.int64, device=self.device)
        self._call("rvz_env_legal", ptr(out))
        return out

    def apply(self, sq: torch.Tensor) -> torch.Tensor:
        self._stream()
        s = sq.to(self.device, torch.int32).contiguous()
        ok = torch.empty(self.n_games, dtype=torch.int32, device=self.device)
        self._call("rvz_env_apply", ptr(s), ptr(ok))
        return ok

    # ------------------------------------------------------------------ fused self-play
    def play_buffers(self, evaluator=None):
        """Allocate what play() needs (the row counter, the launch scratch, the evaluator's
        overflow word) outside any graph capture: allocated inside one, their zero-fill would be
        recorded into the graph and every replay would reset the counter."""
        if getattr(self, "play_rows", None) is None:   # rows evaluated by play() calls
            self.play_rows = torch.zeros(1, dtype=torch.int64, device=self.device)
            # {table hits, table inserts} of play() calls (rvz_play_table)
            self.table_stats = torch.zeros(2, dtype=torch.int64, device=self.device)
            # rows play() left unread (skip_last_eval: searches whose batches after the first
            # each go to a fresh root child)
            self.play_unread = torch.zeros(1, dtype=torch.int64, device=self.device)
        if getattr(self, "play_roots_unread", None) is None:
            # root rows play() left out (skip_forced_roots: the forced searches' own roots)
            self.play_roots_unread = torch.zeros(1, dtype=torch.int64, device=self.device)
        if getattr(self, "play_ahead", None) is None:
            # {ahead rows evaluated, ahead rows taken} of play() calls (rvz_play_ahead)
            self.play_ahead = torch.zeros(2, dtype=torch.int64, device=self.device)
            self._call("rvz_play_ahead_stats", self.play_ahead.data_ptr())
        n = self.lib.rvz_play_scratch_size(self._h)
        sc = getattr(self, "_play_scratch", None)
        if sc is None or sc.numel() < n:
            self._play_scratch = torch.zeros(n, dtype=torch.float32, device=self.device)
        if evaluator is not None and hasattr(evaluator, "ovf_word"):
            evaluator.ovf_word()

    def play(self, evaluator, plies: int, temperature: float, seeds: torch.Tensor, stride: int,
             plies_done: torch.Tensor, games_done: torch.Tensor, reset: bool = True,
             skip_last_eval: bool = False, hist: Optional[torch.Tensor] = None,
             games_per_workgroup: int = 0, budget: Optional[torch.Tensor] = None,
             records=None, skip_forced_roots: bool = False):
        """rvz_play: every game commits `plies` plies (search of num_simulations + move + the
        autoreset bookkeeping of autoreset()) in ONE launch, the h2 LeafEvaluator's trunk and
        heads inside it; the same games, moves and counters as search() + act() + autoreset()
        with that evaluator (fused_softmax). idx_buf / p_buf: each game's last act. hist: int32
        [plies, n_games] for every act's index, or None. budget: int32 [n_games], game g commits
        min(plies, budget[g]) plies (the others stay as they are), or None. records: (black
        int64 [plies, G], white int64 [plies, G], side int32 [plies, G], p float64
        [plies, G, npol]): the position before every act and its policy vector (hist: the move;
        p_buf is then not written), or None. skip_forced_roots (with skip_last_eval): a search
        whose root has at least as many legal moves as it has batches after the first is played
        whole at its first step, without its root's row (play_roots_unread counts those rows);
        the same games. Graph-capturable once play_buffers() ran outside
        the capture (it runs here on the first eager call)."""
        from .network import LeafEvaluator
        if not isinstance(evaluator, LeafEvaluator):
            raise RvzError("play() runs the h2 LeafEvaluator inside the launch; another "
                           "evaluator goes through search() / act()")
        if evaluator.board_size != self.board_size or evaluator.device != self.device:
            raise RvzError("play(): the evaluator's board size / device differ from the engine's")
        for t, dt in ((seeds, torch.int64), (plies_done, torch.int64), (games_done, torch.int64)):
            if t.dtype != dt or t.numel() != self.n_games or not t.is_contiguous():
                raise RvzError("play: seeds / plies_done / games_done int64 [n_games]")
        if hist is not None and (hist.dtype != torch.int32 or hist.shape != (plies, self.n_games)
                                 or not hist.is_contiguous()):
            raise RvzError("play: hist int32 [plies, n_games]")
        if budget is not None and (budget.dtype != torch.int32 or budget.numel() != self.n_games
                                   or not budget.is_contiguous()
                                   or budget.device != self.device):
            raise RvzError("play: budget int32 [n_games] on the engine's device")
        rec = (None,) * 4
        if records is not None and hist is None:
            # the C-ABI's record contract: hist holds each recorded act's move (out_p is not
            # written when records are given), so records without hist would lose the moves
            raise RvzError("play: records need hist (the moves of the recorded plies)")
        if records is not None:
            rb, rw, rs, rp = records
            G = self.n_games
            if not (rb.dtype == rw.dtype == torch.int64 and rs.dtype == torch.int32
                    and rp.dtype == torch.float64 and rb.shape == rw.shape == rs.shape
                    == (plies, G) and rp.shape == (plies, G, self.npol)
                    and all(t.is_contiguous() and t.device == self.device
                            for t in (rb, rw, rs, rp))):
                raise RvzError("play: records = (black int64, white int64 [plies, G], side int32 "
                               "[plies, G], p float64 [plies, G, npol]) on the engine's device")
            rec = tuple(t.data_ptr() for t in records)
        n = self.lib.rvz_play_scratch_size(self._h)
        ready = (getattr(self, "play_rows", None) is not None and
                 getattr(self, "play_roots_unread", None) is not None and
                 getattr(self, "play_ahead", None) is not None and
                 getattr(self, "_play_scratch", None) is not None and
                 self._play_scratch.numel() >= n and getattr(evaluator, "_ovf", None) is not None)
        if not ready:
            if torch.cuda.is_current_stream_capturing():
                raise RvzError("play() inside a graph capture before its buffers exist: call "
                               "Engine.play_buffers(evaluator) (or one eager play) first")
            self.play_buffers(evaluator)
        sc = self._play_scratch
        self._bind(evaluator)
        a = _lib.PlayArgs(evaluator.params.data_ptr(), evaluator.wsplit.data_ptr(),
                          evaluator.filters, evaluator.n_blocks, sc.data_ptr(),
                          evaluator.ovf_word().data_ptr(), int(plies), int(bool(skip_last_eval)),
                          int(bool(reset)), int(games_per_workgroup), float(temperature),
                          seeds.data_ptr(), int(stride), plies_done.data_ptr(),
                          games_done.data_ptr(), self.idx_buf.data_ptr(), self.p_buf.data_ptr(),
                          hist.data_ptr() if hist is not None else None,
                          self.play_rows.data_ptr(),
                          budget.data_ptr() if budget is not None else None,
                          self.table_stats.data_ptr(), *rec, self.play_unread.data_ptr(),
                          int(bool(skip_forced_roots)), self.play_roots_unread.data_ptr())
        self._stream()
        self._call("rvz_play", C.byref(a))

    def ahead(self, mode: int = -1):
        """rvz_play_ahead: ahead rows of play()'s 8x8 / 64-filter form (0: off, 1: fill a pass's
        empty board slot, 2: also instead of holding an odd row, < 0: the default). The same
        games with any setting; play_ahead counts {rows evaluated ahead, rows taken}."""
        self._call("rvz_play_ahead", int(mode))

    def _bind(self, evaluator):
        """Remember the evaluator (check() reads its overflow word) and register this engine with
        it: LeafEvaluator.refresh() (new weights) then drops this engine's memo links itself."""
        evs = self.__dict__.setdefault("_evaluators", [])
        if not any(e is evaluator for e in evs):
            evs.append(evaluator)
            reg = getattr(evaluator, "bind_engine", None)
            if reg is not None:
                reg(self)

    def table(self, slots: int = 1 << 20, max_discs: int = 14):
        """rvz_play_table: the cross-game NN-output table of play() (slots = 0: off). A leaf whose
        position has at most max_discs discs takes the logits and value an earlier evaluation of
        the same position stored (any game of this engine, same weights): the same games, fewer
        evaluated rows. New weights: memo_reset() / LeafEvaluator.refresh() start a new
        generation. Call before capturing a graph."""
        self._stream()
        self._call("rvz_play_table", int(slots), int(max_discs))
        self.table_slots = int(slots)

    def play_gate(self, fraction: float = -1.0, timeout_us: float = 0.0, late_us: float = 0.0):
        """rvz_play_gate: the per-XCD pass gate of play()'s 8x8 forms of 128 / 256 filters (fraction 0: off; < 0:
        the default 0.8 / 400 us / 200 us). Timing only: the same games with any setting."""
        self._call("rvz_play_gate", float(fraction), float(timeout_us), float(late_us))

    def root_noise(self, alpha: float, epsilon: float, salt: int = 0):
        """rvz_search_root_noise: Dirichlet(alpha) noise mixed with weight epsilon into the priors
        of every search root's children (AlphaZero's exploration noise), in search() / act() and
        in play() alike; epsilon = 0 turns it off (the default: the reference's games, bit for
        bit). eta of a root is a function of the game's seed, the root's disc count, salt, alpha
        and the legal mask only (dirichlet_noise() returns the same rows). Not inside a search;
        set it before capturing a graph (a captured launch keeps the setting of its capture)."""
        _lib.check_noise_args(alpha, epsilon)
        self._call("rvz_search_root_noise", float(alpha), float(epsilon), int(salt) & 0xFFFFFFFF)
        self.noise = (float(alpha), float(epsilon), int(salt) & 0xFFFFFFFF)

    def openings(self, black: Optional[torch.Tensor], white: Optional[torch.Tensor] = None,
                 side: Optional[torch.Tensor] = None, salt: int = 0):
        """rvz_env_openings: games start from a pool of positions. black / white int64 [n] (bit
        patterns) and side [n] integers (1 black, 2 white to move), e.g. rvz.opening_suite's
        three; the engine keeps a copy of its own. From then on every reset (reset(),
        autoreset(), play()'s autoreset) with seed s puts the game on pool row
        rvz.opening_index(n, s, salt) with status {side, 0, -1, 0}; nothing else about the reset
        changes and no draw is consumed. openings(None) turns the pool off (the default: the
        start position). A row with overlapping discs, a bit off the board, a side other than
        1 | 2 or no legal square for the mover raises RvzError naming the first such row. The
        games already on the boards stay until they are reset. Not inside a search; it allocates
        and synchronises: set it before capturing a graph (a captured launch keeps the setting of
        its capture)."""
        self._stream()
        if black is None:
            self._call("rvz_env_openings", 0, None, None, None, 0)
            self.pool = None
            return
        if white is None or side is None:
            raise RvzError("openings: black, white and side, or None for off")
        n = black.numel()
        if n < 1 or black.dim() != 1 or white.shape != (n,) or side.shape != (n,) or \
                black.dtype != torch.int64 or white.dtype != torch.int64 or \
                side.dtype.is_floating_point or side.dtype == torch.bool:
            raise RvzError("openings: black / white int64 [n], side [n] integers, n >= 1")
        b = black.to(self.device).contiguous()
        w = white.to(self.device).contiguous()
        sd = side.to(self.device, torch.int32).contiguous()
        self._call("rvz_env_openings", n, b.data_ptr(), w.data_ptr(), sd.data_ptr(),
                   int(salt) & 0xFFFFFFFF)             # synchronises: b, w, sd may go
        self.pool = (n, int(salt) & 0xFFFFFFFF)

    def temperature_schedule(self, moves: Optional[int], late_temperature: float = 0.0):
        """rvz_act_schedule: a game's first `moves` moves are chosen at the temperature of the
        call (act() / play()), every later one at late_temperature (0: the most visited move, no
        draw). moves=None turns it off (the default: one temperature for every ply). Keyed by the
        disc count of the position before the move (from_discs = 4 + moves: every committed ply
        places a disc), so games at different move numbers share a launch and pull-style and
        fused play agree. Not inside a search; set it before capturing a graph (a captured
        launch keeps the setting of its capture)."""
        sched = _lib.check_schedule_args(moves, late_temperature)
        if sched is None:
            self._call("rvz_act_schedule", 0, 0.0)
        else:
            self._call("rvz_act_schedule", 4 + sched[0], sched[1])
        self.schedule = sched

    # ------------------------------------------------------------------ search
    def search_begin(self):
        self._call("rvz_search_begin")

    def search_step(self) -> bool:
        """One batch up to the NN call. False once every batch of this search was issued."""
        self._stream()
        rc = self._call("rvz_search_step", ptr(self.leaf_x), ptr(self.need))
        return rc != RVZ_DONE

    def compact(self, on: bool = True):
        """Compacted leaf batches (rvz_search_compact): the leaves that need an evaluation go to
        rows [0, U) of leaf_x, U on the device (live_count()); an evaluator with
        ``accepts_live_count`` evaluates only those rows (mcts.py:544-623 evaluates U leaves).
        Same visits, p and moves as the uncompacted search."""
        self._call("rvz_search_compact", int(bool(on)))
        self.compact_leaves = bool(on)

    def memo(self, on: bool = True):
        """NN-output memo across consecutive searches (rvz_search_memo): a leaf whose position
        the game's previous search expanded takes that expansion's priors and value instead of
        a new evaluation (the reference re-evaluates it: it rebuilds the tree every move,
        mcts.py:334). Same visits, p and moves; fewer evaluated rows. The evaluator must be
        row-deterministic and unchanged between searches: memo_reset() after new weights."""
        self._stream()
        self._call("rvz_search_memo", int(bool(on)))
        self.memo_on = bool(on)

    def memo_reset(self):
        """Forget the carried expansions (new evaluator weights); graph-capturable."""
        self._stream()
        self._call("rvz_search_memo_reset")

    def live_count(self) -> int:
        """Device address of the int32 live-row count of the most recently issued batch."""
        a = self.lib.rvz_search_live_count(self._h)
        if not a:
            raise RvzError("no live count: compaction off or no batch issued")
        return int(a)

    def rows_total(self) -> int:
        """Live rows evaluated over all completed searches (compaction on; the rows of a last
        batch left by skip_last_eval are not counted)."""
        out = C.c_int64()
        self._call("rvz_search_rows_total", C.byref(out))
        return int(out.value)

    def search_submit(self, policy: torch.Tensor, value: torch.Tensor, is_logits: bool):
        if policy.dtype != torch.float32 or value.dtype != torch.float32:
            raise RvzError("policy/value must be float32")
        if policy.shape != (self.n_games, self.npol) or value.shape != (self.n_games,):
            raise RvzError(f"policy must be [{self.n_games},{self.npol}], value [{self.n_games}]")
        self._stream()
        self._call("rvz_search_submit", ptr(policy), int(bool(is_logits)), ptr(value))
        # the expand + backup is deferred into the next launch: keep the rows alive until then
        self._keep = (policy, value)

    def search_skip(self):
        """Leave the last batch unevaluated (rvz_search_skip): same visits, p and move."""
        self._stream()
        self._call("rvz_search_skip")

    def search(self, evaluator: Callable[[torch.Tensor], Tuple[torch.Tensor, torch.Tensor]],
               fused_softmax: bool = True, skip_last_eval: bool = False):
        """MCTS.search for every live game. evaluator(leaf_x) -> (logits, value), or
        (probabilities, value) when the evaluator has ``outputs_probs = True``.

        fused_softmax=False applies torch's F.softmax (the reference's mcts.py:596) before the
        expand kernel instead of the kernel's fused softmax. skip_last_eval=True does not
        evaluate the last batch (rvz_search_skip; bit-identical visits, one NN call fewer) when
        a search has two batches or more: a single batch's leaf is the root, which the act needs
        expanded, so it is evaluated."""
        self._bind(evaluator)
        self.search_begin()
        k = 0
        while self.search_step():
            k += 1
            if skip_last_eval and k == self.n_batches > 1:
                self.search_skip()
                break
            if self.compact_leaves and getattr(evaluator, "accepts_live_count", False):
                logits, value = evaluator(self.leaf_x, n_live=self.live_count())
            else:
                logits, value = evaluator(self.leaf_x)
            logits = logits.float().contiguous()
            value = value.float().contiguous()
            if getattr(evaluator, "outputs_probs", False):
                # the evaluator hands over softmaxed rows (e.g. recorded reference outputs)
                self.search_submit(logits, value, False)
            elif fused_softmax:
                self.search_submit(logits, value, True)
            else:
                self.search_submit(torch.softmax(logits, dim=1).contiguous(), value, False)

    def visits(self) -> torch.Tensor:
        self._stream()
        self._call("rvz_search_visits", ptr(self.visits_buf))
        return self.visits_buf

    def act(self, temperature: float = 1.0, u: Optional[torch.Tensor] = None,
            apply: bool = True):
        """get_action_probs tail (+ make_move): returns (idx int32[G], p float64[G,npol])."""
        self._stream()
        uu = None
        if u is not None:
            uu = u.to(self.device, torch.float64).contiguous()
            self._u_keep = uu
        self._call("rvz_act", float(temperature), ptr(uu) if uu is not None else None,
                   int(bool(apply)), ptr(self.idx_buf), ptr(self.p_buf))
        return self.idx_buf, self.p_buf


# -------------------------------------------------------------------------- board kernels
def board_legal(black: torch.Tensor, white: torch.Tensor, status: torch.Tensor,
                board_size: int = 8) -> torch.Tensor:
    lib = _lib.load()
    n = black.numel()
    out = torch.empty(n, dtype=torch.int64, device=black.device)
    check(lib.rvz_board_legal(board_size, n, ptr(black), ptr(white), ptr(status), ptr(out),
                              _lib.stream_handle(black.device)), None, "rvz_board_legal")
    return out


def board_apply(black: torch.Tensor, white: torch.Tensor, status: torch.Tensor, sq: torch.Tensor,
                board_size: int = 8) -> torch.Tensor:
    """In place on (black, white, status); returns make_move's bool per board."""
    lib = _lib.load()
    n = black.numel()
    ok = torch.empty(n, dtype=torch.int32, device=black.device)
    check(lib.rvz_board_apply(board_size, n, ptr(black), ptr(white), ptr(status),
                              ptr(sq.to(torch.int32).contiguous()), ptr(ok),
                              _lib.stream_handle(black.device)), None, "rvz_board_apply")
    return ok


def board_canonical(black: torch.Tensor, white: torch.Tensor, status: torch.Tensor,
                    board_size: int = 8) -> torch.Tensor:
    lib = _lib.load()
    n = black.numel()
    out = torch.empty(n, 3, board_size, board_size, dtype=torch.float32, device=black.device)
    check(lib.rvz_board_canonical(board_size, n, ptr(black), ptr(white), ptr(status), ptr(out),
                                  _lib.stream_handle(black.device)), None, "rvz_board_canonical")
    return out


def dirichlet_noise(legal: torch.Tensor, seed32: torch.Tensor, tag: torch.Tensor, salt: int,
                    alpha: float, board_size: int = 8, bits: bool = False):
    """rvz_dirichlet_noise: the eta rows Engine.root_noise mixes into the roots' priors, by the
    same device function. legal int64 [n] (the roots' legal masks, bit patterns), seed32 [n] (the
    games' seeds, taken mod 2^32), tag [n] (the roots' disc counts). Returns eta float32
    [n, S*S+1] (0 at illegal squares and at the pass index), and with bits=True also the
    attempt-0 Philox4x32-10 block of every square, int32 [n, S*S, 4] (uint32 bit patterns)."""
    _lib.check_noise_args(alpha)
    check_board_size(board_size)
    lib = _lib.load()
    dev = legal.device
    lg = legal.to(torch.int64).contiguous()
    n = lg.numel()
    sd = seed32.to(dev).to(torch.int64).bitwise_and(0xFFFFFFFF).to(torch.int32).contiguous()
    tg = tag.to(dev).to(torch.int32).contiguous()
    if sd.numel() != n or tg.numel() != n:
        raise RvzError("dirichlet_noise: legal, seed32 and tag hold one entry per root")
    nsq = board_size * board_size
    out = torch.empty(n, nsq + 1, dtype=torch.float32, device=dev)
    ob = torch.empty(n, nsq, 4, dtype=torch.int32, device=dev) if bits else None
    if n:
        check(lib.rvz_dirichlet_noise(board_size, n, ptr(lg), ptr(sd), ptr(tg),
                                      int(salt) & 0xFFFFFFFF, float(alpha), ptr(out),
                                      ptr(ob) if bits else None, _lib.stream_handle(dev)),
              None, "rvz_dirichlet_noise")
    return (out, ob) if bits else out


def action_probs(visits: torch.Tensor, temperature, u: Optional[torch.Tensor] = None,
                 board_size: int = 8):
    """rvz_action_probs: get_action_probs' tail (mcts.py:656-692) for n rows of visit counts, by
    the device function Engine.act and Engine.play select with. visits int32 [n, S*S+1] on the
    device (e.g. Engine.visits()), temperature a number or one per row, u float64 [n] (the values
    np.random.random_sample() would return; None: zeros). Returns (idx int32 [n], p float64
    [n, S*S+1], drew int32 [n]: 1 where the row consumed its u), device tensors. A row with a
    negative count gets idx -3 and a zero p row."""
    check_board_size(board_size)
    npol = board_size * board_size + 1
    if visits.dim() != 2 or visits.shape[1] != npol:
        raise RvzError(f"visits must be [n, {npol}]")
    lib = _lib.load()
    dev = visits.device
    vis = visits.to(torch.int32).contiguous()
    n = vis.shape[0]
    t = torch.as_tensor(temperature, dtype=torch.float64).to(dev)
    t = t.expand(n).contiguous() if t.dim() == 0 else t.contiguous()
    uu = (torch.zeros(n, dtype=torch.float64, device=dev) if u is None
          else u.to(dev, torch.float64).contiguous())
    if t.shape != (n,) or uu.shape != (n,):
        raise RvzError("action_probs: temperature (unless a scalar) and u hold one entry per row")
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    p = torch.empty(n, npol, dtype=torch.float64, device=dev)
    drew = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        check(lib.rvz_action_probs(board_size, n, ptr(vis), ptr(t), ptr(uu), ptr(idx), ptr(p),
                                   ptr(drew), _lib.stream_handle(dev)), None, "rvz_action_probs")
    return idx, p, drew


def _rows_call(name, black, white, status, board_size, *mid, per_move=False):
    """The batched searches (solve, solve_window, solve_moves, alphabeta): lib.rvz_<name> on the
    rows; `mid` are the arguments the entry point takes between the rows and the outputs, as
    ctypes takes them. Returns the three outputs, fresh tensors on black's device; per_move: the
    first and third hold S*S + 1 entries per row. Every pointer is null when n == 0."""
    lib = _lib.load()
    n = black.numel()
    if status.shape != (n, 4) or white.numel() != n:
        raise RvzError(f"{name}: black and white hold one entry per row, status is [n, 4]")
    dev = black.device
    b = black.to(torch.int64).contiguous()
    w = white.to(dev, torch.int64).contiguous()
    st = status.to(dev, torch.int32).contiguous()
    shape = (n, int(board_size) ** 2 + 1) if per_move else (n,)
    score = torch.empty(shape, dtype=torch.int32, device=dev)
    move = torch.empty(n, dtype=torch.int32, device=dev)
    nodes = torch.empty(shape, dtype=torch.int64, device=dev)
    pb, pw, pst, pscore, pmove, pnodes, stream = (
        [ptr(t) for t in (b, w, st, score, move, nodes)] + [_lib.stream_handle(dev)]
        if n else [None] * 7)
    check(getattr(lib, "rvz_" + name)(int(board_size), n, pb, pw, pst, *mid, pscore, pmove,
                                      pnodes, stream), None, "rvz_" + name)
    return score, move, nodes


def _solve_call(name, black, white, status, board_size, *ints, per_move=False):
    """solve / solve_window / solve_moves: `ints` are max_empties, node_limit and what the entry
    point takes after them."""
    return _rows_call(name, black, white, status, board_size, *map(int, ints), per_move=per_move)


def solve(black: torch.Tensor, white: torch.Tensor, status: torch.Tensor, board_size: int = 8,
          max_empties: int = SOLVE_MAX_EMPTIES, node_limit: int = 2 ** 24):
    """rvz_solve: the exact value of n positions under the engine's rules (exhaustive negamax
    with alpha-beta pruning, one position per lane). black / white int64 [n] (bit patterns),
    status int32 [n, 4] (side, over, winner, passed), device tensors. Returns (score int32 [n],
    move int32 [n], nodes int64 [n]) on the inputs' device: score is the final disc difference
    from the side to move; move is the lowest-index best square, S*S for a forced pass, -2 for a
    root that is over (score valid), -3 above max_empties, -4 abandoned at node_limit visited
    positions, -5 for a malformed row (score 0 for -3 / -4 / -5); nodes counts the positions
    visited."""
    return _solve_call("solve", black, white, status, board_size, max_empties, node_limit)


def solve_window(black: torch.Tensor, white: torch.Tensor, status: torch.Tensor,
                 board_size: int = 8, max_empties: int = SOLVE_MAX_EMPTIES,
                 node_limit: int = 2 ** 24, alpha: int = -64, beta: int = 64,
                 order_min_empties: int = 0):
    """rvz_solve_window: solve() within the window (alpha, beta), -64 <= alpha < beta <= 64.
    Inputs and outputs as solve(). With v the exact score: score == v when alpha < v < beta,
    v <= score <= alpha when v <= alpha, beta <= score <= v when v >= beta (fail-soft); a root
    that is over reports its exact difference. move as solve(), but -6 when score <= alpha (fail
    low: no move reported), and when score >= beta a square whose own value is >= beta (the
    lowest-index one with order_min_empties = 0).
    order_min_empties = K > 0: nodes with at least K empty squares try the move that leaves the
    opponent the fewest replies first (ties to the lowest index); 0: increasing index everywhere,
    and then a row's nodes are at most solve()'s."""
    return _solve_call("solve_window", black, white, status, board_size, max_empties, node_limit,
                       alpha, beta, order_min_empties)


# solve_wld's default order_min_empties: the setting that measured fastest on the MI355X
# (profiles/solve02_wld_e10.json, solve02_wld_e12.json; solve_wld's docstring has the figures)
WLD_ORDER_MIN_EMPTIES = 4


def solve_wld(black: torch.Tensor, white: torch.Tensor, status: torch.Tensor, board_size: int = 8,
              max_empties: int = SOLVE_MAX_EMPTIES, node_limit: int = 2 ** 24,
              order_min_empties: int = WLD_ORDER_MIN_EMPTIES):
    """Win / draw / loss of n positions: solve_window with the window (-1, +1). Returns (outcome
    int32 [n] in {-1, 0, +1} for the side to move: the sign of the exact score; move; nodes).
    outcome is 0 wherever move is -3 / -4 / -5 (not solved); move is -6 for a loss.
    order_min_empties: see solve_window. The default, 4, is the fastest of 0 / 4 / 5 / 6 / 7 on
    32,768 8x8 rows (profiles/solve02_wld_e10.json, solve02_wld_e12.json): 0.63 s at 10 empties
    and 4.8 s at 12 against 2.2 s and 43 s with ordering off, far outside the 5 repeats' spread;
    5 ties with it within that spread (0.63 s, 4.6 s)."""
    score, move, nodes = solve_window(black, white, status, board_size, max_empties, node_limit,
                                      -1, 1, order_min_empties)
    return torch.sign(score), move, nodes


def solve_moves(black: torch.Tensor, white: torch.Tensor, status: torch.Tensor,
                board_size: int = 8, max_empties: int = SOLVE_MAX_EMPTIES,
                node_limit: int = 2 ** 24, alpha: int = -64, beta: int = 64,
                order_min_empties: int = 0):
    """rvz_solve_moves: the value of every root move of n positions, each move on a lane of its
    own. Inputs, window and ordering as solve_window(). Returns (scores int32 [n, S*S+1], count
    int32 [n], nodes int64 [n, S*S+1]) on the inputs' device; index S*S is the pass.
    count >= 1: the number of legal squares (1 for a root that can only pass); the entry of a
    legal square s is solve_window()'s score of the child make_move(root, s), seen from the
    root's side (window and sign mapped when the side changes; a move that ends the game scores
    its final difference), so with m the move's exact value, min(max(entry, alpha), beta) ==
    min(max(m, alpha), beta); nodes is that child's count. SOLVE_ABANDONED marks a move whose own
    search reached node_limit, SOLVE_NOT_A_MOVE (nodes 0) every entry that is no move of the row.
    A pass root's one entry, at S*S, is solve_window()'s answer for the root itself.
    count -2 (root over), -3 (above max_empties), -5 (malformed): the whole row is
    SOLVE_NOT_A_MOVE. Moves share no bounds: each is searched with the whole window."""
    return _solve_call("solve_moves", black, white, status, board_size, max_empties, node_limit,
                       alpha, beta, order_min_empties, per_move=True)


def solve_moves_wld(black: torch.Tensor, white: torch.Tensor, status: torch.Tensor,
                    board_size: int = 8, max_empties: int = SOLVE_MAX_EMPTIES,
                    node_limit: int = 2 ** 24, order_min_empties: int = WLD_ORDER_MIN_EMPTIES):
    """Win / draw / loss of every root move: solve_moves with the window (-1, +1), the scores
    reduced to their sign in {-1, 0, +1} for the side to move; SOLVE_NOT_A_MOVE and
    SOLVE_ABANDONED entries are kept. Returns (outcomes, count, nodes) as solve_moves()."""
    scores, count, nodes = solve_moves(black, white, status, board_size, max_empties, node_limit,
                                       -1, 1, order_min_empties)
    return torch.where(scores <= SOLVE_ABANDONED, scores, torch.sign(scores)), count, nodes


def best_moves(scores: torch.Tensor, count: torch.Tensor, alpha: int = -64, beta: int = 64):
    """The proven-optimal moves of solve_moves()' rows (pure torch, CPU or GPU tensors).
    Returns (best int32 [n], mask bool [n, S*S+1], complete bool [n]). With clamp(x) =
    min(max(x, alpha), beta): best is the maximum of clamp over the row's solved entries, mask
    marks the entries whose clamp equals it, complete means count >= 1 and no entry is
    SOLVE_ABANDONED. An entry's clamp equals its move's exact value's clamp (fail-soft), so for a
    complete row mask is exactly the set of moves optimal at the window's resolution: every best
    move at (-64, 64), every move of the best win / draw / loss class at (-1, 1). Rows that are
    not complete get best 0 and an all-false mask. alpha, beta: the window of the solve_moves()
    call (solve_moves_wld: -1, 1)."""
    if not -64 <= alpha < beta <= 64:
        raise RvzError("best_moves: the window must satisfy -64 <= alpha < beta <= 64")
    scores = scores.to(torch.int32)
    solved = scores > SOLVE_ABANDONED
    complete = (count >= 1) & ~(scores == SOLVE_ABANDONED).any(dim=1)
    clamped = torch.where(solved, scores.clamp(alpha, beta), torch.full_like(scores, -65))
    best = clamped.max(dim=1).values
    mask = solved & (clamped == best.unsqueeze(1)) & complete.unsqueeze(1)
    best = torch.where(complete, best, torch.zeros_like(best))
    return best, mask, complete


# alphabeta_weights: the value of a square by its distance from the nearest edges (row and
# column folded onto one quadrant, the smaller first), and the weight of one legal move more
_AB_SQUARE_CLASS = {(0, 0): 100, (0, 1): -20, (0, 2): 10, (0, 3): 5, (1, 1): -50, (1, 2): -2,
                    (1, 3): -2, (2, 2): -1, (2, 3): -1, (3, 3): -1}
_AB_MOBILITY = 10


def alphabeta_weights(board_size: int = 8):
    """The default evaluation of alphabeta(): a list of S*S + 1 ints, the square table in square
    index order and the mobility weight last. A classical table: corners 100, the squares
    diagonally next to a corner -50 (the lowest), the edge squares next to a corner -20, the
    other edge squares 10 and 5, the second ring -2, the centre -1; one legal move more than the
    opponent is worth 10. Invariant under the eight board symmetries and within
    RVZ_AB_HEUR_MAX (8x8: 928 + 64 * 10 = 1568; 6x6: 860 + 36 * 10 = 1220)."""
    check_board_size(board_size, "alphabeta_weights")
    bs = int(board_size)
    fold = lambda i: min(i, bs - 1 - i)
    table = [_AB_SQUARE_CLASS[tuple(sorted((fold(s // bs), fold(s % bs))))] for s in range(bs * bs)]
    return table + [_AB_MOBILITY]


def alphabeta(black: torch.Tensor, white: torch.Tensor, status: torch.Tensor, board_size: int = 8,
              depth: int = 4, weights: Optional[Sequence[int]] = None, node_limit: int = 2 ** 24):
    """rvz_alphabeta: the depth-limited value of n positions under the engine's rules (negamax
    `depth` placed discs deep with fail-soft alpha-beta pruning, one position per lane; passes cost
    no depth). Inputs as solve(). weights: S*S + 1 ints, the value of each square to its owner
    and, last, of one legal move more than the opponent (None: alphabeta_weights(board_size));
    sum |square| + S*S * |mobility| <= RVZ_AB_HEUR_MAX. Returns (score int32 [n], move int32 [n],
    nodes int64 [n]) on the inputs' device: score is the search's value for the side to move,
    +-(RVZ_AB_WIN + |final disc difference|) where the game is played out (0 for a draw); move is
    the lowest-index best square, S*S for a forced pass, -2 for a root that is over (score
    valid), -4 abandoned at node_limit visited positions, -5 for a malformed row (score 0 for
    -4 / -5); nodes counts the positions visited. 1 <= depth <= RVZ_AB_MAX_DEPTH."""
    nsq = int(board_size) ** 2
    if weights is None:
        weights = alphabeta_weights(board_size)
    wl = [int(x) for x in weights]
    if board_size in (6, 8) and len(wl) != nsq + 1:
        raise RvzError(f"alphabeta: weights must hold {nsq + 1} ints (S*S squares, then mobility)")
    if any(not -2 ** 31 <= x < 2 ** 31 for x in wl):
        raise RvzError("alphabeta: a weight does not fit int32")
    wt = (C.c_int32 * max(len(wl), 1))(*wl)       # host memory: read during the call only
    return _rows_call("alphabeta", black, white, status, board_size, int(depth),
                      C.cast(wt, C.c_void_p), int(node_limit))


def policy_softmax(logits: torch.Tensor, board_size: int = 8) -> torch.Tensor:
    """rvz_policy_softmax: F.softmax(logits, dim=1) (mcts.py:596) exactly as the engine's expand
    computes it from logits (the fused softmax of search_submit(is_logits=True) and of play())."""
    lib = _lib.load()
    lg = logits.float().contiguous()
    n = lg.shape[0]
    if lg.shape != (n, board_size * board_size + 1):
        raise RvzError(f"logits must be [n, {board_size * board_size + 1}]")
    out = torch.empty_like(lg)
    check(lib.rvz_policy_softmax(board_size, n, ptr(lg), ptr(out), _lib.stream_handle(lg.device)),
          None, "rvz_policy_softmax")
    return out
