"""ctypes binding of librvz.so (the C-ABI declared in include/rvz.h).

The library is built in-tree (``make -C alphazero-reversi_amd`` or ``__graft_entry__.build()``)
and is the ONLY implementation of the hot path: there is no CPU fallback. Loading fails loudly
when the library is missing, and every call that returns an error code raises ``RvzError``.

torch is imported first so that librvz.so binds to the HIP runtime torch already loaded (both
carry the soname libamdhip64.so.7): torch streams and tensors are then valid in our launches.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
import os

import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RVZ_LIB", os.path.join(_HERE, "librvz.so"))   # RVZ_LIB: experiments

RVZ_OK, RVZ_DONE = 0, 1
RVZ_LEAF_F32, RVZ_LEAF_BF16 = 0, 1
RVZ_DRAWS = 64          # move-sampling draws held per game (rvz_env_set_draws)
RVZ_SOLVE_MAX_EMPTIES = 14   # rvz_solve: the deepest root its per-lane stack holds
RVZ_SOLVE_NOT_A_MOVE, RVZ_SOLVE_ABANDONED = -128, -127     # rvz_solve_moves: entries without a score
RVZ_AB_MAX_DEPTH = 12        # rvz_alphabeta: the deepest search its per-lane stack holds
RVZ_AB_WIN = 20000           # rvz_alphabeta: a finished game scores +-(RVZ_AB_WIN + |disc difference|)
RVZ_AB_HEUR_MAX = 16000      # rvz_alphabeta: sum |weights[s]| + NSQ * |weights[NSQ]| at most


class RvzError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [("board_size", C.c_int32), ("n_games", C.c_int32),
                ("num_simulations", C.c_int32), ("batch_size", C.c_int32),
                ("c_puct", C.c_double), ("device", C.c_int32), ("leaf_dtype", C.c_int32)]


# name -> (restype, argtypes); kept in the order of include/rvz.h
_P = C.c_void_p
SIGNATURES = {
    "rvz_version": (C.c_int, []),
    "rvz_create": (C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    "rvz_destroy": (None, [_P]),
    "rvz_last_error": (C.c_char_p, [_P]),
    "rvz_set_stream": (C.c_int, [_P, _P]),
    "rvz_sync": (C.c_int, [_P]),
    "rvz_check": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "rvz_env_reset": (C.c_int, [_P, _P, _P]),
    "rvz_env_set_draws": (C.c_int, [_P, _P]),
    "rvz_env_draws": (C.c_int, [_P, _P]),
    "rvz_env_get": (C.c_int, [_P, _P, _P, _P]),
    "rvz_env_set": (C.c_int, [_P, _P, _P, _P]),
    "rvz_env_legal": (C.c_int, [_P, _P]),
    "rvz_env_apply": (C.c_int, [_P, _P, _P]),
    "rvz_board_legal": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    "rvz_board_apply": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "rvz_board_canonical": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    "rvz_policy_softmax": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P]),
    "rvz_search_begin": (C.c_int, [_P]),
    "rvz_search_step": (C.c_int, [_P, _P, _P]),
    "rvz_search_submit": (C.c_int, [_P, _P, C.c_int32, _P]),
    "rvz_env_autoreset": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, C.c_int32]),
    "rvz_resnet_h2_grid": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32]),
    "rvz_resnet_trunk_h2_ex": (C.c_int, [C.c_int32, _P, C.c_int32, _P, _P, C.c_int32,
                                         C.c_int32, _P, _P, _P, _P, C.c_int32, _P]),
    "rvz_resnet_heads_fc_ex": (C.c_int, [C.c_int32, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P,
                                         _P, _P, _P, _P]),
    "rvz_resnet_fwd_h2_ex": (C.c_int, [C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32,
                                       _P, _P, _P, _P, _P]),
    "rvz_search_compact": (C.c_int, [_P, C.c_int32]),
    "rvz_search_memo": (C.c_int, [_P, C.c_int32]),
    "rvz_search_memo_reset": (C.c_int, [_P]),
    "rvz_search_live_count": (C.c_void_p, [_P]),
    "rvz_search_root_noise": (C.c_int, [_P, C.c_double, C.c_double, C.c_uint32]),
    "rvz_dirichlet_noise": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, C.c_uint32, C.c_double,
                                      _P, _P, _P]),
    "rvz_search_rows_total": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "rvz_timer_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "rvz_timer_record": (C.c_int, [_P, C.c_int32, _P]),
    "rvz_timer_elapsed": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_float)]),
    "rvz_timer_destroy": (None, [_P]),
    "rvz_search_skip": (C.c_int, [_P]),
    "rvz_search_visits": (C.c_int, [_P, _P]),
    "rvz_act": (C.c_int, [_P, C.c_double, _P, C.c_int32, _P, _P]),
    "rvz_act_schedule": (C.c_int, [_P, C.c_int32, C.c_double]),
    "rvz_action_probs": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "rvz_solve": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, C.c_int64, _P, _P, _P,
                            _P]),
    "rvz_solve_window": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, C.c_int64,
                                   C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "rvz_solve_moves": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, C.c_int64,
                                  C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "rvz_alphabeta": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P, C.c_int64, _P, _P,
                                _P, _P]),
    "rvz_board_symmetry": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "rvz_training_rows": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, _P, _P,
                                    _P, _P]),
    "rvz_merge_scratch_size": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "rvz_merge_positions": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, _P, _P,
                                      _P, _P, _P, _P, _P, _P]),
    "rvz_replay_batch": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32,
                                   C.c_int32, _P, _P, C.c_int32, C.c_uint64, C.c_uint64, _P, _P,
                                   _P, _P, _P, _P]),
    "rvz_replay_ownership": (C.c_int, [C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P,
                                       _P]),
    "rvz_replay_cdf_size": (C.c_int64, [C.c_int32, C.c_int32]),
    "rvz_replay_cdf": (C.c_int, [C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "rvz_replay_batch_weighted": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int32,
                                            C.c_int32, C.c_int32, _P, _P, _P, C.c_int32,
                                            C.c_uint64, C.c_uint64, _P, _P, _P, _P, _P, _P, _P]),
    "rvz_replay_is_weight_scratch_size": (C.c_int64, [C.c_int32]),
    "rvz_replay_is_weight": (C.c_int, [C.c_int32, _P, _P, C.c_double, _P, _P, _P, _P]),
    "rvz_replay_priority_scratch_size": (C.c_int64, [C.c_int32]),
    "rvz_replay_priority": (C.c_int, [C.c_int32, _P, C.c_int32, _P, _P, C.c_double, C.c_double,
                                      C.c_int32, C.c_double, C.c_double, C.c_double, _P, _P, _P,
                                      _P, _P]),
    "rvz_replay_stale_scratch_size": (C.c_int64, [C.c_int32, C.c_int32]),
    "rvz_replay_stale": (C.c_int, [C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_int32, _P, C.c_int64, _P, _P, _P]),
    "rvz_replay_roots": (C.c_int, [C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P, _P,
                                   _P]),
    "rvz_replay_refresh_scratch_size": (C.c_int64, [C.c_int32]),
    "rvz_replay_refresh": (C.c_int, [C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P,
                                     C.c_int32, _P, C.c_int64, _P, _P]),
    "rvz_records_scratch_size": (C.c_int64, [C.c_int32, C.c_int32]),
    "rvz_records_games": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int32,
                                    _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rvz_records_final": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32,
                                    _P, _P, _P, _P, _P, _P, _P]),
    "rvz_openings_scratch_size": (C.c_int64, [C.c_int32, C.c_int32]),
    "rvz_openings": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "rvz_env_openings": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_uint32]),
    "rvz_opening_index": (C.c_int, [C.c_int32, C.c_int32, _P, C.c_uint32, _P, _P]),
    "rvz_loss_scratch_size": (C.c_int64, [C.c_int32, C.c_int32]),
    "rvz_policy_value_loss": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_double,
                                        C.c_double, _P, _P, _P, _P, _P, _P]),
    "rvz_ownership_loss_scratch_size": (C.c_int64, [C.c_int32, C.c_int32]),
    "rvz_ownership_loss": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rvz_score_loss_scratch_size": (C.c_int64, [C.c_int32, C.c_int32]),
    "rvz_score_loss": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, C.c_double, C.c_double, _P, _P,
                                 _P, _P, _P]),
    "rvz_play_scratch_size": (C.c_int64, [_P]),
    "rvz_play": (C.c_int, [_P, _P]),
    "rvz_play_table": (C.c_int, [_P, C.c_int64, C.c_int32]),
    "rvz_play_gate": (C.c_int, [_P, C.c_double, C.c_double, C.c_double]),
    "rvz_play_ahead": (C.c_int, [_P, C.c_int32]),
    "rvz_play_ahead_stats": (C.c_int, [_P, _P]),
    "rvz_counters": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "rvz_stats_enable": (C.c_int, [_P, C.c_int32]),
    "rvz_stats_read": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "rvz_timing_enable": (C.c_int, [_P, C.c_int32]),
    "rvz_timing_read": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "rvz_tree_nodes": (C.c_int, [_P]),
    "rvz_tree_export": (C.c_int, [_P, _P, _P]),
    "rvz_footprint": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "rvz_resnet_params_size": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "rvz_resnet_work_size": (C.c_int64, [C.c_int32]),
    "rvz_resnet_heads_fc": (C.c_int, [C.c_int32, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P,
                                      _P]),
    "rvz_resnet_h2_size": (C.c_int64, [C.c_int32, C.c_int32]),
    "rvz_resnet_h2_weights": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P]),
    "rvz_resnet_trunk_h2": (C.c_int, [C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32,
                                      _P, _P]),
    "rvz_resnet_fwd_h2": (C.c_int, [C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P,
                                    _P, _P, _P]),
}

_lib = None


class PlayArgs(C.Structure):
    """include/rvz.h rvz_play_args (pointers as integers: device addresses)."""
    _fields_ = [("params", C.c_void_p), ("blob", C.c_void_p), ("filters", C.c_int32),
                ("blocks", C.c_int32), ("scratch", C.c_void_p), ("ovf", C.c_void_p),
                ("plies", C.c_int32), ("skip_last_eval", C.c_int32), ("reset", C.c_int32),
                ("games_per_workgroup", C.c_int32), ("temperature", C.c_double),
                ("seeds", C.c_void_p), ("seed_stride", C.c_int64), ("plies_done", C.c_void_p),
                ("games_done", C.c_void_p), ("out_idx", C.c_void_p), ("out_p", C.c_void_p),
                ("hist", C.c_void_p), ("rows_evaluated", C.c_void_p),
                ("ply_budget", C.c_void_p), ("table_stats", C.c_void_p),
                ("rec_black", C.c_void_p), ("rec_white", C.c_void_p), ("rec_side", C.c_void_p),
                ("rec_p", C.c_void_p), ("rows_unread", C.c_void_p),
                ("skip_forced_roots", C.c_int32), ("roots_unread", C.c_void_p)]


def load() -> C.CDLL:
    """Load librvz.so (no GPU needed to load; calls that launch kernels need one)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RvzError(f"{LIB_PATH} is missing: build it with `make -C alphazero-reversi_amd` "
                           "(there is no CPU fallback for the rvz hot path)")
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def is_int(x) -> bool:
    """An int (any numbers.Integral) that is not a bool."""
    return isinstance(x, numbers.Integral) and not isinstance(x, bool)


def is_number(x, lo: float, hi: float, lo_open: bool = False, hi_open: bool = False) -> bool:
    """A real number (any numbers.Real, not a bool) in [lo, hi], an end marked open left out;
    NaN fails."""
    return (isinstance(x, numbers.Real) and not isinstance(x, bool)
            and (lo < x if lo_open else lo <= x) and (x < hi if hi_open else x <= hi))


_NO_EPSILON = object()


def check_noise_args(alpha, epsilon=_NO_EPSILON) -> None:
    """The argument rules of rvz_search_root_noise / rvz_dirichlet_noise, checked on the host
    before any device call: alpha a positive finite float32 (1e-37 .. 3e38), epsilon (when
    given) in [0, 1]."""
    try:
        a = float(alpha)
    except (TypeError, ValueError, OverflowError):
        raise RvzError(f"root noise: alpha must be a positive finite number, not {alpha!r}")
    if not 1.0e-37 <= a <= 3.0e38:
        raise RvzError(f"root noise: alpha must be positive and finite (float32), not {alpha!r}")
    if epsilon is not _NO_EPSILON:
        try:
            e = float(epsilon)
        except (TypeError, ValueError):
            raise RvzError(f"root noise: epsilon must be a number in [0, 1], not {epsilon!r}")
        if not 0.0 <= e <= 1.0:
            raise RvzError(f"root noise: epsilon must be in [0, 1], not {epsilon!r}")


def check_schedule_args(moves, late_temperature=0.0):
    """The argument rules of rvz_act_schedule (Engine.temperature_schedule), checked on the host
    before any device call: moves None (the schedule is off) or an int >= 0 (the moves of a game
    sampled at the call's temperature), late_temperature a finite number >= 0. Returns None (off)
    or (moves, late_temperature)."""
    if moves is None:
        return None
    if not is_int(moves) or moves < 0:
        raise RvzError(f"temperature schedule: moves must be None or an int >= 0, not {moves!r}")
    if int(moves) > 2 ** 31 - 5:
        raise RvzError(f"temperature schedule: moves = {moves!r} is out of range")
    try:
        late = float(late_temperature)
    except (TypeError, ValueError, OverflowError):
        raise RvzError("temperature schedule: late_temperature must be a finite number >= 0, "
                       f"not {late_temperature!r}")
    if isinstance(late_temperature, bool) or not (0.0 <= late < math.inf):
        raise RvzError("temperature schedule: late_temperature must be a finite number >= 0, "
                       f"not {late_temperature!r}")
    return int(moves), late


def check_board_size(board_size, who: str = "") -> None:
    """8 or 6; who: the caller's name, where its message begins with it."""
    if board_size not in (8, 6):
        raise RvzError((who + ": " if who else "") + "board_size must be 8 or 6")


def check(rc: int, handle=None, what: str = "") -> int:
    if rc < 0:
        msg = load().rvz_last_error(handle)
        raise RvzError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
    return rc


def ptr(t) -> int:
    """Device pointer of a contiguous CUDA (HIP) tensor; 16-byte aligned as the kernels assume."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RvzError("rvz buffers must be device tensors (no host fallback)")
    if not t.is_contiguous():
        raise RvzError("rvz buffers must be contiguous")
    p = t.data_ptr()
    if p % 16:
        raise RvzError("rvz buffers must be 16-byte aligned")
    return p


def stream_handle(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class Timer:
    """rvz_timer: stream-ordered HIP events without system fence (eager timing)."""

    def __init__(self, n_events: int):
        self.capacity = int(n_events)
        h = C.c_void_p()
        check(load().rvz_timer_create(self.capacity, C.byref(h)), None, "rvz_timer_create")
        self.h = h
        self.used = 0

    def record(self, stream_handle) -> int:
        if self.used >= self.capacity:
            raise RvzError("timer full")
        check(load().rvz_timer_record(self.h, self.used, stream_handle), None, "rvz_timer_record")
        self.used += 1
        return self.used - 1

    def elapsed(self, i: int, j: int) -> float:
        ms = C.c_float()
        check(load().rvz_timer_elapsed(self.h, i, j, C.byref(ms)), None, "rvz_timer_elapsed")
        return float(ms.value)

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            try:
                load().rvz_timer_destroy(h)
            except Exception:  # pragma: no cover - interpreter shutdown
                pass
