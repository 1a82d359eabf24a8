"""Data-parallel training of the policy/value net on self-play records.

Counterpart of the reference's ``AlphaZeroPipeline._train_epoch`` (src/trainer/pipeline.py:272-366):
AdamW(lr, weight_decay) (:91-97), CrossEntropy against ``argmax`` of the MCTS policy target plus
MSE on the value (:305-327, criterion :107-113), weighted sum, ``clip_grad_norm_`` (:333-337),
optimizer step. Differences by design:

* one process per GPU; the model is wrapped in DistributedDataParallel, whose bucketed gradient
  all-reduce runs over RCCL (backend "nccl" on ROCm) and overlaps the backward pass — the only
  collective of the whole self-play + training loop (config 4 of BASELINE.json);
* every rank trains on its own shard of the global sample order, drawn from one seeded
  permutation, so the global batch of a step is world_size x batch_size;
* the training arrays come straight from the engine's device-side records
  (``records_to_training``): no host round trip, no per-state Python lists;
* ``policy_target="full"`` (off by default) trains on the whole policy target, weighted per row,
  instead of its argmax (``rvz.full_policy_loss``; the rvz_policy_value_loss HIP kernels).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, Optional

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

from ._lib import is_number
from .engine import (SOLVE_ABANDONED, SOLVE_MAX_EMPTIES, best_moves, board_canonical, solve,
                     solve_moves, solve_moves_wld, solve_wld)
from .loss import full_ownership_loss, full_policy_loss, full_score_loss
from .records import merge_positions as _merge_positions, records_final, training_rows


def records_to_training(rec_black: torch.Tensor, rec_white: torch.Tensor, rec_side: torch.Tensor,
                        rec_idx: torch.Tensor, rec_p: torch.Tensor, final_status: torch.Tensor,
                        board_size: int = 8, canonical=None, exact_endgame: int = 0,
                        solver=None, exact_node_limit: int = 2 ** 24,
                        exact_wld: bool = False, exact_policy: int = 0,
                        moves_solver=None, symmetries: Optional[str] = None,
                        symmetry_seed: int = 0, augment=None, merge_positions: bool = False,
                        merger=None, compact: bool = False, ownership: bool = False,
                        finaler=None) -> Dict[str, torch.Tensor]:
    """Self-play records [plies, G] -> training arrays in the reference's layout and order.

    states f32 [n,3,S,S] (get_canonical_state of the position before each move), policy_targets
    f32 [n,S*S+1] (get_action_probs' p), value_targets f32 [n,1] = +1/-1/0 from the final winner
    relative to the player to move (self_play.py:117-126); games in order, plies in order
    (pipeline.py:179-246). Only plies that committed a move (rec_idx >= 0) are kept.
    canonical(black, white, status, board_size) -> planes: default the rvz_board_canonical HIP
    kernel (tests on a host without a GPU pass the oracle's restatement).
    exact_endgame = N > 0: every kept record whose position has at most N empty squares gets the
    exact value target sign(score) of the endgame solver (+1 / 0 / -1 relative to the player to
    move) in place of the played game's outcome; states and policy targets are untouched. A row
    the solver abandons at its node limit (move -4) keeps its outcome target. Two more keys then,
    0-d int64 tensors (no host synchronisation): "exact_rows", the rows replaced, and
    "exact_unsolved", the rows abandoned. N = 0 (the default) is off: the outputs of before.
    solver(black, white, status, board_size, max_empties) -> (score, move, ...): default rvz.solve
    (the rvz_solve HIP kernel) with node_limit = exact_node_limit.
    exact_wld = True: the default solver is rvz.solve_wld (rvz_solve_window with the window
    (-1, +1)) instead: the same targets, since only the sign is kept, from a smaller search;
    exact_rows / exact_unsolved can differ only through the node limit.
    exact_policy = N > 0 (independent of exact_endgame): every kept record with at most N empty
    squares whose every move the per-move solver decides (rvz.best_moves' `complete`) gets the
    policy target mask / mask.sum(), float32: uniform over the proven-optimal moves (the pass
    index for a root that can only pass), so its argmax, which DDPTrainer trains on by default, is
    the lowest-index optimal move (DDPTrainer(policy_target="full") trains on the whole row).
    Rows above N, and rows with an abandoned move, keep their MCTS target bit for bit; states
    and value targets are untouched. Two more keys then, 0-d int64
    (no host synchronisation): "exact_policy_rows", the rows replaced, and
    "exact_policy_unsolved", the rows within N with an abandoned move. N = 0 (the default) is
    off: the keys and bytes of before.
    moves_solver(black, white, status, board_size, max_empties) -> (scores, count, ...): default
    rvz.solve_moves (the rvz_solve_moves HIP kernel) at the full window, or with exact_wld
    rvz.solve_moves_wld and the window (-1, 1) (optimal then means: of the best win / draw / loss
    class), both with node_limit = exact_node_limit. A replacement is read at that same window.
    symmetries: None (the default: off, the keys and bytes of before), "all" or "random": board
    symmetry augmentation (include/rvz.h has the numbering T_0 .. T_7). It runs last, on the final
    policy and value targets, after the exact_endgame / exact_policy replacements. "all": every
    kept record becomes 8 rows, row 8*i + k its image under T_k (rows [::8] are the rows of
    symmetries=None), the value target repeated. "random": one image per kept record, sym drawn
    with torch.randint(0, 8, ...) from a CPU torch.Generator seeded with symmetry_seed, so the
    result is a pure function of the records and the seed. The states of an image are the images
    of the original's three planes: its third plane is the image of the original's legal mask
    (policy mass only where it is 1), not the engine's own mask of the image position, which can
    differ because move generation wraps around the board edges. Two more keys then, 0-d int64
    device tensors (no host synchronisation): "symmetry_rows", the rows after augmentation, and
    "symmetry_quirk_rows", the rows where those two masks differ. `canonical` is not called.
    augment(black, white, status, policy, sym, board_size, all_images) -> (states, policy, quirk):
    default rvz.training_rows (the rvz_training_rows HIP kernel) with quirk=True.
    merge_positions = True (the default False is off: the keys and bytes of before): one row per
    distinct position, two records being the same position iff their (mover, opponent) bitboards
    are equal (their states are then equal too). It runs after the exact_endgame / exact_policy
    replacements (exact targets are functions of the position, so a group's members agree and
    their mean reproduces them) and before `symmetries`, which then work on each group's first
    record and the merged policy. The rows are the distinct positions in order of first
    occurrence: states the canonical planes of each group's first record (`canonical` is called
    on those alone), policy_targets and value_targets the means over the group, summed in fixed
    point and so bitwise reproducible (include/rvz.h); a position recorded once keeps its targets
    bit for bit. Three more keys then: "position_counts" int32 [rows], each row's number of
    records (repeated 8 times under symmetries="all"), and two 0-d int64 device tensors,
    "merge_rows", the rows after merging, and "merge_input_rows", the records merged. Reading the
    number of rows is this option's one host synchronisation.
    merger(black, white, status, policy, value, board_size) -> dict with "m", "first", "count",
    "policy", "value": default rvz.merge_positions (the rvz_merge_positions HIP kernels).
    compact = True (the default False is off: the keys and bytes of before): the rows a
    rvz.ReplayBuffer holds. In place of "states" the result carries "mover" and "opponent", int64
    [n]: each kept record's bitboards from the side of the player to move (mover = black where
    the side is 1, else white, as rvz_board_canonical), from which rvz_replay_batch writes the
    planes when a row is drawn; `canonical` is not called. policy_targets, value_targets and every
    counter key are those of compact=False, after exact_endgame, exact_policy and merge_positions
    alike (with merging, the bitboards are those of each group's first record). compact=True
    together with `symmetries` raises ValueError: a compact row's symmetry is drawn every time it
    is sampled.
    ownership = True (the default False is off: the keys and bytes of before; needs compact=True):
    two more row keys, "final_mover" and "final_opponent" int64 [n]: the final position of each
    row's game from the row's mover's side (rvz.records_final, the engine's own make_move down the
    records), what a rvz.ReplayBuffer(ownership=True) holds as the row's ownership target. A row
    whose walk does not reach the end of its game (ok = 0: the game is still open at the last
    ply, or a record does not follow from the one before) is dropped from every key, before the
    exact targets are computed, and counted in "ownership_dropped", a 0-d int64 device tensor;
    reading the kept rows is this option's one host synchronisation. ValueError together with
    merge_positions (a merged row would need the mean ownership of its records, which two
    bitboards cannot hold) or with compact=False.
    finaler(rec_black, rec_white, rec_side, rec_idx, src, count, board_size) -> dict with
    "final_mover", "final_opponent", "ok": default rvz.records_final (the rvz_records_final HIP
    kernel).
    """
    o = _record_options(
        board_size=board_size, canonical=canonical, exact_endgame=exact_endgame, solver=solver,
        exact_node_limit=exact_node_limit, exact_wld=exact_wld, exact_policy=exact_policy,
        moves_solver=moves_solver, symmetries=symmetries, symmetry_seed=symmetry_seed,
        augment=augment, merge_positions=merge_positions, merger=merger, compact=compact,
        ownership=ownership, finaler=finaler)
    P, G = rec_idx.shape
    live = (rec_idx >= 0).t().reshape(-1)                    # game-major order
    fin = {}
    if ownership:
        # record (p, g) is window index p * G + g; the kept rows are game-major
        src = torch.arange(P * G, device=rec_idx.device).reshape(P, G).t().reshape(-1)[live]
        ok, fin = o.final_rows((rec_black, rec_white, rec_side, rec_idx), src.to(torch.int32))
        live = live.clone()
        live[live.nonzero().reshape(-1)[~ok]] = False
    black = rec_black.t().reshape(-1)[live].contiguous()
    white = rec_white.t().reshape(-1)[live].contiguous()
    side = rec_side.t().reshape(-1)[live]
    st = _status_rows(side)
    states = o.planes_now(black, white, st)
    policy = rec_p.permute(1, 0, 2).reshape(P * G, -1)[live].to(torch.float32)
    winner = final_status[:, 2].to(torch.int32).unsqueeze(0).expand(P, G).t().reshape(-1)[live]
    over = final_status[:, 1].unsqueeze(0).expand(P, G).t().reshape(-1)[live]
    v = torch.where(winner == side.to(torch.int32), 1.0, -1.0)
    v = torch.where(winner == 0, torch.zeros_like(v), v)
    v = torch.where(over != 0, v, -torch.ones_like(v))      # winner None -> -1 (self_play.py:121-126)
    return {**_training_tail(black, white, st, states, policy, v, o), **fin}


@dataclass(frozen=True)
class _RecordOptions:
    """The options records_to_training and games_to_training share, as their arguments of the
    same names (canonical and finaler with their defaults filled in)."""
    board_size: int
    canonical: Callable
    exact_endgame: int
    solver: Optional[Callable]
    exact_node_limit: int
    exact_wld: bool
    exact_policy: int
    moves_solver: Optional[Callable]
    symmetries: Optional[str]
    symmetry_seed: int
    augment: Optional[Callable]
    merge_positions: bool
    merger: Optional[Callable]
    compact: bool
    ownership: bool
    finaler: Callable

    def planes_now(self, black, white, st):
        """The canonical planes of the kept records, or None where a later step writes the states
        (merging, symmetries) or the rows carry none (compact)."""
        if self.symmetries is None and not self.merge_positions and not self.compact:
            return self.canonical(black, white, st, self.board_size)
        return None

    def final_rows(self, window, src):
        """ownership: the final positions of the records src of `window` (rec_black, rec_white,
        rec_side, rec_idx). Returns (ok, keys): ok bool [n], the records whose walk reaches the
        end of their game, and those records' "final_mover" / "final_opponent" with
        "ownership_dropped"."""
        fin = self.finaler(*window, src, None, self.board_size)
        ok = fin["ok"].to(src.device) != 0
        return ok, {"final_mover": fin["final_mover"][ok],
                    "final_opponent": fin["final_opponent"][ok], "ownership_dropped": (~ok).sum()}


def _record_options(canonical, finaler, **options) -> _RecordOptions:
    """The record options checked: the combinations both functions refuse."""
    o = _RecordOptions(canonical=board_canonical if canonical is None else canonical,
                       finaler=records_final if finaler is None else finaler, **options)
    if o.symmetries not in (None, "all", "random"):
        raise ValueError(f"symmetries must be None, 'all' or 'random', not {o.symmetries!r}")
    if o.compact and o.symmetries is not None:
        raise ValueError("compact=True leaves the symmetry to the replay buffer's draw: "
                         f"symmetries must be None, not {o.symmetries!r}")
    if o.ownership and o.merge_positions:
        raise ValueError("ownership=True keeps one final position per row: merge_positions must "
                         "be False (a merged row would need the mean ownership of its records)")
    if o.ownership and not o.compact:
        raise ValueError("ownership=True adds the final bitboards to the compact rows a replay "
                         "buffer holds: compact must be True")
    return o


def _status_rows(side: torch.Tensor) -> torch.Tensor:
    """The status {side, 0, -1, 0} of a position mid-game, int32 [n, 4]."""
    return torch.stack([side, torch.zeros_like(side), torch.full_like(side, -1),
                        torch.zeros_like(side)], dim=1).to(torch.int32).contiguous()


def _training_tail(black, white, st, states, policy, v, o: _RecordOptions):
    """What records_to_training and games_to_training share: the kept records (black, white, st
    [n, 4], policy float32 [n, S*S+1], v [n] from the games' outcomes; states the canonical planes
    or None where a later step writes them) through exact_endgame, exact_policy, merge_positions,
    compact and symmetries, in records_to_training's order and with its keys. Every target it
    computes is relative to the player to move."""
    board_size, exact_wld, limit = o.board_size, o.exact_wld, o.exact_node_limit
    # compact: the two bitboards are filled in below, once merging has chosen the rows
    out = {"mover": None, "opponent": None} if o.compact else {"states": states}
    out.update({"policy_targets": policy, "value_targets": v.reshape(-1, 1).float()})
    if o.exact_endgame:
        solver = o.solver if o.solver is not None else lambda b, w, s, bs, me: (
            solve_wld if exact_wld else solve)(b, w, s, bs, me, limit)
        score, move = solver(black, white, st, board_size, int(o.exact_endgame))[:2]
        solved = move >= 0                                   # -3: above N; -4: abandoned
        exact = torch.sign(score).to(torch.float32).reshape(-1, 1)
        out["value_targets"] = torch.where(solved.reshape(-1, 1), exact, out["value_targets"])
        out["exact_rows"] = solved.sum()
        out["exact_unsolved"] = (move == -4).sum()
    if o.exact_policy:
        moves_solver = o.moves_solver if o.moves_solver is not None else lambda b, w, s, bs, me: (
            solve_moves_wld if exact_wld else solve_moves)(b, w, s, bs, me, limit)
        scores, count = moves_solver(black, white, st, board_size, int(o.exact_policy))[:2]
        scores, count = scores.to(policy.device), count.to(policy.device)
        mask, complete = best_moves(scores, count, *((-1, 1) if exact_wld else (-64, 64)))[1:]
        exact = mask.to(torch.float32) / mask.sum(dim=1, keepdim=True).clamp(min=1)
        out["policy_targets"] = torch.where(complete.unsqueeze(1), exact, policy)
        out["exact_policy_rows"] = complete.sum()
        out["exact_policy_unsolved"] = ((count >= 1) & (scores == SOLVE_ABANDONED).any(dim=1)).sum()
    if o.merge_positions:
        rows_in = black.numel()
        merged = (_merge_positions if o.merger is None else o.merger)(
            black, white, st, out["policy_targets"].contiguous(),
            out["value_targets"].reshape(-1).contiguous(), board_size)
        m = int(merged["m"])
        first = merged["first"][:m].to(black.device, torch.int64)
        black, white, st = (t[first].contiguous() for t in (black, white, st))
        if o.symmetries is None and not o.compact:
            out["states"] = o.canonical(black, white, st, board_size)
        out["policy_targets"] = merged["policy"][:m]
        out["value_targets"] = merged["value"][:m].reshape(-1, 1)
        out["position_counts"] = merged["count"][:m]
        out["merge_rows"] = torch.tensor(m, dtype=torch.int64, device=black.device)
        out["merge_input_rows"] = torch.tensor(rows_in, dtype=torch.int64, device=black.device)
    if o.compact:
        mine = st[:, 0] == 1
        out["mover"] = torch.where(mine, black, white)
        out["opponent"] = torch.where(mine, white, black)
    if o.symmetries is not None:
        augment = o.augment if o.augment is not None else lambda b, w, s, p, sym, bs, every: (
            training_rows(b, w, s, p, sym, bs, every, quirk=True))
        every = o.symmetries == "all"
        sym = None
        if not every:
            g = torch.Generator().manual_seed(int(o.symmetry_seed))
            sym = torch.randint(0, 8, (black.numel(),), generator=g,
                                dtype=torch.int32).to(black.device)
        out["states"], out["policy_targets"], quirk = augment(
            black, white, st, out["policy_targets"].contiguous(), sym, board_size, every)
        if every:
            out["value_targets"] = out["value_targets"].repeat_interleave(8, dim=0)
            if o.merge_positions:
                out["position_counts"] = out["position_counts"].repeat_interleave(8)
        out["symmetry_rows"] = torch.tensor(out["states"].shape[0], dtype=torch.int64,
                                            device=out["states"].device)
        out["symmetry_quirk_rows"] = (quirk == 1).sum()
    return out


def games_to_training(rows: Dict[str, torch.Tensor], board_size: int = 8, canonical=None,
                      exact_endgame: int = 0, solver=None, exact_node_limit: int = 2 ** 24,
                      exact_wld: bool = False, exact_policy: int = 0, moves_solver=None,
                      symmetries: Optional[str] = None, symmetry_seed: int = 0, augment=None,
                      merge_positions: bool = False, merger=None,
                      compact: bool = True, ownership: bool = False, window=None,
                      finaler=None) -> Dict[str, torch.Tensor]:
    """rvz.records_games' rows -> training arrays: records_to_training for continuous self-play.

    rows: records_games' dict; its first m rows ("m": an int, or the 0-d device tensor, whose
    reading is this function's one host synchronisation) are the finished games' records, games
    in order, plies in order, "value" already relative to the player to move. They go through
    records_to_training's own tail as black = mover, white = opponent, side = 1 (a position from
    its mover's side, the equivalence rvz_replay_batch relies on), so every option means what it
    means there and the result carries the same keys: exact_endgame, exact_policy (with solver,
    moves_solver, exact_node_limit, exact_wld), merge_positions (merger), symmetries (augment,
    symmetry_seed) and compact, which defaults to True here: "mover" and "opponent" in place of
    "states", the rows a rvz.ReplayBuffer holds (compact=False calls `canonical` for the planes).
    Every target those options compute is relative to the mover, so they compose with the value
    targets rows carries.
    ownership = True: records_to_training's option of that name, with `window` = (rec_black,
    rec_white, rec_side, rec_idx), the window records_games cut (rows["src"] indexes it):
    "final_mover" / "final_opponent" per row and "ownership_dropped". Every emitted row belongs
    to a game that ended inside the window, so nothing is dropped unless the window changed."""
    o = _record_options(
        board_size=board_size, canonical=canonical, exact_endgame=exact_endgame, solver=solver,
        exact_node_limit=exact_node_limit, exact_wld=exact_wld, exact_policy=exact_policy,
        moves_solver=moves_solver, symmetries=symmetries, symmetry_seed=symmetry_seed,
        augment=augment, merge_positions=merge_positions, merger=merger, compact=compact,
        ownership=ownership, finaler=finaler)
    if ownership and (window is None or len(window) != 4):
        raise ValueError("ownership=True needs window=(rec_black, rec_white, rec_side, rec_idx), "
                         "the records rows was cut from")
    m = int(rows["m"])
    fin = {}
    if ownership:
        ok, fin = o.final_rows(window, rows["src"][:m])
        rows = {k: rows[k][:m][ok] for k in ("mover", "opponent", "policy", "value")}
        m = rows["mover"].numel()
    black, white = rows["mover"][:m].contiguous(), rows["opponent"][:m].contiguous()
    st = _status_rows(torch.ones(m, dtype=torch.int32, device=black.device))
    return {**_training_tail(black, white, st, o.planes_now(black, white, st),
                             rows["policy"][:m], rows["value"][:m].reshape(-1), o), **fin}


def adjudicate(black: torch.Tensor, white: torch.Tensor, status: torch.Tensor, board_size: int,
               solver=None, node_limit: int = 2 ** 24, check_depth: bool = True):
    """Endgame adjudication: the final status of games stopped short of their end, each live
    game's winner taken from a win / draw / loss solve of its position.

    black / white int64 [G], status int32 [G, 4] (side, over, winner, passed): the games after the
    shortened self-play. Returns (final_status int32 [G, 4], keep bool [G], stats). A game that is
    over keeps its status and is kept. Any other game is solved: over = 1 and winner = the side to
    move for +1, the other side for -1, 0 for a draw; a game the solver abandons at its node limit
    (move -4) keeps its status and gets keep = False (its records are to be dropped). stats: 0-d
    int64 tensors "adjudicated" (live games solved), "adjudicate_unsolved" (abandoned) and
    "already_over".
    A live game with more than 14 empty squares (SOLVE_MAX_EMPTIES; the solver's code -3) cannot
    be adjudicated: with check_depth (the default) that raises ValueError, at the cost of the
    function's only host read; a caller that has established the depth of its games itself
    (SelfPlayTrainer has: every live game holds exactly N empties) passes check_depth=False, and
    then nothing here synchronises with the host (such a game would get keep = False).
    solver(black, white, status, board_size, max_empties) -> (outcome or score, move, ...):
    default rvz.solve_wld with max_empties = 14 and node_limit; only the sign of its first output
    is read, so records_to_training's solvers fit."""
    if solver is None:
        def solver(b, w, s, bs, me):
            return solve_wld(b, w, s, bs, me, node_limit)
    st = status.to(torch.int32)
    over = st[:, 1] != 0
    score, move = solver(black, white, st, board_size, SOLVE_MAX_EMPTIES)[:2]
    score, move = score.to(st.device), move.to(st.device)
    if check_depth and bool((~over & (move == -3)).any()):
        raise ValueError(f"adjudicate: a live game has more than {SOLVE_MAX_EMPTIES} empty squares")
    solved = ~over & ((move >= 0) | (move == -6))
    side = st[:, 0]
    sg = torch.sign(score).to(torch.int32)
    winner = torch.where(sg > 0, side, torch.where(sg < 0, 3 - side, torch.zeros_like(side)))
    final = st.clone()
    final[:, 1] = torch.where(solved, torch.ones_like(side), st[:, 1])
    final[:, 2] = torch.where(solved, winner, st[:, 2])
    unsolved = ~over & (move == -4)
    stats = {"adjudicated": solved.sum(), "adjudicate_unsolved": unsolved.sum(),
             "already_over": over.sum()}
    return final, over | solved, stats


def check_ownership_coef(ownership_coef) -> float:
    """DDPTrainer's rule for ownership_coef (SelfPlayTrainer checks it too)."""
    if not is_number(ownership_coef, 0.0, float("inf"), hi_open=True):
        raise ValueError(f"ownership_coef must be a finite number >= 0, not "
                         f"{ownership_coef!r}")
    return float(ownership_coef)


def check_score_coef(score_coef) -> float:
    """DDPTrainer's rule for score_coef (SelfPlayTrainer checks it too)."""
    if not is_number(score_coef, 0.0, float("inf"), hi_open=True):
        raise ValueError(f"score_coef must be a finite number >= 0, not {score_coef!r}")
    return float(score_coef)


def check_policy_target(policy_target, count_weights) -> None:
    """DDPTrainer's rule for policy_target and count_weights (SelfPlayTrainer checks it too)."""
    if policy_target not in ("argmax", "full"):
        raise ValueError(f"policy_target must be 'argmax' or 'full', not {policy_target!r}")
    if count_weights and policy_target != "full":
        raise ValueError("count_weights=True weights the rows of the full policy loss: "
                         "policy_target must be 'full'")


def _drawn(batch, with_prob: bool, ownership: bool) -> dict:
    """The outputs of ReplayBuffer.sample by name: prob is there with with_prob=True, ownership
    and margin with a ReplayBuffer(ownership=True)."""
    names = ("states", "policy", "value", "slot", "sym") + (("prob",) if with_prob else ()) + \
        (("ownership", "margin") if ownership else ())
    return dict(zip(names, batch))


class DDPTrainer:
    def __init__(self, model: nn.Module, lr: float = 1e-3, weight_decay: float = 1e-4,
                 gradient_clip: float = 1.0, policy_loss_weight: float = 1.0,
                 value_loss_weight: float = 1.0, batch_size: int = 64, bucket_cap_mb: int = 25,
                 lr_milestones=(), lr_gamma: float = 0.1, policy_target: str = "argmax",
                 count_weights: bool = False, loss_fn=None, ownership_coef: float = 0.0,
                 ownership_loss_fn=None, score_coef: float = 0.0,
                 score_weights=(1.0, 1.0), score_loss_fn=None):
        """Defaults = the reference's TrainingConfig (config.py:46-60): AdamW(lr 1e-3, weight decay
        1e-4), clip 1.0, loss weights 1, batch 64, MultiStepLR(milestones [], gamma 0.1)
        (pipeline.py:91-105), stepped once per iteration (scheduler_step, pipeline.py:131).
        policy_target: "argmax" (the default: the reference's criterion, cross-entropy against
        the argmax of the policy target) or "full": AlphaZero's own loss -pi . log p on the whole
        target distribution plus the squared value error, a weighted mean over the batch's rows
        (rvz.full_policy_loss; the rvz_policy_value_loss HIP kernels, float64, deterministic).
        The loss dict then gains "train/policy_kl" (the policy loss minus the mean target
        entropy: the divergence of the net's policy from the target) and
        "train/policy_agreement" (the weighted share of rows whose argmax the net matches).
        count_weights (needs "full"): train_epoch weights every row by data["position_counts"],
        the records a merged row stands for (records_to_training(merge_positions=True)).
        loss_fn(logits, value, policy_targets, value_targets, weights, policy_weight,
        value_weight, board_size) -> (loss, policy_loss, value_loss, stats): default
        rvz.full_policy_loss (tests on a host without a GPU pass the NumPy reference).
        ownership_coef = c > 0 (0, the default, is off: the steps and the loss dict of before):
        train_replay, on a ReplayBuffer(ownership=True), adds c * L_own to every step's loss,
        L_own the ownership head's loss on the drawn rows' final-ownership targets
        (rvz.full_ownership_loss; the rvz_ownership_loss HIP kernels, float64, deterministic),
        with the rows' weights of the policy term. The loss dict then gains
        "train/ownership_loss" and "train/ownership_agreement". c > 0 exactly when the model has
        the head (AlphaZeroNetwork(ownership_head=True)), ValueError otherwise: a head that no
        loss reads leaves DistributedDataParallel's reducer waiting for its gradient.
        ownership_loss_fn(logits, targets, weights, board_size) -> (loss, stats): default
        rvz.full_ownership_loss.
        score_coef = c > 0 (0, the default, is off: the steps and the loss dict of before):
        train_replay, on a ReplayBuffer(ownership=True), adds c * L_score to every step's loss,
        L_score = score_weights[0] * P + score_weights[1] * Q the score head's loss on the drawn
        rows' final disc margins: P the cross-entropy of the margin's class, Q the squared
        distance of the cumulative distributions (rvz.full_score_loss; the rvz_score_loss HIP
        kernels, float64, deterministic), with the rows' weights of the policy term. The loss
        dict then gains "train/score_loss", "train/score_pdf", "train/score_cdf",
        "train/score_abs_error" (the mean distance, in discs, of the predicted mean margin from
        the game's) and "train/score_agreement". c > 0 exactly when the model has the head
        (AlphaZeroNetwork(score_head=True)), ValueError otherwise, for ownership_coef's reason.
        The two coefficients are independent of each other.
        score_loss_fn(logits, margin, weights, pdf_weight, cdf_weight, board_size) ->
        (loss, stats): default rvz.full_score_loss."""
        self.score_coef = check_score_coef(score_coef)
        if (self.score_coef > 0.0) != bool(getattr(model, "score_head", False)):
            raise ValueError("score_coef > 0 goes with a model that has the score head "
                             "(AlphaZeroNetwork(score_head=True)) and 0 with one that has "
                             "none: an unused head breaks DistributedDataParallel's reducer")
        if (not isinstance(score_weights, (tuple, list)) or len(score_weights) != 2 or
                not all(is_number(x, 0.0, float("inf"), hi_open=True) for x in score_weights)):
            raise ValueError("score_weights must be two finite numbers >= 0 (pdf, cdf), not "
                             f"{score_weights!r}")
        self.score_weights = (float(score_weights[0]), float(score_weights[1]))
        self.score_loss_fn = full_score_loss if score_loss_fn is None else score_loss_fn
        self.last_score = None      # the (loss, stats) of the last step's score term
        self.ownership_coef = check_ownership_coef(ownership_coef)
        if (self.ownership_coef > 0.0) != bool(getattr(model, "ownership_head", False)):
            raise ValueError("ownership_coef > 0 goes with a model that has the ownership head "
                             "(AlphaZeroNetwork(ownership_head=True)) and 0 with one that has "
                             "none: an unused head breaks DistributedDataParallel's reducer")
        self.ownership_loss_fn = (full_ownership_loss if ownership_loss_fn is None
                                  else ownership_loss_fn)
        self.last_ownership = None  # the (loss, stats) of the last step's ownership term
        check_policy_target(policy_target, count_weights)
        self.policy_target, self.count_weights = policy_target, bool(count_weights)
        self.loss_fn = full_policy_loss if loss_fn is None else loss_fn
        self.last_stats = None      # "full": the stats of the last train_step (0-d tensors)
        # the loss dict's keys, in the order _step_totals fills its vector
        self._loss_keys = ("train/loss", "train/policy_loss", "train/value_loss") + \
            (("train/policy_kl", "train/policy_agreement") if policy_target == "full" else ()) + \
            (("train/ownership_loss", "train/ownership_agreement")
             if self.ownership_coef > 0.0 else ()) + \
            (("train/score_loss", "train/score_pdf", "train/score_cdf", "train/score_abs_error",
              "train/score_agreement") if self.score_coef > 0.0 else ())
        self.model = model
        self.device = next(model.parameters()).device
        self.distributed = dist.is_available() and dist.is_initialized()
        if self.distributed:
            kw = {"device_ids": [self.device.index]} if self.device.type == "cuda" else {}
            # gradients of ~3 M parameters (10x128) = 11.9 MB: one 25 MB bucket, one all-reduce
            self.net = nn.parallel.DistributedDataParallel(model, bucket_cap_mb=bucket_cap_mb,
                                                           broadcast_buffers=True, **kw)
        else:
            self.net = model
        self.opt = torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=weight_decay)
        self.scheduler = torch.optim.lr_scheduler.MultiStepLR(self.opt, milestones=list(lr_milestones),
                                                              gamma=lr_gamma)
        self.clip = gradient_clip
        self.wp, self.wv = policy_loss_weight, value_loss_weight
        self.batch_size = batch_size

    @torch.no_grad()
    def sync_buffers(self):
        """Broadcast rank 0's BN running statistics: DDP broadcasts buffers before each forward,
        but the last forward of an epoch updates them locally, so without this the ranks would
        self-play with slightly different nets."""
        if not self.distributed:
            return
        for b in self.model.buffers():
            dist.broadcast(b, 0)

    def scheduler_step(self):
        """The per-iteration learning-rate step of the reference's train loop (pipeline.py:131)."""
        self.scheduler.step()

    def rank_world(self):
        return (dist.get_rank(), dist.get_world_size()) if self.distributed else (0, 1)

    def train_step(self, states, policy_targets, value_targets, weights=None, rows=False,
                   ownership=None, margin=None):
        """One optimizer step (pipeline.py:297-340); returns (loss, policy_loss, value_loss).
        weights (policy_target="full" only): float32 [n], each row's weight in the batch's mean;
        None weights every row 1. In "full" mode last_stats holds the step's loss_fn stats; with
        rows=True ("full" only) loss_fn is asked for its per-row losses, last_stats["rows"].
        ownership (ownership_coef > 0 only, and required then): float32 [n, S*S], the rows'
        final-ownership targets; ownership_coef times the head's loss on them, under the same
        weights, is added to the loss, and last_ownership holds that term's (loss, stats).
        margin (score_coef > 0 only, and required then): float32 [n], the rows' final disc
        margins; score_coef times the score head's loss on them, under the same weights, is
        added to the loss, and last_score holds that term's (loss, stats)."""
        if (weights is not None or rows) and self.policy_target != "full":
            raise ValueError("train_step: weights and rows need policy_target='full'")
        if (ownership is not None) != (self.ownership_coef > 0.0):
            raise ValueError("train_step: ownership targets go with ownership_coef > 0 (they "
                             "come from train_replay on a ReplayBuffer(ownership=True))")
        if (margin is not None) != (self.score_coef > 0.0):
            raise ValueError("train_step: margin goes with score_coef > 0 (it comes from "
                             "train_replay on a ReplayBuffer(ownership=True))")
        self.net.train()
        self.opt.zero_grad()
        if ownership is not None or margin is not None:
            logits, value, *aux = self.net(states, aux=True)     # ownership, then score
            own_logits = aux[0] if ownership is not None else None
            score_logits = aux[-1] if margin is not None else None
        else:
            logits, value = self.net(states)
        if self.policy_target == "full":
            board = int(getattr(self.model, "board_size", 8))
            loss, policy_loss, value_loss, self.last_stats = self.loss_fn(
                logits.view(-1, logits.size(-1)), value.squeeze(-1), policy_targets,
                value_targets.reshape(-1), weights, self.wp, self.wv, board,
                **({"rows": True} if rows else {}))
        else:
            policy_loss = F.cross_entropy(logits.view(-1, logits.size(-1)),
                                          policy_targets.argmax(dim=1))
            value_loss = F.mse_loss(value.squeeze(-1), value_targets.reshape(-1))
            loss = self.wp * policy_loss + self.wv * value_loss
        if ownership is not None:
            board = int(getattr(self.model, "board_size", 8))
            own_loss, own_stats = self.ownership_loss_fn(own_logits, ownership, weights, board)
            self.last_ownership = (own_loss.detach(), own_stats)
            loss = loss + self.ownership_coef * own_loss
        if margin is not None:
            board = int(getattr(self.model, "board_size", 8))
            score_loss, score_stats = self.score_loss_fn(
                score_logits, margin, weights, *self.score_weights, board)
            self.last_score = (score_loss.detach(), score_stats)
            loss = loss + self.score_coef * score_loss
        loss.backward()                      # DDP: bucketed RCCL all-reduce during backward
        if self.clip > 0:
            torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.clip)
        self.opt.step()
        return loss.detach(), policy_loss.detach(), value_loss.detach()

    def _step_totals(self, losses, priority=None):
        """The per-step summands of the loss dict, in the order of its keys: the three losses, in
        "full" mode the policy KL and the agreement, with ownership_coef > 0 the ownership term's
        loss and agreement, with score_coef > 0 the score term's five, and `priority`,
        train_replay's two of a prioritized step."""
        vals = [x.double() for x in losses]
        if self.policy_target == "full":
            st = self.last_stats
            vals += [losses[1].double() - st["target_entropy"].double(),
                     st["agreement"].double()]
        if self.ownership_coef > 0.0:
            own_loss, own_stats = self.last_ownership
            vals += [own_loss.double(), own_stats["agreement"].double().to(own_loss.device)]
        if self.score_coef > 0.0:
            score_loss, st = self.last_score
            vals += [score_loss.double()] + [st[k].double().to(score_loss.device) for k in
                                             ("pdf_loss", "cdf_loss", "abs_error", "agreement")]
        vals = torch.stack(vals)
        return vals if priority is None else torch.cat([vals, priority.to(vals.device)])

    def _loss_dict(self, keys, tot, steps):
        """The loss dict of `steps` steps: tot holds the mean of each of `keys`."""
        pairs = [(k, float(x)) for k, x in zip(keys, tot)]
        return dict(pairs[:3] + [("train/lr", self.opt.param_groups[0]["lr"]), ("steps", steps)] +
                    pairs[3:])

    def _min_steps(self, steps: int) -> int:
        """Every rank must run the same number of DDP steps: the minimum over ranks."""
        if self.distributed:
            t = torch.tensor([steps], dtype=torch.int64,
                             device=self.device if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            steps = int(t.item())
        return steps

    def _rank_mean(self, tot: torch.Tensor) -> torch.Tensor:
        """The job's loss: the mean over ranks."""
        ranks = self.rank_world()[1]
        if self.distributed and ranks > 1:
            t = tot.to(self.device if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(t)
            tot = t / ranks
        return tot

    def train_epoch(self, data: Dict[str, torch.Tensor], seed: int = 0,
                    max_steps: Optional[int] = None, local_data: bool = False
                    ) -> Dict[str, float]:
        """One pass over the data. local_data=False: `data` is identical on every rank and each
        rank takes every world-th batch of one seeded permutation. local_data=True: every rank
        holds its own data (its own self-play games, rvz.pipeline) and walks its own permutation
        (seed * world + rank). Either way each step's global batch is world x batch_size, and
        every rank runs the same number of steps (the minimum over ranks). Returns the
        reference's averaged loss dict (pipeline.py:342-366), averaged over ranks too.
        Order: the permutation the reference's DataLoader(shuffle=True) draws when handed a
        generator seeded with `seed` (its base-seed draw, then randperm(n)). On one
        process the last partial batch is trained too, as the reference's DataLoader (no
        drop_last) does; across ranks every step is a full world x batch_size batch.
        With count_weights every row is weighted by data["position_counts"] (ValueError when the
        key is missing)."""
        if self.ownership_coef > 0.0:
            raise ValueError("train_epoch: ownership_coef > 0 trains through train_replay (the "
                             "ownership targets are a ReplayBuffer(ownership=True)'s)")
        if self.score_coef > 0.0:
            raise ValueError("train_epoch: score_coef > 0 trains through train_replay (the "
                             "margins are a ReplayBuffer(ownership=True)'s)")
        if self.count_weights and "position_counts" not in data:
            raise ValueError("train_epoch: count_weights=True needs data['position_counts'] "
                             "(records_to_training(merge_positions=True))")
        rank, world = self.rank_world()
        n = data["states"].shape[0]
        # local data: one stream per (seed, rank) pair, seed * world + rank, so rank r at seed s
        # never repeats rank r + 1's shuffle at seed s - 1 (the pipeline passes seed + iteration)
        g = torch.Generator().manual_seed(seed * world + rank if local_data else seed)
        # DataLoader(shuffle=True, generator=g) first draws its workers' base seed from g, then
        # the RandomSampler's permutation: the same two draws give the same batches
        torch.empty((), dtype=torch.int64).random_(generator=g)
        order = torch.randperm(n, generator=g)
        if local_data:
            rank, world = 0, 1        # indexing within this rank's own permutation
        per_step = self.batch_size * world
        partial = not self.distributed and world == 1
        steps = -(-n // per_step) if partial else n // per_step
        if max_steps is not None:
            steps = min(steps, max_steps)
        steps = self._min_steps(steps)
        tot = torch.zeros(len(self._loss_keys), dtype=torch.float64, device=self.device)
        for s in range(steps):
            idx = order[s * per_step + rank * self.batch_size:
                        s * per_step + (rank + 1) * self.batch_size].to(self.device)
            tot += self._step_totals(self.train_step(
                data["states"][idx], data["policy_targets"][idx], data["value_targets"][idx],
                *((data["position_counts"][idx].to(torch.float32),) if self.count_weights
                  else ())))
        tot /= max(1, steps)
        return self._loss_dict(self._loss_keys, self._rank_mean(tot), steps)

    def train_replay(self, buffer, steps: int, seed: int = 0, symmetries: bool = True,
                     priority_beta: float = 0.4) -> Dict[str, float]:
        """`steps` optimizer steps on minibatches drawn from a rvz.ReplayBuffer: step s trains
        on buffer.sample(batch_size, seed * world + rank, s, symmetries), a uniform draw with
        replacement over the rows held, each under a fresh board symmetry. The buffer is this
        rank's own (its own self-play games), and the seed is spread over the ranks as
        train_epoch(local_data=True) spreads it; each step's global batch is world x batch_size,
        and every rank runs the same number of steps (the minimum over ranks). Returns
        train_epoch's loss dict, averaged over ranks too. The ring stores no record counts, so
        in "full" mode every drawn row weighs 1. With a ReplayBuffer(weighted=True) the draw is in
        proportion to the rows' sampling weights instead; where those are record counts
        (SelfPlayTrainer(replay_sampling="counts")) the sampling carries the counts, and every
        drawn row still weighs 1 in the loss.
        With a ReplayBuffer(prioritized=True) every step is one round of prioritized replay: the
        batch is drawn with its probabilities, every row weighs its importance weight
        (pmin / prob) ** priority_beta in the loss (buffer.is_weights; 0.4 is where Schaul et al.
        start their anneal, 1 corrects the sampling bias in full), and the step's per-row losses
        become the drawn rows' new priorities (buffer.update_priorities with the trainer's loss
        weights). That needs policy_target="full", whose loss takes the weights and returns the
        rows: ValueError otherwise. The loss dict then gains "train/is_weight_mean" (the mean
        importance weight of the drawn rows) and "train/priority_mean" (the mean priority
        written, over the rows that had one). priority_beta is ignored by any other buffer.
        With ownership_coef > 0 the buffer is a ReplayBuffer(ownership=True) (ValueError
        otherwise, and for such a buffer with ownership_coef = 0, whose sample has two outputs
        more): every step also draws the rows' ownership targets and adds the head's loss on them
        (train_step's `ownership`), under the importance weights where there are any.
        score_coef > 0 needs the same buffer, the ring that holds the final positions (the two
        coefficients are independent: the buffer goes with either being positive), and every
        step adds the score head's loss on the drawn rows' margins (train_step's `margin`)."""
        prioritized = bool(getattr(buffer, "prioritized", False))
        own, score = self.ownership_coef > 0.0, self.score_coef > 0.0
        final = own or score                             # the draw has ownership and margin
        if final != bool(getattr(buffer, "ownership", False)):
            raise ValueError("train_replay: ownership_coef > 0 or score_coef > 0 goes with a "
                             "ReplayBuffer(ownership=True), and both 0 with one without")
        if prioritized and self.policy_target != "full":
            raise ValueError("train_replay: a ReplayBuffer(prioritized=True) needs "
                             "policy_target='full' (the importance weights and the loss rows "
                             "are the full policy loss's)")
        rank, world = self.rank_world()
        steps = self._min_steps(int(steps))
        keys = self._loss_keys + (("train/is_weight_mean", "train/priority_mean") if prioritized
                                  else ())
        tot = torch.zeros(len(keys), dtype=torch.float64, device=self.device)
        with_prob = {"with_prob": True} if prioritized else {}
        for s in range(steps):
            b = _drawn(buffer.sample(self.batch_size, seed * world + rank, s, symmetries,
                                     **with_prob), prioritized, final)
            weights, extras = (), ({"ownership": b["ownership"]} if own else {})
            if score:
                extras["margin"] = b["margin"]
            if prioritized:
                weights = (buffer.is_weights(b["prob"], b["slot"], priority_beta),)
                extras["rows"] = True
            losses = self.train_step(b["states"], b["policy"], b["value"], *weights, **extras)
            priority = None
            if prioritized:     # the step's loss rows are the drawn rows' new priorities
                written, state = buffer.update_priorities(b["slot"], self.last_stats["rows"],
                                                          self.wp, self.wv)
                valid = (state >= 0).sum().clamp(min=1)
                priority = torch.stack([weights[0].double().mean(),
                                        written.double().sum() / valid])
            tot += self._step_totals(losses, priority)
        tot /= max(1, steps)
        return self._loss_dict(keys, self._rank_mean(tot), steps)
