"""The self-play + training loop of one rank: BASELINE.json config 4 (C4).

Counterpart of ``AlphaZeroPipeline.train``'s iteration (src/trainer/pipeline.py:114-150):
generate self-play games with the current net (``_generate_self_play_data``, :152-246), train on
them (``_train_epoch``, :272-366), repeat. One process per GPU:

* self-play: this rank's ``games`` games from the start position, lockstep on its own engine,
  recorded on the device (``SelfPlayRunner(record=True)``), one ply = one HIP-graph replay;
  global game g of iteration i is seeded ``seed + i * games * world + g`` (games sharded by rank,
  no collective);
* records -> training arrays on the device (``records_to_training``; no host round trip);
  with ``replay_iterations`` they are compact rows appended to a ``ReplayBuffer`` on the device,
  and every training step samples its minibatch from the last iterations' rows;
* training: ``DDPTrainer`` steps; DDP's bucketed gradient all-reduce over RCCL (backend "nccl"
  on ROCm) during backward is the only collective of the loop; then rank 0's BN statistics are
  broadcast and the evaluator re-reads the weights in place (``LeafEvaluator.refresh``), so the
  captured self-play graph evaluates the new net at its next replay.

The reference's evaluation tournament and checkpointing (:128-140) are out of scope.
"""
from __future__ import annotations

import time
from typing import Dict, Optional

import torch
import torch.distributed as dist

from ._lib import is_int, is_number
from .engine import SOLVE_MAX_EMPTIES, Engine
from .network import LeafEvaluator, leaf_evaluator
from .records import records_games
from .replay import ReplayBuffer, check_recency_decay
from .selfplay import SelfPlayRunner
from .trainer import (DDPTrainer, adjudicate, check_ownership_coef, check_policy_target,
                      check_score_coef, games_to_training, records_to_training)


def _check_options(board_size: int, *, fused, exact_policy, adjudicate_empties, symmetries,
                   merge_positions, replay_iterations, policy_target, count_weights,
                   replay_sampling, replay_recency_decay, replay_priority_alpha,
                   replay_priority_beta, continuous_plies, openings, reanalyse_rows,
                   reanalyse_age, ownership_coef, score_coef) -> tuple:
    """SelfPlayTrainer's option rules (its docstring has what each option means): ValueError for
    every refused value or combination, before a model, a device or the library is touched.
    Returns the options it converts, normalised: (ownership_coef, reanalyse_rows, reanalyse_age,
    replay_priority_beta, replay_recency_decay, continuous_plies, exact_policy,
    replay_iterations, adjudicate_empties, score_coef)."""
    def unit(x):
        return is_number(x, 0.0, 1.0)
    ownership_coef = check_ownership_coef(ownership_coef)
    if ownership_coef > 0.0:
        if not replay_iterations or replay_iterations < 1:
            raise ValueError("ownership_coef > 0 needs replay_iterations >= 1: the ownership "
                             "targets are held by the replay buffer")
        if merge_positions:
            raise ValueError("ownership_coef > 0 keeps one final position per row: "
                             "merge_positions must be False")
        if adjudicate_empties:
            raise ValueError("ownership_coef > 0 needs every game played to its end: "
                             "adjudicate_empties must be 0")
    score_coef = check_score_coef(score_coef)
    if score_coef > 0.0:                        # the margin comes with the final position
        if not replay_iterations or replay_iterations < 1:
            raise ValueError("score_coef > 0 needs replay_iterations >= 1: the final positions "
                             "are held by the replay buffer")
        if merge_positions:
            raise ValueError("score_coef > 0 keeps one final position per row: "
                             "merge_positions must be False")
        if adjudicate_empties:
            raise ValueError("score_coef > 0 needs every game played to its end: "
                             "adjudicate_empties must be 0")
    for name, x in (("reanalyse_rows", reanalyse_rows), ("reanalyse_age", reanalyse_age)):
        if not is_int(x) or x < 0:
            raise ValueError(f"{name} must be an int >= 0, not {x!r}")
    if reanalyse_rows and not replay_iterations:
        raise ValueError("reanalyse_rows needs replay_iterations > 0: it refreshes the "
                         "replay buffer's rows")
    if reanalyse_age and not reanalyse_rows:
        raise ValueError("reanalyse_age needs reanalyse_rows > 0")
    if reanalyse_rows and replay_iterations < reanalyse_age + 2:
        raise ValueError("reanalyse_rows needs replay_iterations >= reanalyse_age + 2: a row "
                         "aged reanalyse_age iterations must stay in the window for the next "
                         "iteration's training steps")
    check_policy_target(policy_target, count_weights)
    if count_weights and not merge_positions:
        raise ValueError("count_weights=True needs merge_positions=True (the counts are "
                         "the merged rows' position_counts)")
    if count_weights and replay_iterations:
        raise ValueError("count_weights=True needs replay_iterations=0: the replay ring "
                         "stores no position counts")
    if replay_sampling not in ("uniform", "counts", "priority"):
        raise ValueError("replay_sampling must be 'uniform', 'counts' or 'priority', not "
                         f"{replay_sampling!r}")
    if replay_sampling == "priority" and not replay_iterations:
        raise ValueError("replay_sampling='priority' needs replay_iterations > 0: it is the "
                         "replay buffer's draw")
    if replay_sampling == "priority" and policy_target != "full":
        raise ValueError("replay_sampling='priority' needs policy_target='full': the "
                         "importance weights and the per-row losses are that loss's")
    if replay_sampling != "priority" and (replay_priority_alpha != 0.6 or
                                          replay_priority_beta != 0.4):
        raise ValueError("replay_priority_alpha and replay_priority_beta need "
                         "replay_sampling='priority'")
    if not unit(replay_priority_alpha):
        raise ValueError("replay_priority_alpha must be in [0, 1], not "
                         f"{replay_priority_alpha!r}")
    beta = replay_priority_beta
    if isinstance(beta, (tuple, list)):
        if len(beta) != 3 or not unit(beta[0]) or not unit(beta[1]) or not is_int(beta[2]) or \
                beta[2] < 1:
            raise ValueError("replay_priority_beta must be a float in [0, 1] or (start, end, "
                             f"iterations >= 1) with both ends in [0, 1], not {beta!r}")
        beta = (float(beta[0]), float(beta[1]), int(beta[2]))
    elif not unit(beta):
        raise ValueError("replay_priority_beta must be a float in [0, 1] or (start, end, "
                         f"iterations), not {beta!r}")
    if replay_sampling == "counts" and not replay_iterations:
        raise ValueError("replay_sampling='counts' needs replay_iterations > 0: it is the "
                         "replay buffer's draw")
    if replay_sampling == "counts" and not merge_positions:
        raise ValueError("replay_sampling='counts' needs merge_positions=True (the weights "
                         "are the merged rows' position_counts)")
    check_recency_decay(replay_recency_decay, "replay_recency_decay")
    if replay_recency_decay != 1.0 and not replay_iterations:
        raise ValueError("replay_recency_decay != 1 needs replay_iterations > 0: it ages "
                         "the replay buffer's rows")
    if continuous_plies is not None:
        if not is_int(continuous_plies) or continuous_plies < 1:
            raise ValueError("continuous_plies must be None or an int >= 1, not "
                             f"{continuous_plies!r}")
        if not replay_iterations:
            raise ValueError("continuous_plies needs replay_iterations > 0: its rows are the "
                             "replay buffer's compact records")
        if not fused:
            raise ValueError("continuous_plies needs fused=True: it is one rvz_play launch "
                             "with autoreset")
        if adjudicate_empties:
            raise ValueError("continuous_plies plays every game to its end: "
                             "adjudicate_empties must be 0")
        if symmetries is not None:
            raise ValueError("continuous_plies leaves the symmetry to the replay buffer's "
                             f"draw: symmetries must be None, not {symmetries!r}")
        continuous_plies = int(continuous_plies)
    if openings is not None and adjudicate_empties:
        raise ValueError("openings start games with more than 4 discs, and adjudication's "
                         "stopping ply assumes 4: adjudicate_empties must be 0")
    if openings is not None and not 3 <= len(openings) <= 4:
        raise ValueError("openings is None or (black, white, side[, salt])")
    exact_policy = int(exact_policy)
    if not 0 <= exact_policy <= SOLVE_MAX_EMPTIES:
        raise ValueError(f"exact_policy must be in [0, {SOLVE_MAX_EMPTIES}]")
    if symmetries not in (None, "all", "random"):
        raise ValueError(f"symmetries must be None, 'all' or 'random', not {symmetries!r}")
    replay_iterations = int(replay_iterations)
    if replay_iterations < 0:
        raise ValueError("replay_iterations must be >= 0")
    if replay_iterations and symmetries is not None:
        raise ValueError("replay_iterations > 0 draws a symmetry with every sampled row "
                         f"(replay_symmetries): symmetries must be None, not {symmetries!r}")
    adjudicate_empties, max_plies = int(adjudicate_empties), board_size * board_size - 4
    if adjudicate_empties and not (1 <= adjudicate_empties <= SOLVE_MAX_EMPTIES and
                                   adjudicate_empties < max_plies):
        raise ValueError(f"adjudicate_empties must be 0 or in [1, {SOLVE_MAX_EMPTIES}] and "
                         f"below {max_plies}")
    return (ownership_coef, int(reanalyse_rows), int(reanalyse_age), beta,
            float(replay_recency_decay), continuous_plies, exact_policy, replay_iterations,
            adjudicate_empties, score_coef)


# the 0-d counters of generate()'s data that run_iteration reports (0 where an option is off)
_COUNTERS = ("exact_rows", "exact_unsolved", "exact_policy_rows", "exact_policy_unsolved",
             "adjudicated", "adjudicate_unsolved", "already_over", "symmetry_rows",
             "symmetry_quirk_rows", "merge_rows", "merge_input_rows")


class SelfPlayTrainer:
    def __init__(self, model, games: int, num_simulations: int = 800, batch_size: int = 64,
                 c_puct: float = 1.0, temperature: float = 1.0, seed: int = 42,
                 train_steps: Optional[int] = None, train_batch: int = 64, lr: float = 1e-3,
                 weight_decay: float = 1e-4, gradient_clip: float = 1.0,
                 graph: bool = True, compact_leaves: bool = True, lr_milestones=(),
                 lr_gamma: float = 0.1, memo: bool = True, fused: bool = True,
                 table_slots: Optional[int] = None, table_discs: int = 14,
                 root_noise=None, temperature_schedule=None, exact_endgame: int = 0,
                 exact_node_limit: int = 2 ** 24, exact_wld: bool = False,
                 adjudicate_empties: int = 0, adjudicate_node_limit: int = 2 ** 24,
                 exact_policy: int = 0, symmetries: Optional[str] = None,
                 symmetry_seed: Optional[int] = None, merge_positions: bool = False,
                 replay_iterations: int = 0, replay_capacity: Optional[int] = None,
                 replay_steps: Optional[int] = None, replay_symmetries: bool = True,
                 policy_target: str = "argmax", count_weights: bool = False,
                 replay_sampling: str = "uniform", replay_recency_decay: float = 1.0,
                 replay_priority_alpha: float = 0.6, replay_priority_beta=0.4,
                 continuous_plies: Optional[int] = None, openings=None,
                 reanalyse_rows: int = 0, reanalyse_age: int = 0, ownership_coef: float = 0.0,
                 score_coef: float = 0.0):
        """score_coef: 0 (off: the code and the keys of before) or c > 0: the auxiliary
        final-score target, independent of ownership_coef and under its rules. The model has the
        score head (AlphaZeroNetwork(score_head=True); ValueError otherwise, as DDPTrainer's);
        the data path carries the final positions as it does for ownership_coef > 0 (either
        coefficient asks for them), and every training step adds c times the head's loss on the
        drawn rows' final disc margins (DDPTrainer(score_coef=c), rvz.full_score_loss); the loss
        dict gains "train/score_loss", "train/score_pdf", "train/score_cdf",
        "train/score_abs_error" and "train/score_agreement", and run_iteration
        "ownership_dropped". Self-play does not read the head. ValueError without
        replay_iterations >= 1, with merge_positions or with adjudicate_empties > 0.
        ownership_coef: 0 (off: the code and the keys of before) or c > 0: the auxiliary
        final-ownership target. The model has the ownership head
        (AlphaZeroNetwork(ownership_head=True); ValueError otherwise, as DDPTrainer's); every
        compact row carries the final position of its game from its mover's side
        (records_to_training / games_to_training(ownership=True): rvz.records_final), the replay
        buffer holds it (ReplayBuffer(ownership=True)) and every training step adds c times the
        head's loss on the drawn rows' ownership targets (DDPTrainer(ownership_coef=c)); the loss
        dict gains "train/ownership_loss" and "train/ownership_agreement" and run_iteration
        "ownership_dropped". Self-play does not read the head. It needs replay_iterations >= 1
        (the targets live in the ring), and raises ValueError with merge_positions (a merged row
        has no single final position) or adjudicate_empties > 0 (the final position is never
        played), under the lockstep path and continuous_plies alike.
        reanalyse_rows: 0 (off: the code and the keys of before) or N: replay reanalysis
        (MuZero's Reanalyse in this loop; ReplayBuffer(stamps=True).reanalyse, the
        rvz_replay_stale / rvz_replay_roots / rvz_replay_refresh HIP kernels). After iteration t's
        weight update, up to N of the stalest rows of the replay buffer whose policy target comes
        from iteration t - reanalyse_age or earlier are searched again with the new net, on an
        engine of their own (made once: `games` roots a chunk, the self-play simulation count and
        batch, no root noise, pool or schedule, temperature 1) and their policy targets are
        overwritten in place and stamped t; the value targets stay, the outcome of a game not
        depending on the net. The rows that iteration t + 1's append will drop from the window
        (ReplayBuffer.rows_leaving: those of iteration t - replay_iterations + 1 and earlier) are
        left out of the selection: no training step would read them again. Every refreshed row
        is therefore trained on for at least one more iteration, which needs
        replay_iterations >= reanalyse_age + 2 for any row to qualify (ValueError otherwise).
        The re-search's engine is checked (Engine.check) after every pass. It needs
        replay_iterations > 0, and reanalyse_age needs
        reanalyse_rows > 0, ValueError otherwise. train() then also reports reanalyse/rows (the
        rows rewritten), reanalyse/skipped (selected rows that were not: none is expected),
        reanalyse/policy_kl (the mean over the rewritten rows of KL(new target || old target), the
        old one floored at 1e-8: how far the new net's search has moved from the search that
        played the row) and reanalyse_s (its wall time, device-synchronised; run_iteration's
        train_s does not include it). The ring's sampling weights are not touched
        (ReplayBuffer.reanalyse says what that means for merged and prioritized rows). Whether
        this improves playing strength has not been measured.
        openings: None (off: every game starts from the start position) or (black, white,
        side[, salt]): a pool of start positions (Engine.openings; rvz.opening_suite builds one),
        set before any graph is captured. Every self-play game, in lockstep and with
        continuous_plies alike, starts from the pool row its seed picks (rvz.opening_index); the
        record side needs nothing else, a game's rows and value targets being functions of its
        records alone. ValueError together with adjudicate_empties, whose stopping ply assumes 4
        discs at the start. With a pool on, records_headless_games (continuous_plies) counts the
        emitted games that started from a pool position other than the start position: they are
        whole games, not games whose head was lost.
        continuous_plies: None (off: the keys and bytes of before) or K >= 1: continuous
        self-play, the operating point bench.py measures. An iteration is ONE rvz_play launch of K
        plies with autoreset (a finished game restarts at once with its slot's next seed, so no
        slot idles and the games spread over all move numbers) into the runner's window, behind a
        carry of the C = S*S - 4 plies before it (SelfPlayRunner(carry_plies=C)). A game has at
        most C records, so every game that ends in the new part lies wholly in the window:
        rvz.records_games(emit_from=C) cuts the window into those games' compact rows with their
        value targets (the rvz_records_games HIP kernels; reading the row count is the one host
        synchronisation, as with merging), games_to_training applies exact_endgame, exact_policy
        and merge_positions to them, they are appended to the replay buffer, and the window rolls
        on. The games are started once, at the first iteration, and continued by the later ones;
        train() refreshes the evaluator (new weights, the memo dropped, a new table generation),
        so a game can be played by two successive nets: its early records carry the search
        policies of the older one. The slots' seeds advance by games x world per finished game.
        It needs the fused h2 path and replay_iterations > 0 (the rows are compact), and raises
        ValueError with adjudicate_empties or symmetries. replay_capacity then defaults to
        replay_iterations x games x (C + K), since no iteration yields more; an iteration that
        finds the buffer still empty (K below a game's length, at the start) trains no step.
        run_iteration also reports games_emitted, records_open, records_abandoned and
        records_headless_games from records_games' stats (in this mode alone).
        root_noise: None (off) or (alpha, epsilon[, salt]): Dirichlet noise at the search
        roots of the self-play games (Engine.root_noise), set before any graph is captured.
        temperature_schedule: None (off) or (moves, late): a game's first `moves` moves are chosen
        at `temperature`, the later ones at `late` (Engine.temperature_schedule), set before any
        graph is captured.
        exact_endgame: 0 (off) or N: the value targets of the records with at most N empty squares
        come from the exact endgame solver (records_to_training; rvz_solve abandoning a row after
        exact_node_limit positions), not from the outcome of the game as played. Self-play itself
        is unchanged. exact_wld: those targets by the win / draw / loss solve (rvz.solve_wld), the
        same values from a smaller search.
        exact_policy: 0 (off) or N in [1, 14]: the policy targets of the records with at most N
        empty squares become uniform over the moves the per-move endgame solver proves optimal
        (records_to_training; rvz_solve_moves with exact_node_limit per move, at the window
        (-1, 1) with exact_wld), not the MCTS visit distribution. Independent of exact_endgame;
        with adjudication on, the rows are those of the shortened games.
        adjudicate_empties: 0 (off) or N in [1, 14], N < S*S - 4: endgame adjudication. Self-play
        stops after S*S - 4 - N plies, where every unfinished game holds exactly N empty squares
        (every committed ply places one disc), and each such game's outcome is the win / draw /
        loss solve of that position (rvz.trainer.adjudicate; a game abandoned after
        adjudicate_node_limit positions is dropped from the iteration's data). The last N plies
        are not searched and yield no training rows; every row's value target is the perfect-play
        outcome from the stopping position.
        symmetries: None (off), "all" or "random": board symmetry augmentation of the iteration's
        training rows (records_to_training; the rvz_training_rows HIP kernel), in generate() and
        with adjudication on alike. "all" turns every row into its 8 images and so multiplies the
        memory of the data by 8: about 16 GB for C4's 32,768 games per rank (some 2 M rows of
        1032 B become 16 M). "random" keeps one image per row, at the memory of before: the
        setting meant for large runs. symmetry_seed: the seed of "random"'s draws; None (the
        default) is seed + iteration, spread over ranks as train_epoch spreads its seed
        ((seed + iteration) * world + rank); an int is used as given, every iteration.
        run_iteration reports symmetry_rows and symmetry_quirk_rows (the rows whose third plane,
        the image of the original's legal mask, differs from the engine's own mask of the image).
        merge_positions: True merges the iteration's records into one training row per distinct
        position (records_to_training; the rvz_merge_positions HIP kernels), carrying the mean
        search policy and the mean outcome of all its occurrences and, under "position_counts",
        their number: the start position is one row, not one per game. It runs before
        `symmetries`, in generate() and with adjudication on alike. train_epoch walks the merged
        rows unweighted, so every distinct position is seen once per pass (count_weights weights
        them by their counts). run_iteration reports
        merge_rows and merge_input_rows (0 when off).
        replay_iterations: 0 (off: every iteration trains on its own games alone) or K: a replay
        buffer on the device (rvz.ReplayBuffer) holds the rows of the last K iterations, this
        rank's own, as compact records of 280 B on 8x8 (bitboards, policy, value; generate() then
        returns "mover" and "opponent" in place of "states"), and every training step draws its
        minibatch from all of them (DDPTrainer.train_replay seeded seed + iteration; the
        rvz_replay_batch HIP kernel): a uniform row, under a fresh board symmetry at every draw
        unless replay_symmetries is False. `symmetries` must then be None (ValueError otherwise);
        exact targets, adjudication and merge_positions apply as before. replay_capacity: the
        buffer's rows, default K x games x max_plies (no iteration yields more than games x
        max_plies). replay_steps: the optimizer steps of an iteration, default ceil(the
        iteration's new rows / train_batch), the steps of a pass over them; train_steps caps
        either. run_iteration reports replay_rows (the rows held after the iteration's append)
        and replay_iterations_held (0 when off).
        replay_sampling: "uniform" (the default: every held row is as likely as any other) or
        "counts": every merged row is appended with its position_counts as its sampling weight
        (ReplayBuffer(weighted=True); the rvz_replay_cdf / rvz_replay_batch_weighted HIP
        kernels), so a position is drawn in proportion to the records it stands for: the start
        position as often as if it had not been merged. It needs replay_iterations > 0 and
        merge_positions=True, ValueError otherwise. The sampling then carries the counts, so
        with policy_target="full" every drawn row weighs 1 in the loss. replay_recency_decay: d in
        (0, 1]: a held row's sampling weight is multiplied by d with every newer iteration
        appended, under any replay_sampling; a d other than 1 needs replay_iterations > 0.
        replay_sampling="priority": prioritized replay (Schaul et al. 2016; ReplayBuffer(
        prioritized=True); the rvz_replay_priority / rvz_replay_is_weight HIP kernels). An
        iteration's rows enter the buffer at the running maximum priority, every training step
        draws in proportion to the priorities, weighs each drawn row by its importance weight
        (pmin / prob) ** beta in the loss, and writes the step's per-row losses back as the rows'
        new priorities, so training dwells on the positions the net currently gets most wrong
        with the sampling bias corrected. It needs replay_iterations > 0 and policy_target="full"
        (the weights and the per-row losses are that loss's), ValueError otherwise.
        replay_priority_alpha in [0, 1]: the exponent of the priorities (0: uniform).
        replay_priority_beta: the exponent of the importance weights, a float in [0, 1] or
        (start, end, iterations): linear in the iteration number from start to end over
        `iterations` iterations, then end. run_iteration then also reports
        replay_priority_max, the running maximum priority after the iteration (in this mode
        alone: the other modes' result keeps its keys).
        policy_target: "argmax" (the default: the reference's criterion) or "full": the trainer's
        loss is AlphaZero's own -pi . log p on the whole policy target (DDPTrainer;
        rvz.full_policy_loss, the rvz_policy_value_loss HIP kernels), so a merged row's mean
        search policy and every proven-optimal move of an exact_policy row are trained on, not
        their argmax alone; train() then also reports train/policy_kl and
        train/policy_agreement. count_weights: True weights each merged row by its
        position_counts, the records it stands for; it needs policy_target="full",
        merge_positions=True and no replay buffer (the ring stores no counts), ValueError
        otherwise.
        table_slots: slots of the fused launch's cross-game NN-output table (0: no table;
        None: the next power of two >= 32 x games, within [2^12, 2^22]: 2^20 for C4's 32,768
        games per rank). Each slot is 576 B of granules + a 4-B claim word on 8x8 (48 granules
        on 6x6): 2^20 slots = 608 MB, 2^12 = 2.4 MB."""
        bs = int(getattr(model, "board_size", 8))
        (self.ownership_coef, self.reanalyse_rows, self.reanalyse_age, self.replay_priority_beta,
         self.replay_recency_decay, self.continuous_plies, self.exact_policy,
         self.replay_iterations, self.adjudicate_empties, self.score_coef) = _check_options(
            bs, fused=fused, exact_policy=exact_policy, adjudicate_empties=adjudicate_empties,
            symmetries=symmetries, merge_positions=merge_positions,
            replay_iterations=replay_iterations, policy_target=policy_target,
            count_weights=count_weights, replay_sampling=replay_sampling,
            replay_recency_decay=replay_recency_decay,
            replay_priority_alpha=replay_priority_alpha,
            replay_priority_beta=replay_priority_beta, continuous_plies=continuous_plies,
            openings=openings, reanalyse_rows=reanalyse_rows, reanalyse_age=reanalyse_age,
            ownership_coef=ownership_coef, score_coef=score_coef)
        # the rows carry their games' final positions when either auxiliary target is on
        self.final_positions = self.ownership_coef > 0.0 or self.score_coef > 0.0
        self.model = model.eval()
        self.device = next(model.parameters()).device
        self.distributed = dist.is_available() and dist.is_initialized()
        self.rank, self.world = ((dist.get_rank(), dist.get_world_size()) if self.distributed
                                 else (0, 1))
        self.games, self.seed = int(games), int(seed)
        self.exact_endgame, self.exact_node_limit = int(exact_endgame), int(exact_node_limit)
        self.exact_wld, self.merge_positions = bool(exact_wld), bool(merge_positions)
        self.symmetries, self.replay_sampling = symmetries, replay_sampling
        self.symmetry_seed = None if symmetry_seed is None else int(symmetry_seed)
        self.replay_steps = None if replay_steps is None else int(replay_steps)
        self.replay_symmetries = bool(replay_symmetries)
        self.adjudicate_node_limit = int(adjudicate_node_limit)
        self.train_steps = train_steps
        self.trainer = DDPTrainer(model, lr=lr, weight_decay=weight_decay,
                                  gradient_clip=gradient_clip, batch_size=train_batch,
                                  lr_milestones=lr_milestones, lr_gamma=lr_gamma,
                                  policy_target=policy_target,
                                  count_weights=bool(count_weights),
                                  ownership_coef=self.ownership_coef,
                                  score_coef=self.score_coef)
        # the h2 kernels when they cover the net, else the module itself on the GPU
        # (ModuleEvaluator: pull-style, eager plies; it reads the live module, so refresh() only
        # drops the memo)
        self.evaluator = leaf_evaluator(model, device=self.device)
        h2 = isinstance(self.evaluator, LeafEvaluator)
        self.eng = Engine(games, num_simulations, batch_size, c_puct, board_size=bs,
                          device=self.device, compact_leaves=compact_leaves, memo=memo)
        if root_noise is not None:
            self.eng.root_noise(*root_noise)
        if temperature_schedule is not None:
            self.eng.temperature_schedule(*temperature_schedule)
        if openings is not None:
            self.eng.openings(*openings)
        self.max_plies = bs * bs - 4
        # fused: every game of the iteration in ONE rvz_play launch with device records, the
        # memo's deferred last batch and the cross-game table (a new generation per refresh());
        # else the pull-style ply graph (per-batch launches, records copied per ply)
        self.fused = bool(fused) and h2
        if table_slots is None:
            table_slots = 1 << min(22, max(12, (32 * self.games - 1).bit_length()))
        if self.fused and table_slots:
            self.eng.table(table_slots, table_discs)
        if self.continuous_plies and not self.fused:
            raise ValueError("continuous_plies needs the fused h2 path: the h2 kernels do not "
                             "cover this net")
        # continuous: a window of max_plies carried plies and continuous_plies new ones, the
        # slots restarting with autoreset; a slot's seeds go seed_g, seed_g + games * world, ...
        continuous = ({"autoreset": True, "carry_plies": self.max_plies,
                       "seed_stride": self.games * self.world}
                      if self.continuous_plies else {})
        self.runner = SelfPlayRunner(self.eng, self.evaluator, temperature, record=True,
                                     max_plies=self.continuous_plies or self.max_plies,
                                     seed_base=self.seed + self.rank * self.games,
                                     fused=self.fused, skip_last_eval=self.fused and memo,
                                     **continuous)
        self.graph = bool(graph) and h2
        self.buffer = None
        if self.replay_iterations:
            if replay_capacity is None:
                replay_capacity = self.replay_iterations * self.games * (
                    self.max_plies + (self.continuous_plies or 0))
            draw = {}
            if self.replay_sampling == "priority":
                draw = {"prioritized": True, "priority_alpha": float(replay_priority_alpha)}
            elif self.replay_sampling == "counts" or self.replay_recency_decay != 1.0:
                draw = {"weighted": True}
            if draw:
                draw["recency_decay"] = self.replay_recency_decay
            self.buffer = ReplayBuffer(int(replay_capacity), bs, self.device,
                                       window_iterations=self.replay_iterations, **draw,
                                       stamps=bool(self.reanalyse_rows),
                                       ownership=self.final_positions)
        if self.reanalyse_rows:
            # the re-search's own engine: the plain search, whatever self-play's engine has set
            self.reanalyse_eng = Engine(games, num_simulations, batch_size, c_puct, board_size=bs,
                                        device=self.device, compact_leaves=compact_leaves)
        self.iteration = 0

    def _seeds(self):
        base = self.seed + self.iteration * self.games * self.world + self.rank * self.games
        self.runner.seeds.copy_(torch.arange(self.games, dtype=torch.int64,
                                             device=self.device) + base)

    def _symmetry_args(self) -> dict:
        seed = self.symmetry_seed
        if seed is None:
            seed = (self.seed + self.iteration) * self.world + self.rank
        return {"symmetries": self.symmetries, "symmetry_seed": seed}

    def _record_args(self) -> dict:
        """This iteration's options as records_to_training and games_to_training take them; the
        rows are compact exactly when there is a replay buffer to hold them."""
        return {"exact_endgame": self.exact_endgame, "exact_node_limit": self.exact_node_limit,
                "exact_wld": self.exact_wld, "exact_policy": self.exact_policy,
                **self._symmetry_args(), "merge_positions": self.merge_positions,
                "compact": bool(self.replay_iterations), "ownership": self.final_positions}

    def generate(self) -> Dict[str, torch.Tensor]:
        """One iteration's self-play: every game of this rank from the start to its end.
        Returns the training arrays (states, policy_targets, value_targets) on the device."""
        run = self.runner
        if self.continuous_plies:
            return self._continuous()
        self._seeds()
        run.start()
        plies = self.max_plies - self.adjudicate_empties
        if self.fused:
            run.play_record(plies)              # one launch: whole games, records on the device
        else:
            for k in range(plies):
                if self.graph and run.graph is None and k == 1:
                    run.capture()               # after one eager ply (kernel warm-up)
                run.ply()
        run.check()
        if self.adjudicate_empties:
            return self._adjudicated(plies)
        if not bool(run.post_status[:, 1].all()):
            raise RuntimeError(f"a game is not over after {self.max_plies} plies")
        return records_to_training(run.rec_black, run.rec_white, run.rec_side, run.rec_idx,
                                   run.rec_p, run.post_status, self.eng.board_size,
                                   **self._record_args())

    def _continuous(self) -> Dict[str, torch.Tensor]:
        """generate() with continuous_plies on: one launch of K plies with autoreset behind the
        carry, the games that finished in it as compact training rows, the window rolled on."""
        run, C = self.runner, self.max_plies
        if self.iteration == 0:         # the games start once; later iterations continue them
            self._seeds()
            run.start()
        run.play_record(self.continuous_plies)
        run.check()
        rows = records_games(run.rec_black, run.rec_white, run.rec_side, run.rec_idx, run.rec_p,
                             self.eng.board_size, emit_from=C)
        out = games_to_training(rows, self.eng.board_size, **self._record_args(),
                                window=(run.rec_black, run.rec_white, run.rec_side, run.rec_idx))
        run.roll()
        out["records_stats"] = rows["stats"]
        return out

    def _adjudicated(self, plies: int) -> Dict[str, torch.Tensor]:
        """generate()'s tail with adjudication on: the games stand after `plies` plies."""
        run, eng, N = self.runner, self.eng, self.adjudicate_empties
        black, white, status = eng.get_state()
        bits = torch.arange(64, dtype=torch.int64, device=self.device)
        discs = (((black | white).unsqueeze(1) >> bits) & 1).sum(1)
        live = status[:, 1] == 0
        if bool((live & (discs != eng.board_size ** 2 - N)).any()):
            raise RuntimeError(f"a live game does not hold {N} empty squares after {plies} plies")
        final, keep, stats = adjudicate(black, white, status, eng.board_size,
                                        node_limit=self.adjudicate_node_limit, check_depth=False)
        # a dropped game's plies leave the data: on a copy, the runner's records stay as played
        rec_idx = torch.where(keep.unsqueeze(0), run.rec_idx[:plies],
                              torch.full_like(run.rec_idx[:plies], -2))
        out = records_to_training(run.rec_black[:plies], run.rec_white[:plies],
                                  run.rec_side[:plies], rec_idx, run.rec_p[:plies], final,
                                  eng.board_size, **self._record_args())
        out.update(stats)
        return out

    def priority_beta(self, iteration: Optional[int] = None) -> float:
        """replay_priority_beta at `iteration` (default: the current one)."""
        beta = self.replay_priority_beta
        if not isinstance(beta, tuple):
            return float(beta)
        it = self.iteration if iteration is None else int(iteration)
        start, end, n = beta
        return end if it >= n else start + (end - start) * it / n

    def _append(self, data: Dict[str, torch.Tensor]) -> None:
        """The iteration's compact rows into the replay buffer; with replay_sampling="counts" each
        merged row's position_counts is its sampling weight (with "priority" the buffer gives the
        rows its running maximum priority)."""
        counts = ({"weight": data["position_counts"].to(torch.float32)}
                  if self.replay_sampling == "counts" else {})
        own = ({"final_mover": data["final_mover"], "final_opponent": data["final_opponent"]}
               if "final_mover" in data else {})       # ownership_coef or score_coef > 0
        self.buffer.append(data["mover"], data["opponent"], data["policy_targets"],
                           data["value_targets"], self.iteration, **counts, **own)

    def train(self, data: Dict[str, torch.Tensor]) -> Dict[str, float]:
        """_train_epoch over this iteration's data (each rank walks its own games; DDP averages
        the gradients), then the evaluator picks up the new weights. With a replay buffer the
        iteration's rows are appended to it first and the steps draw from the whole window."""
        if self.buffer is not None:
            self._append(data)
            steps = self.replay_steps
            if steps is None:
                steps = -(-data["mover"].shape[0] // self.trainer.batch_size)
            if self.train_steps is not None:
                steps = min(steps, self.train_steps)
            if self.continuous_plies and len(self.buffer) == 0:
                steps = 0               # no game has finished yet: nothing to draw from
            beta = ({"priority_beta": self.priority_beta()}
                    if self.replay_sampling == "priority" else {})
            out = self.trainer.train_replay(self.buffer, steps, seed=self.seed + self.iteration,
                                            symmetries=self.replay_symmetries, **beta)
        else:
            out = self.trainer.train_epoch(data, seed=self.seed + self.iteration,
                                           max_steps=self.train_steps, local_data=True)
        self.trainer.sync_buffers()
        self.trainer.scheduler_step()          # pipeline.py:131, once per iteration
        self.model.eval()
        self.evaluator.refresh()               # also drops the engine's memo (the old net's outputs)
        if self.reanalyse_rows:
            out.update(self._reanalyse())
        return out

    def _reanalyse(self) -> Dict[str, float]:
        """Up to reanalyse_rows rows stamped iteration - reanalyse_age or earlier, searched again
        with the net train() has just refreshed and stamped with this iteration."""
        dev, t = self.device, self.iteration
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        below = t - self.reanalyse_age + 1
        rows = skipped = 0
        kl = 0.0
        buf = self.buffer
        if below > 0 and len(buf) > buf.rows_leaving(t + 1):
            got = buf.reanalyse(self.reanalyse_eng, self.evaluator, self.reanalyse_rows,
                                max(0, below - 65536), below, t, with_old=True,
                                first=buf.rows_leaving(t + 1))
            self.reanalyse_eng.check()          # the re-search's device error word
            sel = got["slot"] >= 0
            new = buf.policy[got["slot"].clamp(min=0).long()].double()
            old = got["old_policy"].double().clamp(min=1e-8)
            # a row that was not rewritten still holds its old target and adds 0 (but for the floor)
            terms = torch.where(new > 0, new * (new.clamp(min=1e-300).log() - old.log()),
                                torch.zeros_like(new))
            total = (terms.sum(1) * sel).sum()
            rows, skipped = (int(x) for x in got["counts"].tolist())
            skipped -= got["slot"].numel() - int(got["selected"][0].item())   # not the padding
            skipped -= (-got["slot"].numel()) % self.reanalyse_eng.n_games
            kl = float(total.item()) / max(rows, 1)
        torch.cuda.synchronize(dev)
        return {"reanalyse/rows": rows, "reanalyse/skipped": skipped, "reanalyse/policy_kl": kl,
                "reanalyse_s": time.perf_counter() - t0}

    def run_iteration(self) -> Dict[str, float]:
        """generate + train; wall times of both phases (device-synchronised) in the result. With
        continuous_plies it reports records_headless_games (rvz_records_games' out_stats[5]): the
        emitted games whose first record is not the start position. With an opening pool on
        (openings=...) those are the games that started from a pool position other than the
        start position: whole games, not games whose head was lost."""
        dev = self.device
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        steps0 = int(self.runner.steps.item())
        data = self.generate()
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        plies = int(self.runner.steps.item()) - steps0
        out = self.train(data)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        self.iteration += 1
        out.update({"selfplay_s": t1 - t0, "train_s": t2 - t1 - out.get("reanalyse_s", 0.0),
                    "board_steps": plies,
                    "samples": int(data["policy_targets"].shape[0]),
                    **{k: int(data.get(k, 0)) for k in _COUNTERS},
                    "replay_rows": len(self.buffer) if self.buffer is not None else 0,
                    "replay_iterations_held": (len(self.buffer.rows_by_iteration())
                                               if self.buffer is not None else 0)})
        if self.final_positions:
            out["ownership_dropped"] = int(data["ownership_dropped"])
        if self.replay_sampling == "priority":
            out["replay_priority_max"] = self.buffer.max_priority()
        if self.continuous_plies:
            stats = data["records_stats"].tolist()
            out.update({"games_emitted": stats[1], "records_open": stats[2],
                        "records_abandoned": stats[3], "records_headless_games": stats[5]})
        return out
