"""rvz — MI355X-native Reversi self-play engine (env + MCTS hot path of AlphaZero-Reversi).

Drop-in classes mirroring the reference's API (src/game, src/mcts, src/self_play):
    ReversiGame, Board      single-game rules, run in the HIP kernels
    MCTS                    search / get_action_probs / update_with_move
    SelfPlay                generate_games / generate_training_data, games in lockstep
Batched core:
    Engine                  n games + trees resident in HBM, C-ABI of include/rvz.h
    SelfPlayRunner          one ply per call, HIP-graph capturable
    LaneRunner              independent lanes of SelfPlayRunners, one stream each, one graph
    AlphaZeroNetwork, LeafEvaluator   the policy/value net at the evaluation boundary
    solve                   exact endgame values of a batch of positions (rvz_solve)
    solve_window, solve_wld the same within a caller's (alpha, beta) / as win, draw or loss, with
                            optional move ordering (rvz_solve_window)
    solve_moves, solve_moves_wld   the value of every root move (rvz_solve_moves); best_moves
                            reduces them to the proven-optimal moves of each row
    alphabeta               depth-limited heuristic search of a batch of positions (rvz_alphabeta),
                            alphabeta_weights its default evaluation; arena.AlphaBetaPlayer plays it
    board_symmetry, training_rows   the eight board symmetries on bitboards (rvz_board_symmetry)
                            and augmented training rows straight from them (rvz_training_rows);
                            symmetry_compose / symmetry_inverse give the group table
    merge_positions         one training row per distinct position, the mean of the targets of
                            all its occurrences (rvz_merge_positions)
    ReplayBuffer, replay_batch   a ring of compact training records on the device across
                            iterations, and a minibatch drawn from it under random board
                            symmetries in one launch (rvz_replay_batch)
    replay_cdf, replay_batch_weighted   the same draw in proportion to a per-row weight:
                            ReplayBuffer(weighted=True), a table of integer prefix sums
                            (rvz_replay_cdf) and the search through it
                            (rvz_replay_batch_weighted)
    replay_priority, replay_is_weight   prioritized replay: a trained batch's losses written
                            back as the rows' sampling weights (rvz_replay_priority) and the
                            importance weights of a drawn batch (rvz_replay_is_weight):
                            ReplayBuffer(prioritized=True)
    replay_stale, replay_roots, replay_refresh   replay reanalysis: the stalest rows chosen on
                            the device (rvz_replay_stale), ring rows as engine roots
                            (rvz_replay_roots) and the new search's policy rows written over the
                            old targets (rvz_replay_refresh): ReplayBuffer(stamps=True).reanalyse
    records_games           a window of autoreset self-play records cut into finished games:
                            compact rows with value targets, open games held back
                            (rvz_records_games); SelfPlayRunner(carry_plies=...) keeps the window
    records_final, replay_ownership, ownership_loss, full_ownership_loss   the auxiliary
                            final-ownership target: the final position of each record's game
                            (rvz_records_final), a drawn batch's +1 / -1 / 0 targets under its
                            own symmetries (rvz_replay_ownership; ReplayBuffer(ownership=True)),
                            and the deterministic float64 loss of an ownership head
                            (rvz_ownership_loss); AlphaZeroNetwork(ownership_head=True)
    score_loss, full_score_loss, differentiable_score   the auxiliary final-score target: the
                            deterministic float64 loss of a score-distribution head on the final
                            disc margin a ReplayBuffer(ownership=True) returns with every batch
                            (rvz_score_loss); AlphaZeroNetwork(score_head=True)
    openings, opening_suite, opening_index   the distinct positions after d plies under the
                            engine's own rules (rvz_openings), the balanced ones among them, and
                            the pool row a seed picks (rvz_opening_index); Engine.openings starts
                            games from such a pool, Arena.play_openings plays a match over one
    policy_value_loss, full_policy_loss   the loss on the full policy target, weighted per row,
                            with its gradients in one deterministic float64 call
                            (rvz_policy_value_loss), and its differentiable torch form
"""
from ._lib import RvzError, load  # noqa: F401
from .engine import (AB_HEUR_MAX, AB_MAX_DEPTH, AB_WIN, SOLVE_ABANDONED,  # noqa: F401
                     SOLVE_NOT_A_MOVE, Engine, action_probs, alphabeta, alphabeta_weights,
                     best_moves, board_apply, board_canonical, board_legal, dirichlet_noise,
                     policy_softmax, solve, solve_moves, solve_moves_wld, solve_window, solve_wld)
from .game import Board, ReversiGame  # noqa: F401
from .loss import (differentiable_score, full_ownership_loss, full_policy_loss,  # noqa: F401
                   full_score_loss, ownership_loss, policy_value_loss, score_loss)
from .mcts import MCTS  # noqa: F401
from .network import (AlphaZeroNetwork, LeafEvaluator, ModuleEvaluator,  # noqa: F401
                      load_reference_state_dict)
from .records import (board_symmetry, merge_positions, opening_index,  # noqa: F401
                      opening_suite, openings, records_final, records_games, replay_batch,
                      replay_batch_weighted, replay_cdf, replay_is_weight, replay_ownership,
                      replay_priority, replay_refresh, replay_roots, replay_stale,
                      symmetry_compose, symmetry_inverse, training_rows)
from .replay import ReplayBuffer  # noqa: F401
from .selfplay import LaneRunner, SelfPlay, SelfPlayRunner  # noqa: F401

__version__ = "0.1.0"
