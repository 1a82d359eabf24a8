/*
 * rvz.h — C-ABI of the MI355X-native Reversi self-play engine (librvz.so, gfx950).
 *
 * The reference (RandomMike1280/AlphaZero-Reversi) has no FFI on this path: its boundary is three
 * duck-typed Python protocols (game / model / MCTS). Each entry point below replaces one piece of
 * that surface; the line each one replaces is cited next to it. The Python host mirror in
 * alphazero-reversi_amd/rvz (ReversiGame, MCTS, SelfPlay) binds these with ctypes
 * (INTEGRATION.md shows the binding a reference maintainer would add).
 *
 * Conventions
 *  - Every array argument is a DEVICE pointer (HBM, e.g. torch.Tensor.data_ptr()) unless the
 *    comment says "host". Work is enqueued on the engine's stream (rvz_set_stream) or on the
 *    stream argument; nothing here synchronises except rvz_sync / rvz_check.
 *  - Squares are row-major: square s <-> (row, col) = (s / S, s % S), bit s of a bitboard
 *    (board.py:49). The policy index S*S is the pass move (-1, -1) (mcts.py:666-667,687-688).
 *  - Game status is int32[4] per game: {side to move 1|2, game_over 0|1, winner -1 (None)|0|1|2,
 *    passed_moves_in_a_row} (board.py:33-37, game.py:20-23).
 *  - Return codes: RVZ_OK (0) or a negative RVZ_E*; rvz_last_error() explains the last failure.
 *    Game-level illegality is data, not an error: make_move's False is written to out_ok.
 *  - One engine per device per process; not re-entrant. The caller owns every in/out buffer.
 */
#ifndef RVZ_H
#define RVZ_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RVZ_OK 0
#define RVZ_DONE 1          /* rvz_search_step: every batch of this search has been issued */
#define RVZ_EINVAL (-22)
#define RVZ_ENOMEM (-12)
#define RVZ_EHIP (-5)
#define RVZ_EDEVICE (-71)   /* a kernel raised its device-side error word (rvz_check) */

#define RVZ_LEAF_F32 0      /* leaf planes in float32, exactly game.get_canonical_state() */
#define RVZ_LEAF_BF16 1     /* the same 0/1 planes as bfloat16 (exact) for a bf16 evaluator */

/* Live-row counts of a compacted leaf batch (rvz_search_compact, the n_live argument of
 * rvz_resnet_*_ex): the rows are handed out per stripe of RVZ_LIVE_STRIPE rows (game g draws
 * from stripe g / RVZ_LIVE_STRIPE), one int32 counter per stripe, RVZ_LIVE_PITCH int32 apart;
 * stripe s has its live rows at [s * RVZ_LIVE_STRIPE, s * RVZ_LIVE_STRIPE + n_live[s * PITCH]). */
#define RVZ_LIVE_STRIPE 128
#define RVZ_LIVE_PITCH 16

typedef struct rvz_engine rvz_engine;

typedef struct rvz_config {
    int32_t board_size;       /* 8 (reference; board.py:27-28) or 6 (build-defined variant) */
    int32_t n_games;          /* games owned by this engine (one tree each) */
    int32_t num_simulations;  /* MCTS(num_simulations=800)  mcts.py:197 */
    int32_t batch_size;       /* MCTS(batch_size=64)        mcts.py:198; ceil(sims/batch) <= 64 */
    double c_puct;            /* MCTS(c_puct=1.0)           mcts.py:197 */
    int32_t device;           /* HIP device ordinal */
    int32_t leaf_dtype;       /* RVZ_LEAF_F32 | RVZ_LEAF_BF16 */
} rvz_config;

/* ---- lifetime -------------------------------------------------------------------------- */
/* replaces MCTS.__init__ (mcts.py:197-235) + the per-game ReversiGame() of self_play.py:71 */
int rvz_create(const rvz_config *cfg /* host */, rvz_engine **out /* host */);
void rvz_destroy(rvz_engine *e);
const char *rvz_last_error(const rvz_engine *e);          /* e may be NULL: last create error */
int rvz_set_stream(rvz_engine *e, void *hip_stream);        /* hipStream_t; NULL = default */
int rvz_sync(rvz_engine *e);                                /* hipStreamSynchronize */
/* sync + read/clear the device error word: bit 1 a game's draw stream ran out, 2 node pool, 4 path
 * depth, 8 non-finite NN value or probability, 16 an rvz_play queue wait timed out, 32 a root-noise
 * Gamma sampler ran out of attempts (rvz_search_root_noise / rvz_dirichlet_noise) */
int rvz_check(rvz_engine *e, int32_t *host_err);
int rvz_version(void);

/* ---- env, engine-owned (board.py / game.py over n_games boards in HBM) --------------------- */
/* Reset games to the start position (board.py:25-39) and seed each game's numpy-compatible
 * MT19937 stream with seeds[g] (np.random.seed, the RNG behind mcts.py:684). mask: reset only
 * games with mask[g] != 0 (NULL = all). */
int rvz_env_reset(rvz_engine *e, const uint32_t *seeds, const uint8_t *mask);
/* The self-play loop's per-ply bookkeeping (self_play.py:80-101 with every game slot kept busy):
 * plies[g] += 1 when idx[g] >= 0 (rvz_act committed a move); with reset != 0 a game that is over
 * adds 1 to done[g], takes seeds[g] += stride (int64, in place) and restarts from the start
 * position with np.random.seed(seeds[g] mod 2^32) semantics, as rvz_env_reset. idx: rvz_act's
 * out_idx; plies, done: int64 [n_games] per-game counters (sum them to read totals). */
int rvz_env_autoreset(rvz_engine *e, const int32_t *idx, int64_t *seeds, int64_t stride,
                      int64_t *plies, int64_t *done, int32_t reset);
/* The move-sampling draws of each game (np.random.choice's one random_sample() per move,
 * mcts.py:684): rvz_env_reset fills game g's RVZ_DRAWS values from np.random.seed(seeds[g]);
 * rvz_env_set_draws replaces them with u[g][0..RVZ_DRAWS) (float64, device) and rewinds every
 * game to its first value, so a caller can hand each game its slice of ONE stream — the
 * reference's generate_games draws every game's moves in sequence from the global np.random
 * state (self_play.py:66-101, seeded once at pipeline.py:74-80). rvz_env_draws writes the number
 * of values each game has consumed since then (int32 [n_games]; rvz_act / rvz_play at
 * temperature 0 draw none). A game that would draw more than RVZ_DRAWS sets device error bit 1. */
#define RVZ_DRAWS 64
int rvz_env_set_draws(rvz_engine *e, const double *u);
int rvz_env_draws(rvz_engine *e, int32_t *out_pos);
int rvz_env_get(rvz_engine *e, uint64_t *black, uint64_t *white, int32_t *status);
int rvz_env_set(rvz_engine *e, const uint64_t *black, const uint64_t *white, const int32_t *status);
/* ReversiGame.get_valid_moves (game.py:72-79 -> board.py:70-133) as a bitmask per game */
int rvz_env_legal(rvz_engine *e, uint64_t *out_mask);
/* ReversiGame.make_move (game.py:36-70 -> board.py:135-251); sq[g] = -1 is the pass (-1,-1) */
int rvz_env_apply(rvz_engine *e, const int32_t *sq, int32_t *out_ok);

/* ---- board kernels on caller arrays (stateless; n boards) ------------------------------ */
int rvz_board_legal(int32_t board_size, int32_t n, const uint64_t *black, const uint64_t *white,
                    const int32_t *status, uint64_t *out_mask, void *hip_stream);
int rvz_board_apply(int32_t board_size, int32_t n, uint64_t *black, uint64_t *white,
                    int32_t *status, const int32_t *sq, int32_t *out_ok, void *hip_stream);
/* ReversiGame.get_canonical_state (game.py:131-162): float32 [n, 3, S, S] */
int rvz_board_canonical(int32_t board_size, int32_t n, const uint64_t *black,
                        const uint64_t *white, const int32_t *status, float *out,
                        void *hip_stream);

/* F.softmax(policy_logits, dim=1) of _process_batch (mcts.py:596) over n rows of S*S+1 logits:
 * bitwise the probabilities the expand computes when rvz_search_submit gets logits (is_logits = 1)
 * and inside rvz_play (the same device function). The tests feed the oracle with it. */
int rvz_policy_softmax(int32_t board_size, int32_t n, const float *logits, float *probs,
                       void *hip_stream);

/* ---- search (MCTS.search, mcts.py:322-407, one tree per game, lockstep over games) -------- */
/* New root per live game from the engine's env state (mcts.py:334-341). */
int rvz_search_begin(rvz_engine *e);
/* Issue the next batch (mcts.py:348-392 up to the NN call): traversals, immediate terminal
 * backups, _process_batch pass 1. Writes the leaf planes of game g into row g of leaf_x
 * ([n_games, 3, S, S], leaf_dtype) and need[g] = the number of queued traversal copies that
 * wait for row g (0: row g unused this batch). Returns RVZ_DONE (and does nothing) when the
 * search has issued all ceil(num_simulations / batch_size) batches. */
int rvz_search_step(rvz_engine *e, void *leaf_x, int32_t *need);
/* _process_batch pass 2 (mcts.py:600-623): expand every waiting leaf from policy row g and back
 * up value[g]. policy is [n_games, S*S+1] float32: softmaxed probabilities (is_logits = 0,
 * exactly mcts.py:596's input) or raw logits (is_logits = 1: softmax fused into the kernel).
 * Deferred: the work runs at the head of the next rvz_search_step / rvz_act launch (fused into
 * that kernel) or of rvz_search_visits / rvz_tree_export, so policy and value must stay valid and
 * unmodified on the stream until that call. */
int rvz_search_submit(rvz_engine *e, const float *policy, int32_t is_logits, const float *value);
/* Instead of rvz_search_submit for the LAST batch of a search (after the rvz_search_step that
 * issued it): leave its leaves unevaluated. The evaluation of the last batch feeds only state the
 * discarded tree never reads (the leaf's children priors, W along the path; mcts.py:600-640), so
 * rvz_search_visits / rvz_act then back up the visit counts alone and return exactly the visits,
 * p and move of the evaluated search (tests/test_gpu_search.py::test_skip_last_eval_bit_exact).
 * Needs a search of at least two batches (num_simulations > batch_size; RVZ_EINVAL otherwise:
 * a single batch's leaf is the root, whose expansion the act needs; rvz_play's skip_last_eval
 * is ignored for such searches).
 * Off unless called (one NN call fewer per move; not the reference's call sequence). bench.py's
 * headline uses it by default (--evals table, and --evals lazy: the memo + this, so the skipped
 * evaluation is made later only if a search reaches that position; rvz_play's skip_last_eval is
 * the same; --evals reference turns it off). */
int rvz_search_skip(rvz_engine *e);
/* Compacted leaf batches (on != 0; off by default): rvz_search_step writes the leaves that need an
 * evaluation (need[g] > 0; mcts.py:544-623 evaluates exactly those) to the first rows of their
 * game's stripe of RVZ_LIVE_STRIPE rows, in an unspecified order, and rvz_search_submit reads each
 * game's policy / value from that game's row. The per-stripe counts stay on the device:
 * rvz_search_live_count returns the address of the most recently issued batch's counts (layout
 * above; stable for the engine's life per batch index of a search, so a captured graph may bake
 * it in), for the n_live argument of rvz_resnet_*_ex. An evaluator that ignores them and
 * evaluates all n_games rows gives the same search. Visits, p and moves are identical to the
 * uncompacted search. */
int rvz_search_compact(rvz_engine *e, int32_t on);
const int32_t *rvz_search_live_count(const rvz_engine *e);
/* NN-output memo across consecutive searches (on != 0; off by default). The reference rebuilds
 * the tree at every move (mcts.py:334), so the next search's root — the child the move went to —
 * and often some of its descendants are positions this game's previous search already expanded
 * from an NN evaluation. With the memo on, such a leaf is expanded from that earlier output (the
 * priors of its children and its value, kept in the other half of the node pool) instead of
 * being queued for the evaluator: need[g] = 0 and no leaf row for it. A leaf evaluator's row
 * outputs must depend only on the position (true of rvz_resnet_fwd_h2 and any deterministic
 * per-row net), and the net must not change between the two searches: call
 * rvz_search_memo_reset after new weights. Visits, p and moves are identical to the search
 * without the memo (tests/test_gpu_memo.py); it changes only how many rows are evaluated.
 * The memo needs a second half of the node pool (the previous tree): the first call with on != 0
 * reallocates the pool (device pointers change), so enable it before capturing a graph.
 * The carried links are dropped automatically by rvz_env_reset / rvz_env_autoreset (per game),
 * rvz_env_set, rvz_env_apply, rvz_act without apply and an abandoned search. Not inside a
 * search. */
int rvz_search_memo(rvz_engine *e, int32_t on);
int rvz_search_memo_reset(rvz_engine *e);
/* Dirichlet noise on the priors of a search root's children (AlphaZero's exploration noise; the
 * reference carries dirichlet_alpha / dirichlet_epsilon, config.py:25-26, but no code reads
 * them). Off by default and unless epsilon > 0; with it off every game, counter and output byte is
 * what it is without this call. With it on, wherever a search's ROOT is expanded (from an
 * evaluated row in rvz_search_step / rvz_act / rvz_play, from the memo, from a table hit) each
 * child's prior becomes
 *     P'(s) = fl32( fl32((1 - eps) * P(s)) + fl32(eps * eta(s)) ),  s over the root's legal squares,
 * P the softmaxed prior the expansion writes otherwise, eps = (float)epsilon and 1 - eps =
 * 1.0f - eps (float32, computed once here), the two products and the sum each rounded on their
 * own. Non-root expansions, values, backups, UCB and rvz_act are unchanged; the memo's carried
 * priors and the table's logits stay clean (the mix goes into the root's own copy).
 * eta ~ Dirichlet(alpha, ..., alpha) over the k legal squares (k = 1: eta = 1) is a pure function
 * of (seed32[g], the root's disc count, salt, (float)alpha, the root's legal mask), seed32[g] being
 * the uint32 game g's MT19937 stream was last seeded with (rvz_env_reset, rvz_env_autoreset,
 * rvz_play's autoreset): it does not depend on the launch geometry, the schedule, pull-style or
 * fused play, the memo / table / compaction / gate settings, and it consumes none of the game's
 * move-sampling draws (rvz_env_draws is unaffected). Generator: Philox4x32-10, key (seed32, salt),
 * counter (attempt, square, disc count, 0); Marsaglia-Tsang Gamma in the log domain
 * (csrc/rvz_dirichlet.hip.h). A Gamma rejection loop that ran out of its 64 attempts takes its
 * proposal and sets device error bit 32 (rvz_check).
 * RVZ_EINVAL: alpha <= 0, non-finite or not a positive normal float32 (outside 1e-37 .. 3e38);
 * epsilon outside [0, 1]; inside a search. The setting travels in the kernel arguments: launches issued (or captured into a
 * graph: rvz_play, rvz_search_step, rvz_act) before the call keep the setting they were issued
 * with, so a captured graph replays with the noise setting of its capture; set it before
 * capturing. */
int rvz_search_root_noise(rvz_engine *e, double alpha, double epsilon, uint32_t salt);
/* Stateless, on caller arrays: the eta rows of n roots, by the SAME device function the search
 * uses. legal uint64 [n] (bits >= S*S ignored), seed32 uint32 [n], tag int32 [n] (the root's disc
 * count), out float32 [n][S*S+1] (0 at illegal squares and at the pass index; a row without legal
 * squares is all zeros), out_bits (nullable, 16-byte aligned) uint32 [n][S*S][4]: the attempt-0
 * Philox block of every square. RVZ_EINVAL: board size, n < 0, a bad alpha (as above), a null
 * legal / seed32 / tag / out with n > 0. The call has no engine: an exhausted rejection loop sets
 * a word of the device that the next rvz_check of any engine on that device reports (bit 32). */
int rvz_dirichlet_noise(int32_t board_size, int32_t n, const uint64_t *legal,
                        const uint32_t *seed32, const int32_t *tag, uint32_t salt, double alpha,
                        float *out, uint32_t *out_bits, void *hip_stream);
/* Host int64: the live rows of every evaluated batch of every search completed by rvz_act since
 * compaction was first enabled (0 if never enabled; a batch left by rvz_search_skip is not
 * counted); synchronises the engine stream. */
int rvz_search_rows_total(rvz_engine *e, int64_t *out /* host */);
/* {move: child.visit_count} (mcts.py:406-407) as int32 [n_games, S*S+1] */
int rvz_search_visits(rvz_engine *e, int32_t *out);
/* get_action_probs' tail (mcts.py:656-692) + SelfPlay's make_move (self_play.py:98):
 * p (float64 [n_games, S*S+1]) and the chosen index (int32 [n_games]; S*S = pass, -2 = game
 * already over) per game. Samples with each game's MT19937 stream, or with u[g] when u != NULL
 * (float64 [n_games]; the value np.random.random_sample() would return). apply != 0 then plays
 * the move on the engine's env (ReversiGame.make_move semantics). */
int rvz_act(rvz_engine *e, double temperature, const double *u, int32_t apply, int32_t *out_idx,
            double *out_p);
/* Move-number temperature schedule of the act (AlphaZero samples a game's first moves at tau = 1
 * and plays the rest (near-)greedily; the reference has one temperature for every ply,
 * self_play.py:84). Off by default and whenever from_discs <= 0; with it off every game, counter
 * and output byte is what it is without this call. With it on, a game whose position before the
 * move (the search root) holds at least from_discs discs acts with late_temperature in place of
 * the temperature of the call (rvz_act's argument, rvz_play_args.temperature); a game with fewer
 * discs acts with the call's. Nothing else of get_action_probs' tail changes: the power's fast
 * paths and the correctly rounded power, the pairwise sum, the cdf and searchsorted, the first
 * maximum at temperature 0 are the same code with the game's own temperature. A game acting at
 * temperature 0 draws nothing: its rvz_env_draws count does not advance, and neither u[g] nor its
 * draw buffer is read (the existing rule, per game).
 * Every committed ply places one disc (a pass happens inside make_move), so a game from the start
 * position holds 4 + k discs before its move k + 1: from_discs = 4 + N samples the first N moves
 * at the call's temperature. The game's temperature is a pure function of its position: it does
 * not depend on the launch geometry, pull-style or fused play, the memo / table / compaction /
 * gate / root-noise settings, rvz_play's reset or ply_budget phase, or how the position came
 * about (rvz_env_set included), so games at different move numbers share one launch.
 * RVZ_EINVAL (rvz_last_error set): late_temperature negative or non-finite with from_discs > 0;
 * inside a search. The setting travels in the kernel arguments: launches issued (or captured
 * into a graph: rvz_act, rvz_play) before the call keep the setting they were issued with, so a
 * captured graph replays with the schedule of its capture; set it before capturing. */
int rvz_act_schedule(rvz_engine *e, int32_t from_discs, double late_temperature);
/* Stateless, on caller arrays: get_action_probs' tail (mcts.py:656-692) for n independent rows of
 * visit counts, one wave per row, by the SAME device function rvz_act and rvz_play select with.
 * visits int32 [n][S*S+1] (index S*S: the pass; a row's sum must stay below 2^31), temperature
 * float64 [n] (row r's own; 0: the first maximum), u float64 [n] (the value
 * np.random.random_sample() would return; read only by a row that samples). out_idx int32 [n],
 * out_p float64 [n][S*S+1], out_drew (nullable) int32 [n]: 1 if the row consumed u[r] (temperature
 * != 0 and a nonzero row), else 0. For re-deriving move probabilities from exported visit counts
 * (rvz_search_visits) at another temperature. Device pointers; asynchronous on hip_stream.
 * RVZ_EINVAL: board size, n < 0, a null visits / temperature / u / out_idx / out_p with n > 0.
 * The counts are checked in the kernel (no host synchronisation): a row holding a negative count
 * gets out_idx = -3, a zero out_p row and out_drew 0. */
int rvz_action_probs(int32_t board_size, int32_t n, const int32_t *visits,
                     const double *temperature, const double *u, int32_t *out_idx, double *out_p,
                     int32_t *out_drew, void *hip_stream);

/* ---- exact endgame solver ----------------------------------------------------------------
 * Stateless, on caller arrays: the game-theoretic value of n independent positions under the
 * rules the engine plays by (Board.get_valid_moves board.py:70-133 without file masks, the flip
 * walk board.py:196-219, ReversiGame.make_move game.py:36-70 -> board.py:135-251 with its
 * auto-pass and game end, the winner counting discs only, board.py:363-373), by exhaustive
 * negamax with alpha-beta pruning, one position per lane (csrc/rvz_solve.hip):
 *   solve(g) = discs(g.side) - discs(other side) if g is over, else the maximum over g's moves
 *   (the squares of its legal mask in increasing index, or the pass alone when it has none) of
 *   the child made by make_move: solve(child) if the child kept the side (auto-pass), else
 *   -solve(child).
 * black / white uint64 [n], status int32 [n][4] (side, over, winner, passed: rvz_env_get's
 * layout; `passed` counts, a root with passed = 1 and no move ends the game by passing; `winner`
 * is not read). out_score int32 [n]: solve(row), the final disc difference from the row's side to
 * move (no bonus for empty squares). out_move int32 [n]: the lowest square index among the root
 * moves that reach out_score; S*S when the root's only move is the pass; or, with out_score 0
 * unless noted:
 *   -2  the root is already over (out_score is its disc difference);
 *   -3  more than max_empties empty squares: not searched;
 *   -4  abandoned: the search would have visited more than node_limit positions;
 *   -5  malformed row (black & white overlap, bits at or above S*S, side not 1 | 2), checked in
 *       the kernel (no host synchronisation): not searched.
 * out_nodes (nullable) int64 [n]: the positions visited for the row, the root included (0 for -3
 * and -5, node_limit for -4). Score and move equal the unpruned definition exactly; a row's node
 * count depends on that row and the build alone, not on n, the row's index or its neighbours.
 * max_empties in [0, RVZ_SOLVE_MAX_EMPTIES] (the depth the per-lane LDS stack holds);
 * node_limit > 0 bounds every row's work (there is no unbounded form). Device pointers;
 * asynchronous on hip_stream; graph-capturable (no allocation, no synchronisation). At most 32
 * calls may be executing at once on one device (each takes one of 32 row counters in turn; a
 * captured call keeps the one of its capture).
 * RVZ_EINVAL (before any HIP call): board size not 6 | 8, n < 0, max_empties out of range,
 * node_limit <= 0, a null black / white / status / out_score / out_move with n > 0. n = 0
 * returns RVZ_OK without a launch. */
#define RVZ_SOLVE_MAX_EMPTIES 14
int rvz_solve(int32_t board_size, int32_t n, const uint64_t *black, const uint64_t *white,
              const int32_t *status, int32_t max_empties, int64_t node_limit, int32_t *out_score,
              int32_t *out_move, int64_t *out_nodes, void *hip_stream);
/* rvz_solve with a caller's window and optional move ordering (kernel k_solve_window). Everything
 * not stated here is rvz_solve's: the rules, the row layout, the codes -2 / -3 / -4 / -5 and the
 * in-kernel validation, out_nodes, the launch shape, asynchronous and graph-capturable, and the
 * 32 row counters, which the two calls share (at most 32 calls of either kind executing at once).
 * Let v = rvz_solve's score of the row. out_score = r, fail-soft:
 *   alpha < v < beta: r == v;   v <= alpha: v <= r <= alpha;   v >= beta: beta <= r <= v.
 * So (-1, +1) gives sign(r) == sign(v), the win / draw / loss question, and (-64, 64) gives
 * r == v. A root that is already over reports its exact disc difference and move -2 whatever the
 * window; so do the pass roots that end the game (move S*S).
 * out_move: S*S when the root's only move is the pass; -6 ("fail low: no move reported") when
 * r <= alpha; otherwise a root square whose own exact value m satisfies m == v when r < beta and
 * m >= beta when r >= beta. With order_min_empties == 0 it is the lowest-index such square (for
 * alpha < v < beta that is rvz_solve's move); with ordering on, which qualifying square is
 * reported is unspecified, but a pure function of the row and the build.
 * The root's children are searched with (max(best so far, alpha), beta), a pass root's child
 * with the negated window.
 * order_min_empties = K > 0: at every node with at least K empty squares the next move tried is
 * the untried move whose child leaves the side to move there the fewest legal squares (a child
 * that ends the game or auto-passes counts as 0; ties to the lowest index); below K empties, and
 * everywhere when K == 0, moves are tried in increasing index. Ordering changes which positions
 * are visited, never r's contract above.
 * out_nodes: with order_min_empties == 0, at most rvz_solve's count for the row, for every window
 * (same move order, nested windows: DESIGN.md); with ordering on there is no per-row bound. A
 * row's outputs depend on the row, the arguments and the build alone.
 * RVZ_EINVAL as rvz_solve, and unless -64 <= alpha < beta <= 64 and order_min_empties >= 0. */
int rvz_solve_window(int32_t board_size, int32_t n, const uint64_t *black, const uint64_t *white,
                     const int32_t *status, int32_t max_empties, int64_t node_limit,
                     int32_t alpha, int32_t beta, int32_t order_min_empties,
                     int32_t *out_score, int32_t *out_move, int64_t *out_nodes, void *hip_stream);
/* The value of every root move (kernel k_solve_moves): per row, rvz_solve_window of each child.
 * Everything not stated here is rvz_solve_window's: the rules, the row layout, the in-kernel
 * validation, alpha / beta / order_min_empties, asynchronous and graph-capturable, and the 32 row
 * counters, which the three calls share. out_scores int32 [n][S*S+1], out_count int32 [n],
 * out_nodes (nullable) int64 [n][S*S+1]; index S*S is the pass.
 * A root that is not over and has k >= 1 legal squares: out_count = k, and for each legal square
 * s, with c = make_move(root, s) (auto-pass and game end inside, as everywhere):
 *   c is over: out_scores[s] = the final disc difference from the root's side, out_nodes[s] = 1;
 *   otherwise the entry is rvz_solve_window's answer for c as a row with the same max_empties,
 *   node_limit and order_min_empties: window (alpha, beta) and its score when c kept the root's
 *   side (auto-pass), window (-beta, -alpha) and its score negated when the side changed;
 *   out_nodes[s] is that call's count. A child that call abandons (-4) gives out_scores[s] =
 *   RVZ_SOLVE_ABANDONED with its out_nodes; node_limit bounds every move on its own.
 * So with m the move's exact value in the root's terms every entry r is fail-soft:
 *   alpha < m < beta: r == m;   m <= alpha: m <= r <= alpha;   m >= beta: beta <= r <= m,
 * and min(max(r, alpha), beta) == min(max(m, alpha), beta). Moves share no bounds: each is
 * searched with the caller's whole window. Every other entry of the row, the pass included, is
 * RVZ_SOLVE_NOT_A_MOVE with out_nodes 0.
 * A pass root (not over, no legal square): out_count = 1, entry S*S holds rvz_solve_window's
 * score and nodes for the root itself (RVZ_SOLVE_ABANDONED for its -4), every square is
 * RVZ_SOLVE_NOT_A_MOVE.
 * Row codes in out_count, the whole row RVZ_SOLVE_NOT_A_MOVE with nodes 0: -2 the root is over,
 * -3 more than max_empties empty squares, -5 malformed row.
 * The call writes every element of the three outputs for all n rows (no pre-fill needed), each
 * from exactly one lane. A row's outputs depend on the row, the arguments and the build alone,
 * not on n, the row's index, its neighbours or the launch geometry. The unit of work a lane takes
 * is one root move, so a row's moves are searched side by side.
 * RVZ_EINVAL (before any HIP call) as rvz_solve_window (out_scores and out_count taking the place
 * of out_score and out_move), and when n * (S*S + 1) does not fit in int32. n = 0 returns RVZ_OK
 * without a launch. */
#define RVZ_SOLVE_NOT_A_MOVE (-128)
#define RVZ_SOLVE_ABANDONED (-127)
int rvz_solve_moves(int32_t board_size, int32_t n, const uint64_t *black, const uint64_t *white,
                    const int32_t *status, int32_t max_empties, int64_t node_limit,
                    int32_t alpha, int32_t beta, int32_t order_min_empties, int32_t *out_scores,
                    int32_t *out_count, int64_t *out_nodes, void *hip_stream);

/* ---- depth-limited heuristic search -------------------------------------------------------
 * Stateless, on caller arrays: the value of n independent positions by a negamax that stops
 * `depth` placed discs below the root and scores the frontier with a classical evaluation (a
 * square table plus mobility), one position per lane (csrc/rvz_alphabeta.hip): a fixed,
 * net-independent opponent of adjustable strength. The rules are rvz_solve's: the legal mask
 * without file masks, the flip walk, make_move with its auto-pass and game end, moves in
 * increasing square index. The row layout (black / white uint64 [n], status int32 [n][4]) and
 * the device pointers are rvz_solve's too.
 * With NSQ = S*S, weights int32 [NSQ + 1] on the HOST, and for a position g that is not over,
 * P the mover's discs and O the other side's:
 *   h(g) = sum over squares s of weights[s] * ([s in P] - [s in O])
 *        + weights[NSQ] * (popcount(legal(P, O)) - popcount(legal(O, P)))
 * in integer arithmetic, from the mover's side. For a position that is over, with
 * diff = discs(side to move) - discs(other side):
 *   T(g) = RVZ_AB_WIN + diff when diff > 0, -RVZ_AB_WIN + diff when diff < 0, 0 when diff == 0,
 * so a proven result always outranks a heuristic one. Then
 *   value(g, d) = T(g) if g is over, h(g) if d == 0, else the maximum over g's legal squares s
 *   in increasing index of, with c = make_move(g, s): value(c, d - 1) if c kept g's side
 *   (auto-pass), -value(c, d - 1) otherwise.
 * A ply of depth is one placed disc: an auto-pass inside make_move costs none, and neither does
 * a pass root (not over, the mover without a legal square): its value is -value(child after the
 * pass, d), or T when the pass ends the game (passed = 1, or the other side has no move either),
 * and its move is NSQ.
 * The weights are validated on the host before any HIP call:
 *   sum over s of |weights[s]| + NSQ * |weights[NSQ]| <= RVZ_AB_HEUR_MAX,
 * hence |h| < RVZ_AB_WIN - 64 and every score fits int16. They are read at call time and travel
 * by value in the kernel's arguments: the call allocates nothing, copies nothing and does not
 * synchronise; it is asynchronous on hip_stream and graph-capturable, and a captured call keeps
 * the weights of its capture.
 * out_score int32 [n]: value(row, depth). out_move int32 [n]: the lowest-index root square that
 * reaches out_score; NSQ for a pass root; or a row code, checked in the kernel (no host
 * synchronisation):
 *   -2  the row is already over: out_score = T(row), nodes 1;
 *   -4  abandoned at node_limit: out_score 0, nodes = node_limit (rvz_solve's counting: the
 *       root counts, and so does every committed move, frontier and finished children included);
 *   -5  malformed row (rvz_solve's three checks): out_score 0, nodes 0.
 * There is no -3. out_nodes (nullable) int64 [n]: the positions visited for the row.
 * Score and move equal the unpruned definition exactly (fail-soft alpha-beta, the root's
 * children searched with (best so far, +inf) and compared strictly). A row's three outputs
 * depend on the row, the arguments and the build alone, not on n, the row's index, its
 * neighbours or the launch geometry.
 * At most 32 rvz_alphabeta calls may be executing at once on one device: each takes one of 32
 * row counters in turn (a captured call keeps the one of its capture). The counters are the
 * kernel's own, so rvz_solve* calls and rvz_alphabeta calls never share one.
 * RVZ_EINVAL (before any HIP call): board size not 6 | 8, n < 0, depth outside
 * [1, RVZ_AB_MAX_DEPTH], node_limit <= 0, null weights, the weight bound violated, a null
 * black / white / status / out_score / out_move with n > 0. n = 0 returns RVZ_OK without a
 * launch. */
#define RVZ_AB_MAX_DEPTH 12
#define RVZ_AB_WIN 20000
#define RVZ_AB_HEUR_MAX 16000
int rvz_alphabeta(int32_t board_size, int32_t n, const uint64_t *black, const uint64_t *white,
                  const int32_t *status, int32_t depth, const int32_t *weights /* host */,
                  int64_t node_limit, int32_t *out_score, int32_t *out_move,
                  int64_t *out_nodes /* nullable */, void *hip_stream);

/* ---- board symmetries of training records -------------------------------------------------
 * The eight symmetries of the square board (csrc/rvz_symmetry.hip), for augmenting self-play
 * records: a position, its search policy and its outcome have seven equally valid mirror and
 * rotation images. Numbering, used everywhere: k = 4*f + r with r in [0, 4), f in {0, 1}, and for
 * an [S][S] array x indexed (row, col)
 *   T_k(x) = np.fliplr(np.rot90(x, r)) if f else np.rot90(x, r)        (NumPy is the definition)
 * In coordinates, T_k(x)[i][j] = x[src_k(i, j)] with
 *   k = 0: (i, j)            k = 1: (j, S-1-i)        k = 2: (S-1-i, S-1-j)    k = 3: (S-1-j, i)
 *   k = 4: (i, S-1-j)        k = 5: (S-1-j, S-1-i)    k = 6: (S-1-i, j)        k = 7: (j, i)
 * so T_0 is the identity, T_4 mirrors the columns, T_6 the rows, T_7 is the transpose and T_5 the
 * anti-transpose. A bitboard is the [S][S] 0/1 array with square s = row*S + col at bit s. A
 * policy row of S*S+1 entries transforms its first S*S entries as an [S][S] array; entry S*S, the
 * pass, stays in place.
 * The engine's rules are NOT symmetric: move generation applies no file masks (board.py:102-124),
 * so lines wrap around the board edges, and for some positions legal(T(pos)) != T(legal(pos)).
 * rvz_training_rows defines the third input plane of an image as the IMAGE OF THE ORIGINAL'S legal
 * mask, which keeps every sample consistent with its policy target (mass only where plane 3 is 1),
 * and reports through out_quirk the rows where the engine's own mask of the image position differs.
 * Both entry points are stateless, on caller arrays (device pointers), asynchronous on hip_stream
 * and graph-capturable: no allocation, no copy, no synchronisation, no table in memory. */
/* The images of n boards, one lane per board, transformed in registers (8x8: a transpose by three
 * delta swaps, a bit reversal and a byte swap; 6x6: a bit gather). black / white uint64 [n],
 * sym int32 [n]; out_black[i] / out_white[i] = T_sym[i] of row i's two bitboards. On 6x6 input
 * bits at or above 36 are ignored and no such bit is ever set in an output. out_black / out_white
 * may be exactly black / white (in place); any other overlap is undefined. A sym[i] outside
 * [0, 8) writes 0 to both outputs of that row (checked in the kernel, no host synchronisation).
 * RVZ_EINVAL (before any HIP call): board size not 6 | 8, n < 0, a null pointer with n > 0.
 * n = 0 returns RVZ_OK without a launch. */
int rvz_board_symmetry(int32_t board_size, int32_t n, const uint64_t *black,
                       const uint64_t *white, const int32_t *sym, uint64_t *out_black,
                       uint64_t *out_white, void *hip_stream);
/* Augmented training rows straight from the bitboards, one wavefront per input row, lane = output
 * square; every output byte is written once. black / white uint64 [n], status int32 [n][4] (only
 * the side is read, as rvz_board_canonical), policy float32 [n][S*S+1], sym int32 [n], fan 1 | 8.
 *   fan = 1: output row i is the image of input row i under T_sym[i];
 *   fan = 8: sym is ignored (may be NULL); output row 8*i + k is the image under T_k, so rows
 *            0, 8, 16, ... are the untransformed rows.
 * out_states float32 [n*fan][3][S][S], 16-byte aligned: T applied to each of the three planes
 * rvz_board_canonical writes for the ORIGINAL position (mover, opponent, the engine's legal mask
 * of the original); for k = 0 the bytes are rvz_board_canonical's.
 * out_policy float32 [n*fan][S*S+1]: the permuted row, out[s] = policy[src_k(s)] for s < S*S and
 * out[S*S] = policy[S*S]; the values are moved, never recomputed.
 * out_quirk (nullable) int32 [n*fan]: 1 when the engine's legal mask of the image position (mover
 * T(P), opponent T(O)) differs from the image of the original's mask (the wrap-around quirk), 0
 * when they agree, -1 for a row whose sym is outside [0, 8); that row's states and policy are all
 * zero (fan = 1 only; checked in the kernel, no host synchronisation).
 * Every output element of all n*fan rows is written by exactly one lane (no pre-fill needed). A
 * row's outputs depend on that row and its sym alone, not on n, the row's index or its neighbours.
 * The outputs must not overlap the inputs or each other.
 * RVZ_EINVAL (before any HIP call): board size not 6 | 8, n < 0, fan not 1 | 8,
 * n * fan * (S*S + 1) not fitting in int32, and with n > 0 a null black / white / status / policy /
 * out_states / out_policy, a null sym with fan = 1, or an out_states that is not 16-byte aligned.
 * n = 0 returns RVZ_OK without a launch. */
int rvz_training_rows(int32_t board_size, int32_t n, const uint64_t *black, const uint64_t *white,
                      const int32_t *status, const float *policy,
                      const int32_t *sym /* nullable with fan = 8 */, int32_t fan,
                      float *out_states, float *out_policy, int32_t *out_quirk /* nullable */,
                      void *hip_stream);

/* ---- one training row per distinct position ----------------------------------------------
 * Self-play plays many games at once, so the same position is recorded many times (the start
 * position once per game), each time with another noisy search policy and another outcome.
 * rvz_merge_positions (csrc/rvz_merge.hip) turns n records into one row per distinct position,
 * carrying the mean of the members' targets.
 * Identity: with P the mover's bitboard and O the opponent's (P = side == 1 ? black : white, as
 * rvz_board_canonical), two rows are the same position iff their (P, O) are equal: the network's
 * three input planes are functions of (P, O), and the targets are relative to the mover. A
 * black-to-move row and its colour-swapped white-to-move twin therefore merge. Of status only
 * the side is read.
 * Order: output row j is the j-th distinct position in order of first occurrence; out_first[j] is
 * the lowest input index of its group (strictly increasing in j), out_count[j] its members,
 * out_group[i] the output row of input row i. Rows at and above m = *out_m of out_first,
 * out_count, out_policy and out_value are not written.
 * Sums: fixed point, so that no result depends on the order of the hardware's adds. With
 * q(x) = (int64) rint((double) x * 2^36) (the product is exact), entry e of a group of c members
 * is (float) ((double) sum of q(x_e) / ((double) c * 2^36)), the division and both conversions
 * IEEE round-to-nearest; |sum| < 2^61. A group of one member copies its row's policy and value
 * bit for bit (moved, never recomputed), so merging all-distinct rows is the identity.
 * A row is malformed if black & white != 0, a bit at or above S*S is set, the side is not 1 or 2,
 * a policy entry is outside [0, 1] or the value outside [-1, 1] (NaN fails both): it gets
 * out_group -1, joins no group and is not counted in m (checked in the kernel, no host
 * synchronisation).
 * A row's group and every group's outputs depend on the inputs alone, not on timing, the launch
 * geometry or table_log2. Device pointers, asynchronous on hip_stream, graph-capturable: no
 * allocation, no copy, no memset, no synchronisation; the scratch needs no preparation. Outputs
 * must not overlap the inputs, the scratch or each other.
 * table_log2: 0 for the default hash table (the smallest power of two >= 2n slots), else 2^table_log2
 * slots, which must exceed n (tests force long probe chains with it). The scratch holds the
 * table, five int32 per row and 8 * (S*S + 2) bytes of sums for each of at most n / 2 groups of
 * two or more.
 * The environment variable RVZ_MERGE_HOT=0 (experiments) turns off the per-workgroup LDS
 * pre-reduction of large groups' sums; the results are the same bytes.
 * rvz_merge_scratch_size: the scratch's bytes, non-decreasing in n; negative for bad arguments.
 * RVZ_EINVAL (before any HIP call): board size not 6 | 8, n < 0, n * (S*S + 1) >= 2^31, a
 * table_log2 that is negative, above 30 or gives no more than n slots, and with n > 0 a null
 * pointer or a scratch that is not 16-byte aligned. n = 0 returns RVZ_OK without a launch, and
 * then nothing, *out_m included, is written. */
int64_t rvz_merge_scratch_size(int32_t board_size, int32_t n, int32_t table_log2);
int rvz_merge_positions(int32_t board_size, int32_t n, const uint64_t *black,
                        const uint64_t *white, const int32_t *status /* [n][4] */,
                        const float *policy /* [n][S*S+1] */, const float *value /* [n] */,
                        int32_t table_log2, void *scratch, int32_t *out_m /* [1] */,
                        int32_t *out_first /* [n] */, int32_t *out_count /* [n] */,
                        float *out_policy /* [n][S*S+1] */, float *out_value /* [n] */,
                        int32_t *out_group /* [n] */, void *hip_stream);

/* ---- replay buffer: a minibatch drawn from a ring of compact records ----------------------
 * A sliding window over the last iterations' records, held compactly: a record is its mover
 * bitboard, its opponent bitboard (P = side == 1 ? black : white, as rvz_board_canonical), its
 * policy row and its value, 16 + 4 * (S*S + 1) + 4 bytes (280 B on 8x8, 168 B on 6x6) against the
 * 1028 B (580 B) of its expanded planes and policy. rvz_replay_batch (csrc/rvz_replay.hip) draws
 * nb training rows from such a ring in one launch: a uniform record, a random board symmetry,
 * and the row rvz_training_rows writes for that record under that symmetry. Stateless, on caller
 * arrays (device pointers), asynchronous on hip_stream and graph-capturable: no allocation, no
 * copy, no synchronisation, no table in memory, no host randomness.
 * The ring: mover / opponent uint64 [capacity], policy float32 [capacity][S*S+1], value float32
 * [capacity]. It holds `live` rows (1 <= live <= capacity); logical row i, oldest first, sits in
 * slot (start + i) % capacity. Slots outside the live rows are never read.
 * Output row r, one wavefront per row, lane = output square:
 *   x = Philox4x32-10(key (seed & 0xffffffff, seed >> 32),
 *                     counter (r, step & 0xffffffff, step >> 32, 0))      (Salmon et al., SC'11)
 *   i = idx[r] if idx is given, else (uint32) (((uint64) x.0 * (uint32) live) >> 32): the
 *       multiply-high draw. Every i gets floor(2^32 / live) or one more of the 2^32 words, so its
 *       probability is within 2^-32 of 1 / live: a relative bias of at most live / 2^32.
 *   k = sym[r] if sym is given, else x.1 & 7 if random_sym != 0, else 0.
 * With P, O, the policy row and v read from slot (start + i) % capacity, the row is exactly what
 * rvz_training_rows (fan 1) writes for that record (black = P, white = O, side 1) under T_k:
 * out_states float32 [nb][3][S][S], 16-byte aligned, the images of the three planes of the
 * original position, the third being the image of the original's legal mask; out_policy float32
 * [nb][S*S+1] the permuted policy row, values moved and never recomputed; out_value float32 [nb]
 * = v bit for bit; out_slot int32 [nb] the slot read and out_sym int32 [nb] = k, so that a caller
 * can see which record and which image a drawn row is. There is no quirk output.
 * A given idx[r] outside [0, live) (checked in the kernel, no host synchronisation): that row's
 * states and policy are all zero, out_value[r] = 0, out_slot[r] = -1 and out_sym[r] = -1. A given
 * sym[r] outside [0, 8): the same zero row with out_value[r] = 0 and out_sym[r] = -1; out_slot[r]
 * still reports the slot.
 * Every output element of all nb rows is written by exactly one lane (no pre-fill needed). A
 * row's outputs depend on (the ring's contents, start, live, capacity, seed, step, r, idx[r],
 * sym[r]) alone, not on nb or the launch geometry. Offsets into the ring are 64-bit, so
 * capacity * (S*S + 1) may pass 2^31. The outputs must not overlap the ring or each other.
 * RVZ_EINVAL (before any HIP call): board size not 6 | 8, capacity < 1, live outside
 * [1, capacity], start outside [0, capacity), nb < 0, nb * (S*S + 1) not fitting in int32, and
 * with nb > 0 a null mover / opponent / policy / value / out_states / out_policy / out_value /
 * out_slot / out_sym or an out_states that is not 16-byte aligned. nb = 0 returns RVZ_OK without
 * a launch. */
int rvz_replay_batch(int32_t board_size, int32_t capacity, const uint64_t *mover,
                     const uint64_t *opponent /* [capacity] */,
                     const float *policy /* [capacity][S*S+1] */,
                     const float *value /* [capacity] */, int32_t start, int32_t live, int32_t nb,
                     const int32_t *idx /* [nb], nullable */,
                     const int32_t *sym /* [nb], nullable */, int32_t random_sym, uint64_t seed,
                     uint64_t step, float *out_states /* [nb][3][S][S], 16-byte aligned */,
                     float *out_policy /* [nb][S*S+1] */, float *out_value /* [nb] */,
                     int32_t *out_slot /* [nb] */, int32_t *out_sym /* [nb] */, void *hip_stream);

/* rvz_replay_ownership (csrc/rvz_replay.hip): the ownership targets of a drawn batch. A ring that
 * also holds each row's final position (rvz_records_final's two bitboards, 16 B a row) passes the
 * draw's own out_slot and out_sym; one wavefront per output row, lane = output square. With
 * P = final_mover[slot[r]], O = final_opponent[slot[r]] and x the S x S array that is +1 where P
 * has a disc, -1 where O has one and 0 elsewhere:
 *   out_own[r] = T_sym[r](x), the numbering and direction of rvz_replay_batch's state planes
 *                (T_k(x) = fliplr^f(rot90^r(x)), k = 4f + r, as NumPy defines them)
 *   out_margin[r] = popcount(P) - popcount(O), which is also the sum of out_own[r].
 * A slot[r] outside [0, capacity), a sym[r] outside [0, 8), or a slot whose two bitboards overlap
 * or have a bit at or above S*S: an all-zero row with margin 0 (so rvz_replay_batch's -1 / -1
 * rows give zero rows). Every output element is written by exactly one lane. Stateless,
 * asynchronous on hip_stream, graph-capturable.
 * RVZ_EINVAL (before any HIP call): board size not 6 | 8, capacity < 1, nb < 0, nb * (S*S + 1)
 * not fitting in int32, and with nb > 0 a null pointer. nb = 0 returns RVZ_OK without a launch. */
int rvz_replay_ownership(int32_t board_size, int32_t capacity,
                         const uint64_t *final_mover, const uint64_t *final_opponent, /* [capacity] */
                         int32_t nb, const int32_t *slot, const int32_t *sym,          /* [nb] */
                         float *out_own /* [nb][S*S] */, float *out_margin /* [nb] */,
                         void *hip_stream);

/* ---- weighted replay sampling: rows drawn in proportion to a per-row weight ----------------
 * The ring gains weight float32 [capacity], one sampling weight per slot (a merged position's
 * record count, a recency factor, a priority). rvz_replay_cdf turns the live rows' weights into a
 * table of integer prefix sums, and rvz_replay_batch_weighted is rvz_replay_batch drawing logical
 * row i with probability q_i / total from that table. Both are stateless, on caller arrays
 * (device pointers), asynchronous on hip_stream and graph-capturable: no allocation, no copy, no
 * memset, no synchronisation, no host randomness; the table needs no preparation.
 * Fixed point: q(w) = (uint64) rint((double) w * 2^16) (round half to even). A weight is valid
 * iff it is finite and 0 <= w <= 65536 (-0 is 0); then q <= 2^32, and with live < 2^31 the total
 * stays below 2^63. An invalid weight (NaN, negative, above 65536, infinite) has q = 0: the row is
 * never drawn, and it is counted. Every sum is an integer, so the table's bytes depend neither on
 * the tile nor on the order of the adds.
 * The table, uint64 words, 16-byte aligned, rvz_replay_cdf_size(capacity, tile_log2) bytes
 * (non-decreasing in capacity; negative for capacity < 1 or a bad tile_log2):
 *   [0] total = C[live - 1]      [1] the invalid weights among the live rows
 *   [2] start                    [3] live
 *   [4 + i] C[i] = q_0 + ... + q_i for i < live, q_i the q of the weight in slot
 *           (start + i) % capacity: logical order, oldest first, the ring's wrap handled here
 *   behind that, private scratch of the scan's upper levels.
 * Words [0, 4 + live) are the contract. The scan is tiled and spread over consecutive launches:
 * a workgroup scans its tile into C (a shuffle scan of the 64-bit values within a wavefront, the
 * wavefronts combined through LDS) and writes the tile's total; the totals are scanned the same
 * way, level on level until one tile holds them (three levels for 2^31 rows at the default tile
 * of 2^11 rows); the offsets are added back level by level. No workgroup ever waits on another.
 * tile_log2: 0 for the default tile, else 2^tile_log2 rows per workgroup with tile_log2 in
 * [6, 12] (a test hook: at 6, 64 * 64 + 1 rows reach the third level); the table's contract
 * words do not depend on it.
 * rvz_replay_cdf RVZ_EINVAL (before any HIP call): capacity < 1, live outside [0, capacity],
 * start outside [0, capacity), tile_log2 outside {0} and [6, 12], and with live > 0 a null
 * weight, a null cdf or a cdf that is not 16-byte aligned. live = 0 returns RVZ_OK without a
 * launch, and then nothing is written.
 *
 * rvz_replay_batch_weighted: rvz_replay_batch's arguments and, per output row r, its Philox
 * block x (the same key and counter), its k and its outputs; the logical row is drawn otherwise:
 *   u = word[r] if word is given, else ((uint64) x.2 << 32) | x.3
 *   t = (u * total) >> 64 in 128-bit terms (the multiply-high of two 64-bit words), 0 <= t < total
 *   i = the smallest logical row with C[i] > t. A row with q = 0 has C[i] == C[i - 1] and is
 *       never chosen. Of the 2^64 words, floor(2^64 q_i / total) or one more lead to row i: its
 *       probability is within 2^-64 of q_i / total.
 * A given idx[r] takes the place of the draw, with rvz_replay_batch's handling of an idx outside
 * [0, live); the table is then read for out_prob alone. The draws are NOT those of
 * rvz_replay_batch, not even with all weights equal: that call draws from x.0, this one from
 * x.2 and x.3. Only k (x.1) is shared.
 * out_prob float32 [nb], nullable: (float) ((double) q_i / (double) total) of the row taken
 * (given or drawn) wherever out_slot[r] >= 0, else 0, and 0 with total == 0; a caller forms
 * importance weights from it.
 * Zero rows (states and policy all zero, out_value 0, out_slot -1, out_sym -1, out_prob 0) are
 * written for every row when the table's words [2], [3] differ from the call's start / live (a
 * stale table), and for every row without a given idx when total == 0. Both are checked in the
 * kernel, no host synchronisation.
 * The search reads 64 evenly spaced pivots of the current range per round, one per lane, and one
 * ballot narrows the range 64-fold: 4 rounds at 2^21 rows, 6 at 2^31. The result is defined by
 * the rule above, not by the method.
 * Every output element of all nb rows is written by exactly one lane. A row's outputs depend on
 * (the ring, the table, start, live, capacity, seed, step, r, idx[r], sym[r], word[r]) alone, not
 * on nb or the launch geometry. The outputs must not overlap the ring, the table or each other.
 * RVZ_EINVAL (before any HIP call): as rvz_replay_batch, and with nb > 0 a null cdf or a cdf
 * that is not 16-byte aligned. nb = 0 returns RVZ_OK without a launch. */
int64_t rvz_replay_cdf_size(int32_t capacity, int32_t tile_log2);
int rvz_replay_cdf(int32_t capacity, const float *weight /* [capacity] */, int32_t start,
                   int32_t live, int32_t tile_log2, void *cdf /* 16-byte aligned */,
                   void *hip_stream);
int rvz_replay_batch_weighted(int32_t board_size, int32_t capacity, const uint64_t *mover,
                              const uint64_t *opponent /* [capacity] */,
                              const float *policy /* [capacity][S*S+1] */,
                              const float *value /* [capacity] */,
                              const void *cdf /* rvz_replay_cdf's table */, int32_t start,
                              int32_t live, int32_t nb, const int32_t *idx /* [nb], nullable */,
                              const int32_t *sym /* [nb], nullable */,
                              const uint64_t *word /* [nb], nullable */, int32_t random_sym,
                              uint64_t seed, uint64_t step,
                              float *out_states /* [nb][3][S][S], 16-byte aligned */,
                              float *out_policy /* [nb][S*S+1] */, float *out_value /* [nb] */,
                              int32_t *out_slot /* [nb] */, int32_t *out_sym /* [nb] */,
                              float *out_prob /* [nb], nullable */, void *hip_stream);

/* ---- prioritized replay: importance weights and loss-driven priorities ---------------------
 * The two calls that join rvz_replay_batch_weighted (its out_slot and out_prob) and
 * rvz_policy_value_loss (its out_row) into the prioritized replay of Schaul et al. (2016): the
 * importance weights of a drawn batch, and the batch's losses written back into the ring's weight
 * as the rows' new sampling weights. Both (csrc/rvz_priority.hip) are stateless, on caller arrays
 * (device pointers), asynchronous on hip_stream and graph-capturable: no allocation, no copy, no
 * memset, no synchronisation; the scratch needs no preparation; no workgroup waits on another;
 * every output element is written exactly once; rows are checked in the kernel, no host
 * synchronisation. Neither sees a board: only slots, losses and probabilities.
 * All arithmetic is float64 (IEEE, no contraction); pow is the correctly rounded power
 * (csrc/rvz_pow.hip.h pow_cr, the one k_act uses), so the results are a pure function of the
 * arguments, independent of nb's neighbours and of the launch geometry, and a host reference
 * reproduces them bit for bit.
 *
 * rvz_replay_is_weight: row r is valid iff slot[r] >= 0 and prob[r] is finite and > 0;
 *   pmin = the smallest prob among the valid rows
 *   out_weight[r] = (float) pow((double) pmin / (double) prob[r], beta)   for a valid row, else 0
 *   out_min_prob  = pmin, or 0 with no valid row (then every weight is 0)
 * This is (N P(i))^-beta divided by its maximum over the batch (N cancels): every valid row's
 * weight lies in (0, 1] and the rarest drawn row weighs 1; a zero row of a stale or empty table
 * weighs nothing in the loss. pmin is an integer minimum over the bit patterns of the valid
 * probabilities (positive floats order as their bits), so it depends on no order.
 * rvz_replay_is_weight_scratch_size: the scratch's bytes (16); negative for nb < 0.
 * RVZ_EINVAL (before any HIP call): nb < 0, beta not finite or outside [0, 1], and with nb > 0 a
 * null prob / slot / out_weight / scratch or a scratch that is not 16-byte aligned. nb = 0 returns
 * RVZ_OK without a launch, and then nothing is written.
 *
 * rvz_replay_priority: row[r] = {Lp, Lv, H} is rvz_policy_value_loss's out_row of the batch whose
 * out_slot is slot. Per row r:
 *   k = subtract_entropy ? (Lp - H > 0 ? Lp - H : 0) : Lp
 *       with the flag, the divergence KL(target || net policy): Lp alone never reaches 0 on a
 *       high-entropy target; a divergence that rounding made negative is 0
 *   e = policy_coef * k + value_coef * Lv        two products and one sum, each rounded on its own
 *   valid iff 0 <= slot[r] < capacity, Lp, Lv and H are finite, Lp >= 0, Lv >= 0 and e is finite
 *   p = (float) min(cap, max(floor, pow(e, alpha)))
 * floor >= 2^-16 keeps a written row's fixed-point weight in rvz_replay_cdf above 0, so it can be
 * drawn again; alpha = 0 writes pow = 1 everywhere (uniform sampling).
 * weight (the ring's per-slot weights, in/out) becomes what the sequential loop
 *   for r in 0 .. nb - 1: if valid(r): weight[slot[r]] = p_r
 * leaves: of the valid rows that name one slot (a batch is drawn with replacement, and one record
 * can appear under several symmetries with different losses) the one with the highest r wins, and
 * a slot no valid row names keeps its bytes. The result does not depend on timing.
 *   out_state[r]    = 1 for a winner, 0 for a valid row a later one superseded, -1 if invalid
 *   out_priority[r] = p_r for a valid row, else 0
 *   *max_priority   = max(*max_priority, max over the valid rows of p_r), winners or not: a
 *                     running maximum (an integer maximum on the bits of non-negative floats;
 *                     the value held must be one, not NaN)
 * The caller guarantees that no append has overwritten the batch's slots between the draw and
 * this call: the call cannot tell a slot's new tenant from the row that was drawn. The table of
 * prefix sums is not updated: rebuild it with rvz_replay_cdf before the next draw.
 * weight, slot, row, the scratch and the outputs must not overlap.
 * rvz_replay_priority_scratch_size: the scratch's bytes (16 + 4 per row + a hash table of the
 * power of two >= max(2 nb, 64) entries of 8 bytes), non-decreasing in nb; negative for nb < 0 or
 * nb > 2^30.
 * RVZ_EINVAL (before any HIP call): capacity < 1, nb < 0 or nb > 2^30, a coefficient that is
 * negative or not finite, alpha outside [0, 1], floor / cap breaking 2^-16 <= floor <= cap <=
 * 65536, and with nb > 0 a null weight / slot / row / scratch or a scratch that is not 16-byte
 * aligned. nb = 0 returns RVZ_OK without a launch, and then nothing is written. */
int64_t rvz_replay_is_weight_scratch_size(int32_t nb);
int rvz_replay_is_weight(int32_t nb, const float *prob /* [nb] */, const int32_t *slot /* [nb] */,
                         double beta, void *scratch /* 16-byte aligned */,
                         float *out_weight /* [nb] */, float *out_min_prob /* [1], nullable */,
                         void *hip_stream);
int64_t rvz_replay_priority_scratch_size(int32_t nb);
int rvz_replay_priority(int32_t capacity, float *weight /* [capacity], in/out */, int32_t nb,
                        const int32_t *slot /* [nb]: the batch's out_slot */,
                        const double *row /* [nb][3]: rvz_policy_value_loss's out_row */,
                        double policy_coef, double value_coef, int32_t subtract_entropy,
                        double alpha, double floor, double cap,
                        void *scratch /* 16-byte aligned */,
                        float *max_priority /* [1], in/out, nullable */,
                        float *out_priority /* [nb], nullable */,
                        int32_t *out_state /* [nb], nullable */, void *hip_stream);

/* ---- replay reanalysis: stale policy targets refreshed by a new search ----------------------
 * With a window of K iterations the trainer learns from rows whose policy target is the visit
 * distribution of the net that played them, up to K checkpoints ago. The ring stores positions as
 * (mover, opponent) bitboards, so a row can be searched again: MuZero's Reanalyse (Schrittwieser
 * et al., 2020) in an AlphaZero loop. The three calls below (csrc/rvz_reanalyse.hip) are the record
 * side of that loop; the search between the last two is the engine's own (rvz_env_set,
 * rvz_search_*, rvz_act at temperature 1 with apply = 0). The ring gains stamp int32 [capacity]:
 * the iteration whose net produced the slot's policy. The outcome `value` does not depend on the
 * net and is no argument of any of the three: they cannot touch it.
 * All three are stateless, on caller arrays (device pointers), asynchronous on hip_stream and
 * graph-capturable: no allocation, no copy, no memset, no synchronisation; the scratch needs no
 * preparation; no workgroup waits on another (consecutive launches); rows are checked in the
 * kernel, no host synchronisation. Only integer atomics are used and nothing floating-point is
 * reduced across rows, so equal inputs give equal bytes.
 *
 * rvz_replay_stale: the request (n, lo, below), 0 <= lo < below, below - lo <= 65536, over the
 * ring's live rows (capacity, start, live as in rvz_replay_batch; logical row i, oldest first, in
 * slot (start + i) % capacity; slots outside the live rows are never read).
 *   A live row is eligible iff 0 <= stamp < below; its age class is max(stamp - lo, 0), so every
 *   stamp at or below lo shares class 0. A negative stamp is out of range: the row is ineligible
 *   and counted in out_count[1].
 *   The call selects min(n, eligible) rows with the smallest age classes; ties in the last class
 *   taken go to the older logical row (the smaller i).
 *   out_slot int32 [n]: the selected rows' slots in logical-row order, oldest first, then -1 up
 *   to n; every element is written exactly once. out_count int32 [2]: the rows selected, and the
 *   live rows with a stamp out of range.
 * The computation: a class histogram in the scratch (cleared, then integer atomicAdd, once per
 * distinct class of a wavefront, through a histogram per workgroup in LDS up to 2,048 classes); one workgroup scans the classes to the threshold class T and
 * the rows `take` wanted from it; a tiled stable compaction in consecutive launches (tiles of 1,024
 * rows): per-tile counts of the rows below T and of the rows in T, one scan of the pairs, then the
 * write, a selected row going to (rows below T before it) + min(rows of T before it, take).
 * rvz_replay_stale_scratch_size(capacity, classes): the scratch's bytes for a ring of `capacity`
 * slots and classes = below - lo (16 + 4 per class + 8 per tile of the capacity, each part rounded
 * up to 16), non-decreasing in both; negative for capacity < 1 or classes outside [1, 65536].
 * RVZ_EINVAL (before any HIP call): capacity < 1, live outside [1, capacity], start outside
 * [0, capacity), n < 0, lo < 0, below <= lo, below - lo > 65536, and with n > 0 a null stamp /
 * out_slot / out_count / scratch, a scratch that is not 16-byte aligned or scratch_bytes below
 * what the size function reports. n = 0 returns RVZ_OK without a launch, and then nothing is
 * written.
 *
 * rvz_replay_roots: n ring rows as the arrays rvz_env_set takes, one lane per row.
 *   0 <= slot[r] < capacity: out_black[r] = mover[slot], out_white[r] = opponent[slot] and
 *     out_status[r] = {1, 0, -1, 0}: a live game with black to move, no winner, no pass behind
 *     it, as rvz_replay_batch also treats the mover as black.
 *   slot[r] == -1: empty boards and out_status[r] = {1, 1, 0, 0}, a game that is over: the engine
 *     searches nothing for it and rvz_act answers -2.
 *   Any other slot, or a row whose two bitboards overlap or hold a bit at or above S*S: the same
 *     finished row, and one count in out_bad int32 [1] (cleared by the call's first launch).
 * RVZ_EINVAL (before any HIP call): board size not 6 | 8, capacity < 1, n < 0 or n > 2^30, and with
 * n > 0 a null pointer or an out_status that is not 16-byte aligned. n = 0 returns RVZ_OK without a
 * launch.
 *
 * rvz_replay_refresh: the act's rows written over the old targets. slot int32 [n] (what
 * rvz_replay_roots took), p float64 [n][S*S+1] and idx int32 [n]: rvz_act's out_p and out_idx at
 * temperature 1. One wavefront per row. Row r is skipped, and writes nothing, iff
 *   slot[r] is outside [0, capacity) (the -1 padding among them), or idx[r] == -2 (the engine
 *   treated the game as over), or the row holds a negative or non-finite entry, or its float64
 *   sum s has |s - 1| > 1e-9; s is defined as: x_l = p[r][l] for l < min(S*S+1, 64), 0 for the
 *   other l < 64; x_0 += p[r][64] on 8x8; then for d = 32, 16 .. 1: x_l = x_l + x_(l ^ d).
 * A row that is not skipped sums to 1 by construction: it is the act's pairwise sum
 * (rvz_action_probs). policy float32 [capacity][S*S+1] and stamp int32 [capacity] (in/out) become
 * what the sequential loop
 *   for r in 0 .. n - 1: if not skipped(r): policy[slot[r]][j] = (float) p[r][j] for every j
 *                                           stamp[slot[r]] = new_stamp
 * leaves: where several rows name one slot the one with the highest r wins (the slot table of
 * rvz_replay_priority, csrc/rvz_slot_table.hip.h), and a slot no unskipped row names keeps its
 * bytes. The result does not depend on timing. Offsets into the ring are 64-bit.
 *   out_counts int32 [2] (cleared by the call's first launch) = {the slots written, the rows
 *   skipped}; n less both is the rows a later row superseded.
 * The caller guarantees that no append has overwritten the slots since rvz_replay_stale chose
 * them. policy, stamp, slot, p, idx, the scratch and out_counts must not overlap.
 * rvz_replay_refresh_scratch_size(n): the scratch's bytes (4 per row + a hash table of the power
 * of two >= max(2 n, 64) entries of 8 bytes), non-decreasing in n; negative for n < 0 or n > 2^30.
 * RVZ_EINVAL (before any HIP call): board size not 6 | 8, capacity < 1, n < 0 or n > 2^30,
 * new_stamp < 0, and with n > 0 a null policy / stamp / slot / p / idx / out_counts / scratch, a
 * scratch that is not 16-byte aligned or scratch_bytes below what the size function reports.
 * n = 0 returns RVZ_OK without a launch, and then nothing is written.
 *
 * Not done: a value refresh (blending z with the search's root Q: rvz_play's forced searches and
 * its deferred last batch rely on W staying unread), and the fused rvz_play path for the
 * re-search: the pull-style search ships. */
int64_t rvz_replay_stale_scratch_size(int32_t capacity, int32_t classes);
int rvz_replay_stale(int32_t capacity, const int32_t *stamp /* [capacity] */, int32_t start,
                     int32_t live, int32_t n, int32_t lo, int32_t below,
                     void *scratch /* 16-byte aligned */, int64_t scratch_bytes,
                     int32_t *out_slot /* [n] */, int32_t *out_count /* [2] */, void *hip_stream);
int rvz_replay_roots(int32_t board_size, int32_t capacity, const uint64_t *mover,
                     const uint64_t *opponent /* [capacity] */, int32_t n,
                     const int32_t *slot /* [n] */, uint64_t *out_black, uint64_t *out_white,
                     int32_t *out_status /* [n][4], 16-byte aligned */,
                     int32_t *out_bad /* [1] */, void *hip_stream);
int64_t rvz_replay_refresh_scratch_size(int32_t n);
int rvz_replay_refresh(int32_t board_size, int32_t capacity,
                       float *policy /* [capacity][S*S+1], in/out */,
                       int32_t *stamp /* [capacity], in/out */, int32_t n,
                       const int32_t *slot /* [n] */, const double *p /* [n][S*S+1] */,
                       const int32_t *idx /* [n] */, int32_t new_stamp,
                       void *scratch /* 16-byte aligned */, int64_t scratch_bytes,
                       int32_t *out_counts /* [2] */, void *hip_stream);

/* ---- continuous self-play records: a window of autoreset play cut into finished games -------
 * rvz_play with reset = 1 keeps every slot busy: a finished game restarts at once, and a slot's
 * column of the records (rec_black / rec_white / rec_side / rec_p / hist at [ply][game]) holds
 * one game after another. rvz_records_games (csrc/rvz_records.hip) turns a window of such records
 * into the compact rows a replay ring holds: it finds the game boundaries, recovers each finished
 * game's winner by the engine's own rules, gives every record its value target relative to its
 * mover, holds back the games that are still open and compacts the rest. It is stateless, on
 * caller arrays (device pointers), asynchronous on hip_stream and graph-capturable: no
 * allocation, no copy, no memset, no synchronisation; the scratch needs no preparation; no
 * workgroup waits on another (three consecutive launches); every output element below is written
 * exactly once; records are checked in the kernel, no host synchronisation. No atomics and no
 * floating-point arithmetic but one conversion: the outputs are a pure function of the inputs and
 * emit_from, independent of timing and launch geometry.
 *
 * The walk, per slot g, over the plies p = 0 .. plies - 1 in order. There is at most one open
 * segment, and an expected position (black, white, side, and the engine's count of passes in a
 * row) that exists exactly while a segment is open.
 *   rec_idx[p][g] < 0: no record at this ply (a game already over without reset, a ply beyond a
 *     ply_budget, the caller's pre-fill): out_state = -1; the open segment and the expectation
 *     stay as they are.
 *   Otherwise the record is (black, white, side, idx). It is malformed if black & white != 0, a
 *     bit at or above S*S is set, side is not 1 or 2, idx > S*S, or make_move refuses the move:
 *     the make_move of csrc/rvz_rules.hip.h the engine plays by (the wrap-around quirk, the
 *     auto-pass, the game end, set_winner), idx == S*S being the pass. A malformed record gets
 *     out_state = -5, the open segment is abandoned and the expectation cleared.
 *   If a segment is open and (black, white, side) differs from the expectation, the chain is
 *     broken: the open segment is abandoned (every record of it gets out_state = 3) and a new
 *     segment starts at this record.
 *   If no segment is open, one starts here, with no passes in a row behind it; it is headless
 *     iff the record is not the start position with black to move.
 *   The move is applied. If the game is now over, the segment ends at p with winner w (0 draw,
 *     1, 2): for p >= emit_from every record of it is emitted (out_state = 1), for p < emit_from
 *     every record gets out_state = 2 (an earlier window emitted it); no segment is open
 *     afterwards. Otherwise the expectation becomes the position after the move.
 *   After the last ply, the records of a segment still open get out_state = 0.
 * Emitted rows are slot-major: slots in increasing g, within a slot in increasing p (games in
 * order, plies in order). *out_m is their number; rows at and above it are not written. Row j of
 * the record at (p, g), whose segment ended with winner w:
 *   out_src[j]      = p * n_games + g
 *   out_mover[j]    = side == 1 ? black : white, out_opponent[j] the other board
 *   out_policy[j][a] = (float) rec_p[p][g][a]     IEEE round to nearest
 *   out_value[j]    = 0 if w == 0, +1 if w == side, else -1
 * out_stats: [0] emitted rows, [1] emitted games, [2] open records, [3] abandoned records,
 * [4] malformed records, [5] emitted games that are headless, [6] records in state 2, [7] 0.
 * Carry: a game has at most S*S - 4 records (every committed ply places a disc), so a caller that
 * keeps the last C = S*S - 4 plies of a window in front of the next K new ones and passes
 * emit_from = C emits every finished game exactly once, whole.
 * rvz_records_scratch_size: the scratch's bytes (8 + 28 per slot and 8 per record, each part
 * rounded up to 16), non-decreasing in both arguments; negative for plies < 1, n_games < 1 or
 * plies * n_games * 37 >= 2^31.
 * RVZ_EINVAL (before any HIP call): board size not 6 | 8, plies < 1, n_games < 1,
 * plies * n_games * (S*S + 1) >= 2^31, emit_from outside [0, plies], a null pointer other than
 * out_state, or a scratch that is not 16-byte aligned. The inputs, the scratch and the outputs
 * must not overlap. */
int64_t rvz_records_scratch_size(int32_t plies, int32_t n_games);
int rvz_records_games(int32_t board_size, int32_t plies, int32_t n_games,
                      const uint64_t *rec_black, const uint64_t *rec_white, /* [plies][n_games] */
                      const int32_t *rec_side,                              /* [plies][n_games] */
                      const int32_t *rec_idx,   /* [plies][n_games]: rvz_play's hist */
                      const double *rec_p,      /* [plies][n_games][S*S+1] */
                      int32_t emit_from, void *scratch /* 16-byte aligned */,
                      int32_t *out_m /* [1] */,
                      uint64_t *out_mover, uint64_t *out_opponent,  /* [plies*n_games] */
                      float *out_policy /* [plies*n_games][S*S+1] */,
                      float *out_value /* [plies*n_games] */,
                      int32_t *out_src /* [plies*n_games] */,
                      int32_t *out_state /* [plies][n_games], nullable */,
                      int64_t *out_stats /* [8] */, void *hip_stream);

/* rvz_records_final (csrc/rvz_records.hip): the final position of the game a record belongs to,
 * from the mover's side: the ownership target of a training row (who holds every square when the
 * game ends; the sum over the squares is the final disc margin). Stateless, on caller arrays
 * (device pointers), asynchronous on hip_stream and graph-capturable: no allocation, no copy, no
 * memset, no synchronisation, no scratch; two consecutive launches (out_stats zeroed, then a lane
 * per row); every row output of a handled row is written exactly once; out_stats is summed with
 * 64-bit integer atomics, so the outputs are a pure function of the inputs.
 * Rows j < min(n, *count) are handled (count null: j < n; a negative *count: none), so a caller
 * passes rvz_records_games' out_m and out_src straight through without a host read; rows at and
 * above the bound are not written. Row j, with src[j] = p * n_games + g: the walk starts at the
 * record at (p, g) with no passes in a row behind it and goes down column g through the plies p,
 * p + 1, ... A ply whose rec_idx < 0 is skipped. Every other record is checked as
 * rvz_records_games checks it (no overlapping discs, no bit at or above S*S, side 1 | 2,
 * idx <= S*S), every record after the first must equal the position the previous make_move left
 * (black, white and side), and its move is applied with the make_move of csrc/rvz_rules.hip.h
 * (idx == S*S the pass). When the game ends with boards (B, W), for the row's own side:
 *   out_final_mover[j] = side == 1 ? B : W, out_final_opponent[j] the other, out_ok[j] = 1.
 * In every other case the two boards are 0 and out_ok[j] = 0: src[j] outside
 * [0, plies * n_games), rec_idx < 0 at src[j], a malformed record, a refused move, a broken chain
 * (unlike rvz_records_games, no new segment starts), or the window ends with the game still open.
 * out_stats: [0] rows handled, [1] rows with ok = 1, [2] rows whose game is still open at the
 * window's end, [3] every other row with ok = 0. A row costs at most S*S - 4 make_move calls.
 * RVZ_EINVAL (before any HIP call): board size not 6 | 8, plies < 1, n_games < 1,
 * plies * n_games * (S*S + 1) >= 2^31, n < 0, a null record array or out_stats, and with n > 0 a
 * null src or row output. n = 0 returns RVZ_OK without a launch, and then nothing is written. */
int rvz_records_final(int32_t board_size, int32_t plies, int32_t n_games,
                      const uint64_t *rec_black, const uint64_t *rec_white,
                      const int32_t *rec_side, const int32_t *rec_idx,   /* [plies][n_games] */
                      int32_t n, const int32_t *src /* [n] */,
                      const int32_t *count /* [1], nullable, device */,
                      uint64_t *out_final_mover, uint64_t *out_final_opponent, /* [n] */
                      int32_t *out_ok /* [n] */, int64_t *out_stats /* [4] */, void *hip_stream);

/* ---- opening pools: the positions after d plies, and games that start from them --------------
 * rvz_openings (csrc/rvz_openings.hip) enumerates the distinct positions after `plies` plies
 * under the engine's own rules (the make_move of csrc/rvz_rules.hip.h: the wrap-around quirk, the
 * auto-pass, the game end). It is stateless, on caller arrays (device pointers), asynchronous on
 * hip_stream and graph-capturable: no allocation, no copy, no memset, no synchronisation; the
 * scratch needs no preparation; no workgroup waits on another (1 + 5 * plies consecutive
 * launches, each reading the level's size from the scratch, so the host never learns a count);
 * every output element below is written exactly once. Integer atomics only: the outputs are a
 * pure function of (board_size, plies), independent of max_rows (while no level overflows),
 * timing and launch geometry.
 * Level 0 is the start position with black to move. Level k + 1 from level k: for every row of
 * level k in order and every square of its legal mask in increasing index, the child make_move
 * produces. A child that is over is dropped and counted; the others are the level's candidates,
 * in (parent order, square order). Two candidates are the same position iff (black, white, side)
 * are equal; the level keeps each distinct position once, in order of first occurrence.
 * Row j of level `plies`: out_black[j], out_white[j], out_status[j] = {side, 0, -1, 0} (a fresh
 * start with no passes behind it, as rvz_records_games assumes when a segment opens). *out_m is
 * the row count; rows at and above it are not written.
 * out_stats: [0] rows, [1] the last level's candidates before de-duplication, [2] finished
 * children dropped over all levels, [3] candidates removed as duplicates over all levels, [4] the
 * largest level's candidate count, [5..7] 0. Level 0 counts as one candidate.
 * A level with more than max_rows candidates: *out_m = -1 and out_stats[0] = -1 (checked on the
 * device; the later launches are no-ops), out_stats[4] is that level's candidate count, the row
 * outputs are unspecified.
 * rvz_openings_scratch_size: the scratch's bytes (64 + 52 per row + 4 per table slot, the table a
 * power of two >= 2 * max_rows, each part rounded up to 16); negative for bad arguments.
 * RVZ_EINVAL (before any HIP call): board size not 6 | 8, plies < 0 or > S*S - 4, max_rows < 1,
 * max_rows * 4 >= 2^31, a null pointer, or a scratch that is not 16-byte aligned. */
int64_t rvz_openings_scratch_size(int32_t board_size, int32_t max_rows);
int rvz_openings(int32_t board_size, int32_t plies, int32_t max_rows,
                 void *scratch /* 16-byte aligned */, int32_t *out_m /* [1] */,
                 uint64_t *out_black, uint64_t *out_white /* [max_rows] */,
                 int32_t *out_status /* [max_rows][4] */, int64_t *out_stats /* [8] */,
                 void *hip_stream);

/* rvz_env_openings: games start from a pool of n positions (n = 0: off, the copy is freed;
 * nothing set: every game, counter and output byte is what it is without the pool). black /
 * white / side [n] are device pointers; the engine copies them into memory of its own. Like
 * rvz_search_memo it allocates and synchronises: call it before any graph is captured. Every row
 * is checked in a kernel: no overlapping discs, no bit at or above S*S, side 1 | 2, and the mover
 * has at least one legal square; a pool with a bad row is refused with RVZ_EINVAL (the setting
 * stays as it was) and rvz_last_error names the first such row. RVZ_EINVAL also inside a search.
 * The pool, n and salt travel with each launch: launches already issued keep their setting.
 * With a pool on, wherever a game is reset with seed32 = s (rvz_env_reset, rvz_env_autoreset,
 * rvz_play's autoreset), its position becomes pool row i with status {side[i], 0, -1, 0}:
 *   x = Philox4x32-10(key (s, salt), counter (0, 0, 0, 1))      i = (uint32) ((x.0 * n) >> 32)
 * (counter word 3 = 1 keeps the block apart from the root noise's, whose word 3 is 0). Everything
 * else about the reset (the MT19937 seeding, the draws, the carried link, seed32) is unchanged:
 * picking an opening consumes none of the game's draws, and i is a pure function of (s, salt, n).
 * rvz_opening_index: out_index[k] = i for seed32[k], by the same device function; stateless, on
 * device pointers, asynchronous on hip_stream. RVZ_EINVAL: n_pool < 1, n < 0, a null pointer with
 * n > 0; n = 0 returns RVZ_OK without a launch. */
int rvz_env_openings(rvz_engine *e, int32_t n, const uint64_t *black, const uint64_t *white,
                     const int32_t *side /* [n] */, uint32_t salt);
int rvz_opening_index(int32_t n_pool, int32_t n, const uint32_t *seed32 /* [n] */, uint32_t salt,
                      int32_t *out_index /* [n] */, void *hip_stream);

/* ---- policy/value loss on the full policy target -------------------------------------------
 * AlphaZero's own loss, -pi . log p + (y - t)^2, on the whole target distribution (a merged
 * position's mean search policy, the uniform distribution over the proven-optimal moves, a visit
 * distribution) and weighted per row, forward and backward in one call. rvz_policy_value_loss
 * (csrc/rvz_loss.hip) is stateless, on caller arrays (device pointers), asynchronous on
 * hip_stream and graph-capturable: no allocation, no copy, no memset, no synchronisation; the
 * scratch needs no preparation.
 * All arithmetic is float64 (IEEE, no contraction) on the float32 inputs. With z = logits,
 * pi = policy_target, y = value (the net's tanh output), t = value_target, A = S*S + 1, per row r:
 *   m = max_a z[a]                     lse = m + log sum_a exp(z[a] - m)
 *   logp[a] = z[a] - lse               p[a] = exp(logp[a])
 *   S  = sum_a pi[a]
 *   Lp = -sum_{a: pi[a] > 0} pi[a] * logp[a]
 *   H  = -sum_{a: pi[a] > 0} pi[a] * log pi[a]
 *   Lv = (y - t)^2
 *   agree = 1 if the first maximum of z and the first maximum of pi are the same index, else 0
 *   w = weight[r], or 1 with a null weight
 * A row is malformed if a logit or y is not finite, a pi entry is outside [0, 1], t is outside
 * [-1, 1], or its weight is negative or not finite (NaN fails each test): it gets w = 0, a zero
 * out_row, zero gradients, and is counted. Rows are checked in the kernel, no host
 * synchronisation.
 *   W = sum_r w        P = sum_r w Lp / W        V = sum_r w Lv / W
 *   out_loss = { policy_weight * P + value_weight * V, P, V, sum_r w H / W, W,
 *                sum_r w agree / W, malformed rows, 0 }
 *   out_row[r] = { Lp, Lv, H }
 *   grad_logits[r][a] = (float) ((policy_weight * w / W) * (S * p[a] - pi[a]))
 *   grad_value[r]     = (float) ((value_weight * w / W) * 2 * (y - t))
 * the derivatives of out_loss[0] with respect to z and y. With W == 0 every mean and every
 * gradient is 0; no NaN is written anywhere.
 * Sums: a row's sums over a are a fixed float64 butterfly over the wavefront that holds the row
 * (lane = a; on 8x8 lane 0 also carries the pass entry), so out_row[r] depends on row r alone,
 * not on n, r or the neighbours. The cross-row sums are float64 in a fixed tree whose shape
 * depends on n alone: 4096 consecutive rows per node (a thread adds items t, t + 1024, t + 2048,
 * t + 3072, the 64 lanes of a wave by the butterfly, the 16 waves in order), level on level to one
 * node. No floating-point atomics: the same inputs give the same bytes on every call. Every
 * output element is written exactly once; out_row, and the two gradients together, may be null
 * and are then not computed.
 * rvz_loss_scratch_size: the scratch's bytes (64 + 64 per row + the tree's upper levels),
 * non-decreasing in n; negative for bad arguments.
 * RVZ_EINVAL (before any HIP call): board size not 6 | 8, n < 0, n * A >= 2^31, a loss weight
 * that is negative or not finite, and with n > 0 a null logits / value / policy_target /
 * value_target / scratch / out_loss, exactly one of the two gradients, or a scratch that is not
 * 16-byte aligned. n = 0 returns RVZ_OK without a launch, and then nothing is written. */
int64_t rvz_loss_scratch_size(int32_t board_size, int32_t n);
int rvz_policy_value_loss(int32_t board_size, int32_t n, const float *logits /* [n][A] */,
                          const float *value /* [n] */, const float *policy_target /* [n][A] */,
                          const float *value_target /* [n] */,
                          const float *weight /* [n], nullable: every row 1 */,
                          double policy_weight, double value_weight,
                          void *scratch /* 16-byte aligned */, double *out_loss /* [8] */,
                          double *out_row /* [n][3], nullable */,
                          float *grad_logits /* [n][A] */, float *grad_value /* [n] */,
                          void *hip_stream);

/* rvz_ownership_loss (csrc/rvz_loss.hip): the loss of an auxiliary ownership head against
 * rvz_replay_ownership's targets, on rvz_policy_value_loss's row wave (lane = square), cross-row
 * tree and scratch, with its weighting, normalisation, determinism and float64 arithmetic. With
 * o = logits and t = target, both float32 [n][S*S], per row r:
 *   L = (1 / S*S) * sum_a (tanh(o[a]) - t[a])^2
 *   agree = the share of the squares with t[a] != 0 where o[a] has the sign of t[a] (0 for a row
 *           without such a square)
 *   w = weight[r], or 1 with a null weight
 * A row is malformed if a logit is not finite, a target is not -1, 0 or +1, or its weight is
 * negative or not finite: it gets w = 0, a zero out_row, a zero gradient, and is counted.
 *   W = sum_r w
 *   out_loss = { sum_r w L / W, the same, 0, 0, W, sum_r w agree / W, malformed rows, 0 }
 *              (rvz_policy_value_loss's layout: the loss, the first term, no second term, no
 *              entropy)
 *   out_row[r] = { L, agree }
 *   grad_logits[r][a] = (float) ((w / W) * (2 / S*S) * (tanh(o[a]) - t[a]) * (1 - tanh(o[a])^2))
 * With W == 0 every mean and every gradient is 0; no NaN is written anywhere. The same inputs
 * give the same bytes on every call; every output element is written exactly once; out_row and
 * grad_logits may each be null and are then not computed.
 * rvz_ownership_loss_scratch_size: rvz_loss_scratch_size's bytes, non-decreasing in n; negative
 * for bad arguments.
 * RVZ_EINVAL (before any HIP call): board size not 6 | 8, n < 0, n * (S*S + 1) >= 2^31, and with
 * n > 0 a null logits / target / scratch / out_loss or a scratch that is not 16-byte aligned.
 * n = 0 returns RVZ_OK without a launch, and then nothing is written. */
int64_t rvz_ownership_loss_scratch_size(int32_t board_size, int32_t n);
int rvz_ownership_loss(int32_t board_size, int32_t n, const float *logits /* [n][S*S] */,
                       const float *target /* [n][S*S] */,
                       const float *weight /* [n], nullable: every row 1 */,
                       void *scratch /* 16-byte aligned */, double *out_loss /* [8] */,
                       double *out_row /* [n][2], nullable */,
                       float *grad_logits /* [n][S*S], nullable */, void *hip_stream);

/* rvz_score_loss (csrc/rvz_loss.hip): the loss of an auxiliary final-score head against
 * rvz_replay_ownership's out_margin, on rvz_policy_value_loss's cross-row tree and scratch, with
 * its weighting, normalisation, determinism and float64 arithmetic (IEEE, no contraction, on the
 * float32 inputs). The head gives one logit per final disc margin: K = 2 S*S + 1 classes, class k
 * the margin k - S*S from the mover's side. With z = logits and c = (int) margin + S*S, per row r:
 *   m = max_k z[k]                     lse = m + log sum_k exp(z[k] - m)
 *   p[k] = exp(z[k] - lse)
 *   Lpdf = lse - z[c]                  (the difference, not -log p[c]: finite where p[c] underflows)
 *   C[j] = sum_{i <= j} p[i]           T[j] = 1 if j >= c else 0
 *   e[j] = C[j] - T[j]                 for the thresholds j = 0 .. K-2 (e[K-1] is identically 0
 *                                      and is left out)
 *   Lcdf = (1 / (K-1)) * sum_{j <= K-2} e[j]^2
 *   mean = sum_k p[k] * (k - S*S)      abserr = |mean - margin|
 *   agree = 1 if the first maximum of z is c, else 0
 *   w = weight[r], or 1 with a null weight
 * Lpdf is the cross-entropy of the score distribution; Lcdf, the squared distance of the two
 * cumulative distributions, is what tells a miss by 2 discs from a miss by 40.
 * A row is malformed if a logit is not finite, margin is not an integer in [-S*S, S*S], or its
 * weight is negative or not finite (NaN fails each test): it gets w = 0, a zero out_row, a zero
 * gradient, and is counted. Rows are checked in the kernel, no host synchronisation.
 *   W = sum_r w        P = sum_r w Lpdf / W        Q = sum_r w Lcdf / W
 *   out_loss = { pdf_weight * P + cdf_weight * Q, P, Q, sum_r w abserr / W, W,
 *                sum_r w agree / W, malformed rows, 0 }
 *   out_row[r] = { Lpdf, Lcdf, mean, agree }
 *   grad_logits[r][k] = (float) ((w / W) * (pdf_weight * (p[k] - [k == c])
 *                                           + cdf_weight * (2 / (K-1)) * p[k] * (R[k] - Qr)))
 *   R[k] = sum_{j = k}^{K-2} e[j]  (R[K-1] = 0)        Qr = sum_{j <= K-2} e[j] * C[j]
 * the derivative of out_loss[0] with respect to z: dLpdf/dz[k] = p[k] - [k == c] as for any
 * softmax cross-entropy, and with dp[i]/dz[k] = p[i] ([i == k] - p[k]),
 *   dC[j]/dz[k] = sum_{i <= j} p[i] ([i == k] - p[k]) = p[k] ([k <= j] - C[j])
 *   dLcdf/dz[k] = (2 / (K-1)) sum_j e[j] p[k] ([k <= j] - C[j]) = (2 / (K-1)) p[k] (R[k] - Qr).
 * With W == 0 every mean and every gradient is 0; no NaN is written anywhere.
 * Sums: one wavefront holds a row, lane l the CPL = ceil(K / 64) consecutive classes l * CPL ..
 * l * CPL + CPL - 1 (3 a lane on 8x8, 2 on 6x6). C is the lane's own running sum, lowest class
 * first, added to the sum of the lanes below it, which a fixed float64 scan over the lanes' totals
 * gives (steps d = 1, 2, ... 32, lane l adding lane l - d's value); R is the mirror image from the
 * top. A row's scalar sums are the lane's terms added lowest class first, then the float64
 * butterfly of rvz_policy_value_loss. So out_row[r] and grad_logits[r] depend on row r alone
 * (and W), and the cross-row sums are rvz_policy_value_loss's tree. No floating-point atomics: the
 * same inputs give the same bytes on every call. Every output element is written exactly once;
 * out_row and grad_logits may each be null and are then not computed.
 * rvz_score_loss_scratch_size: rvz_loss_scratch_size's bytes, non-decreasing in n; negative for
 * bad arguments (n * K >= 2^31 among them).
 * RVZ_EINVAL (before any HIP call): board size not 6 | 8, n < 0, n * K >= 2^31, a loss weight that
 * is negative or not finite, and with n > 0 a null logits / margin / scratch / out_loss or a
 * scratch that is not 16-byte aligned. n = 0 returns RVZ_OK without a launch, and then nothing is
 * written. */
int64_t rvz_score_loss_scratch_size(int32_t board_size, int32_t n);
int rvz_score_loss(int32_t board_size, int32_t n, const float *logits /* [n][K] */,
                   const float *margin /* [n] */,
                   const float *weight /* [n], nullable: every row 1 */,
                   double pdf_weight, double cdf_weight,
                   void *scratch /* 16-byte aligned */, double *out_loss /* [8] */,
                   double *out_row /* [n][4], nullable */,
                   float *grad_logits /* [n][K], nullable */, void *hip_stream);

/* ---- fused self-play ---------------------------------------------------------------------
 * Replaces SelfPlay.generate_games' ply loop (self_play.py:80-101: MCTS.search + get_action_probs
 * + make_move, mcts.py:322-407 and :642-694) together with its leaf evaluator
 * (AlphaZeroNetwork.predict, network.py:136-158) when the evaluator is the h2 ResNet: ONE launch in
 * which each workgroup plays its own games, every game committing `plies` plies (each a full
 * search of num_simulations), with the per-ply bookkeeping of rvz_env_autoreset. The games, moves,
 * p and counters are bit-identical to the pull-style loop (rvz_search_step / the
 * rvz_resnet_fwd_h2 evaluator with logits / rvz_search_submit / rvz_act / rvz_env_autoreset) on
 * the same engine state; the engine's memo and root-noise settings apply; compaction is inherent (only the live
 * leaves are evaluated). Not inside a search; graph-capturable (no allocation, no sync). */
typedef struct rvz_play_args {
    const float *params;         /* packed fp32 net (rvz_resnet_params_size layout) */
    const uint16_t *blob;        /* its h2 weight blob (rvz_resnet_h2_weights), 16-byte aligned */
    int32_t filters;             /* 64 | 128 (| 256 on board 8) */
    int32_t blocks;              /* residual blocks */
    float *scratch;              /* rvz_play_scratch_size(e) floats, 16-byte aligned */
    float *ovf;                  /* the evaluator's sticky f16-overflow word (set to 1), nullable */
    int32_t plies;               /* plies every game commits in this call, >= 1 */
    int32_t skip_last_eval;      /* each search's last batch unevaluated (rvz_search_skip), and
                                    no row for a search's batches after the first when its root
                                    has at least as many legal moves as there are such batches:
                                    each goes whole to a fresh child (N == 0 scores inf,
                                    mcts.py:96-97), so nothing reads those rows. Same games. */
    int32_t reset;               /* finished games restart (rvz_env_autoreset's reset) */
    int32_t games_per_workgroup; /* > 0: static schedule, each workgroup owns that many games for
                                    every ply; <= 0: task queue, the workgroups draw (group of
                                    -games_per_workgroup games, ply) tasks (0: 4 games) */
    double temperature;
    int64_t *seeds;              /* int64 [n_games], as rvz_env_autoreset */
    int64_t seed_stride;
    int64_t *plies_done;         /* int64 [n_games], += 1 per committed move */
    int64_t *games_done;         /* int64 [n_games], += 1 per finished game (reset != 0) */
    int32_t *out_idx;            /* int32 [n_games]: each game's last act (as rvz_act) */
    double *out_p;               /* float64 [n_games, S*S+1]: its policy vector */
    int32_t *hist;               /* int32 [plies][n_games]: every act's index, nullable */
    int64_t *rows_evaluated;     /* int64 [1] += the leaf rows evaluated by the call, nullable */
    const int32_t *ply_budget;   /* int32 [n_games]: game g commits min(plies, ply_budget[g])
                                    plies in this call (<= 0: none; it is left as it is), nullable
                                    (every game commits `plies`). bench.py staggers the games'
                                    phases with it (game g at ply g mod 60 of its game) */
    int64_t *table_stats;        /* int64 [2] += {table hits, table inserts} (rvz_play_table), nullable */
    /* Self-play records (self_play.py:88-101, the trainer's input; all four or none): for every
     * act of the call, at [p][g] with p = the act's ply within the call, the position before the
     * move (board bitboards and the side to move) and get_action_probs' vector (rec_p float64
     * [plies][n_games][S*S+1]); hist holds the move. out_p is then not written. */
    uint64_t *rec_black;         /* uint64 [plies][n_games], nullable */
    uint64_t *rec_white;
    int32_t *rec_side;           /* int32 [plies][n_games] */
    double *rec_p;
    int64_t *rows_unread;        /* int64 [1] += the rows the call left unread (skip_last_eval: the
                                    child rows of searches whose root has at least as many legal
                                    moves as batches after the first; their last batch's row, which
                                    skip_last_eval defers anyway, is not counted), nullable */
    int32_t skip_forced_roots;   /* with skip_last_eval: a search (of two batches or more) whose root
                                    is not over and has at least as many legal moves as batches
                                    after the first is played whole at its first step: its visit
                                    counts are fixed by the move order alone (batch size on each of
                                    the first children in move order, the remainder on the last), so
                                    the root's own row is left out as well, and no batch walks the
                                    tree. Same games. 0: off (the rows of skip_last_eval alone) */
    int64_t *roots_unread;       /* int64 [1] += the root rows skip_forced_roots left out (forced
                                    searches whose root took no NN output from the memo), nullable;
                                    rows_unread keeps counting the child rows of those searches */
} rvz_play_args;
/* The task queue is a ready schedule: a workgroup takes the least-advanced group whose previous
 * ply is published (one {published | claimed} word per group in the scratch, zeroed per launch),
 * so it waits only when every group with plies left is being played by another workgroup.
 * A task-queue wait that times out (a workgroup that found no ready group while plies were left,
 * bounded spin) sets device error bit 16 (rvz_check): the other workgroups then stop drawing tasks and the
 * launch drains, leaving games at different ply counts. The engine state is then undefined until
 * every game is reset (rvz_env_reset). */
int64_t rvz_play_scratch_size(const rvz_engine *e);
int rvz_play(rvz_engine *e, const rvz_play_args *a);
/* Cross-game NN-output table for rvz_play (off by default; slots = 0 turns it off and frees it).
 * The reference evaluates every leaf (mcts.py:544-623) and carries an inert transposition table
 * for reuse (mcts.py:228-320, 368-385); here, a leaf whose position (mover, opponent, legal-move
 * bitboards: exactly the NN input planes, game.py:131-162) has at most max_discs discs is looked
 * up in a device hash table of `slots` entries (a power of two) before it is queued, and an
 * evaluated row of such a position is stored: a hit expands the leaf from the stored logits and
 * value, which are bitwise what the h2 evaluator returns for that position (its row outputs depend
 * only on the row: tests/test_gpu_network.py), from any earlier evaluation by any game of the
 * engine. Visits, p and moves are identical with and without it (tests/test_gpu_table.py); it
 * changes how many rows are evaluated. Like the memo it requires unchanged weights:
 * rvz_search_memo_reset (new weights in place) starts a new table generation, and so does a call
 * of rvz_play with another weight blob (a kernel on the stream: refused with RVZ_EINVAL while the
 * stream is capturing, so a captured graph never replays it; play once eagerly per evaluator
 * before capturing). 8-byte {datum, generation} granules written and read with agent-scope
 * accesses, so workgroups on every XCD share it without fences. Not inside a search. */
int rvz_play_table(rvz_engine *e, int64_t slots, int32_t max_discs);
/* The per-XCD pass gate of rvz_play's 8x8 forms of 128 and 256 filters (the task-queue schedule).
 * There every trunk pass streams the whole f16-pair weight set (10x128: 11.8 MB), which the
 * workgroups of an XCD, each at its own layer, cannot share through the XCD's 4 MB L2. With the
 * gate a workgroup about to start a pass waits until `fraction` of its XCD's running workgroups
 * have arrived or `timeout_us` has passed since its own arrival, so the XCD's passes start
 * together and read each layer's weights together; a workgroup arriving within `late_us` of the
 * latest round's opening joins that round at once. Timing only: games, moves and counters are
 * identical with any setting (tests/test_gpu_play.py). fraction 0 turns it off; fraction < 0
 * restores the default (0.8, 400 us, 200 us: C3 +8-10% on MI355X, C3's workload at 10x256
 * +10%). The environment
 * variable RVZ_PLAY_GATE="fraction,us[,late_us]" overrides the setting (experiments). */
int rvz_play_gate(rvz_engine *e, double fraction, double timeout_us, double late_us);
/* Ahead rows of rvz_play's 8x8 / 64-filter form (two boards per trunk pass). A pass left with one
 * live board evaluates, in its empty board slot, the row some game of the group will ask for next:
 * the position of the next unvisited child of an expanded root with fewer legal moves than the
 * search has batches after the first, to which the next batch goes whole (mcts.py:96-97). The
 * outputs wait in that game's slot under the position's (mover, opponent, legal-move) bitboards;
 * the search takes them when it queues a leaf with the same key, instead of a row of its own, and
 * the slot is dropped when the game moves. A row's outputs depend only on its position, so games,
 * moves, p and counters are identical with any setting (tests/test_gpu_play_ahead.py); only the
 * passes change. mode 1 (the default): fill empty board slots; 2: also in place of holding an odd
 * row back a cycle; 0: off; < 0: the default. The other forms have no ahead rows. The environment
 * variable RVZ_PLAY_AHEAD overrides the setting (experiments). */
int rvz_play_ahead(rvz_engine *e, int32_t mode);
/* The ahead rows' counters: every later rvz_play adds {ahead rows evaluated, ahead rows a search
 * took} to stats (device int64 [2], kept by the caller; null: not counted, the default).
 * rows_evaluated counts the former among its rows. */
int rvz_play_ahead_stats(rvz_engine *e, int64_t *stats);

/* ---- introspection (tests / bench) -------------------------------------------------------- */
/* Stream-ordered HIP event timer, events without system fence (the engine's own launch timing
 * uses the same): record i / j around launches on a stream, rvz_timer_elapsed synchronises on j
 * and returns the ms between them (host float). Not for stream capture. */
typedef struct rvz_timer rvz_timer;
int rvz_timer_create(int32_t n_events, rvz_timer **out);
int rvz_timer_record(rvz_timer *t, int32_t i, void *hip_stream);
int rvz_timer_elapsed(rvz_timer *t, int32_t i, int32_t j, float *ms /* host */);
void rvz_timer_destroy(rvz_timer *t);

/* Host copy of per-engine counters: [0] search batches issued, [1] kernel launches. */
int rvz_counters(const rvz_engine *e, int64_t *out2 /* host */);
/* Algorithmic-byte counters (bench roofline): while enabled, every search kernel adds the bytes
 * its algorithm must move (nodes scanned, planes/rows written, backups) to a device counter;
 * read returns host int64[3] = {k_step (expand + select), k_act (expand + act), standalone
 * k_expand_backup} since the last enable. Off by default (one atomic per game per launch). */
int rvz_stats_enable(rvz_engine *e, int32_t on);
int rvz_stats_read(rvz_engine *e, int64_t *out3 /* host */);
/* Launch timing (bench roofline): while enabled, every k_step (rvz_search_step) and k_act
 * (rvz_act) launch is bracketed by a pair of HIP events recorded on the engine stream, created with
 * hipEventDisableSystemFence (no cache write-back/invalidate around the timed kernel). read
 * synchronises and returns the mean milliseconds and the launch counts {k_step, k_act}. */
int rvz_timing_enable(rvz_engine *e, int32_t on);
int rvz_timing_read(rvz_engine *e, double *out_ms /* host [2] */, int32_t *out_n /* host [2] */);
/* Tree export for tests: nodes_out [n_games * nodes_per_game] x {int32 N, f32 W, f32 P, f32 C},
 * meta_out [n_games * nodes_per_game] uint32 (device). nodes_per_game = rvz_tree_nodes(). */
int rvz_tree_nodes(const rvz_engine *e);
int rvz_tree_export(rvz_engine *e, void *nodes_out, uint32_t *meta_out);
/* Sizes of the engine's device-resident state, for DESIGN/bench accounting (host out). */
int rvz_footprint(const rvz_engine *e, int64_t *bytes_tree, int64_t *bytes_env);

/* ---- the leaf evaluator (the policy/value net, the boundary's callee) ---- */
/* The reference's AlphaZeroNetwork forward (network.py:30-117, BN folded): x float32
 * [n, 3, board, board] (the leaf planes) -> logits float32 [n, board^2 + 1], value float32 [n].
 * params: the packed fp32 buffer laid out as in csrc/rvz_resnet_common.hip.h
 * (rvz.network.pack_resnet_params), 16-byte aligned, of rvz_resnet_params_size(board, filters,
 * blocks) floats (negative: unsupported shape). filters 64 or 128 (boards 8 and 6) or 256 (board
 * 8; the fused rvz_play too), any block count.
 * work: float scratch of rvz_resnet_work_size(n) elements (the 1x1-conv head outputs handed from
 * the trunk launch to the FC-heads launch, + the overflow word). */
int64_t rvz_resnet_params_size(int32_t board, int32_t filters, int32_t blocks);
int64_t rvz_resnet_work_size(int32_t n);
/* The batched FC heads alone (work -> logits, value; f32 MFMA, fp32 products and sums). */
int rvz_resnet_heads_fc(int32_t board, const float *work, int32_t n, const float *params,
                        int32_t filters, int32_t blocks, float *logits, float *value,
                        void *hip_stream);

/* The forward, fp32 emulated on the f16 MFMA with two parts per operand (the leaf evaluator):
 * x = x0 + x1 (f16 each, 22 significant bits), weights pre-scaled per output channel by a power
 * of two, the three partial products x0w0 + x0w1 + x1w0 accumulated in one fp32
 * accumulator (error of an fp32 GEMM; see csrc/rvz_resnet.hip k_resnet_h2). Boards 8 and 6.
 * blob: rvz_resnet_h2_weights' output (scaled f16 parts + inverse scales, then a range table of
 * {max over output channels of sum |w|, max |bias|} per conv layer, once per parameter update),
 * rvz_resnet_h2_size(filters, blocks) uint16 elements, 16-byte aligned.
 * Activation range: a pass whose unscaled activations reach f16's limit (65520) re-runs the
 * boards that did with their images scaled by a power of two chosen from the range table's
 * bounds (exact; fp32-class relative to the board's largest activation); other boards' outputs
 * are unchanged bit for bit.
 * work: rvz_resnet_work_size(n) floats (16-byte aligned); work[n * 192] (zero it before the first
 * use) is set to 1 (never cleared by the kernel) if a scaled re-run still overflowed (a bound
 * error: the outputs are not valid; no finite net reaches it); words n * 192 + 2, 3 hold the trunk's 64-bit board-unit
 * counter (units dealt to workgroups in start order; any initial value below 2^63). A misaligned
 * work returns RVZ_EINVAL. A workspace must not be shared by launches that can run concurrently
 * (two streams, or one buffer reused across overlapping launches): every launch claims its
 * board units from the counter, and interleaved claims would skip or repeat units silently.
 * Give each stream (each lane) its own workspace. */
int64_t rvz_resnet_h2_size(int32_t filters, int32_t blocks);
int rvz_resnet_h2_weights(const float *params, int32_t filters, int32_t blocks, uint16_t *blob,
                          void *hip_stream);
int rvz_resnet_fwd_h2(int32_t board, const float *x, int32_t n, const float *params,
                      const uint16_t *blob, int32_t filters, int32_t blocks, float *work,
                      float *logits, float *value, void *hip_stream);
int rvz_resnet_trunk_h2(int32_t board, const float *x, int32_t n, const float *params,
                        const uint16_t *blob, int32_t filters, int32_t blocks, float *work,
                        void *hip_stream);
/* Extended forms. n_live (device int32 per-stripe counts as laid out at RVZ_LIVE_STRIPE, nullable):
 * only the live rows of each stripe are evaluated (a compacted leaf batch, rvz_search_compact);
 * workgroups whose boards are all dead exit at once and leave their rows of logits / value / work
 * as they were. The row results do not
 * depend on the row's position in the batch (tests/test_gpu_network.py). stamps (nullable,
 * bench.py): every trunk workgroup w stores the device's 100 MHz wall clock (s_memrealtime) at its
 * start and end in stamps[2w], stamps[2w+1] (uint64 [rvz_resnet_h2_grid(board, filters, n)][2];
 * bits 56-63 of the end stamp: the workgroup's evaluated boards, 0 for a dead workgroup; bits
 * 52-55: the XCD it ran on):
 * max(end) - min(start) is the launch's span, readable after a replayed HIP graph (torch's HIP
 * runtime refuses external event records in stream capture). stamp_ctr (device uint32, nullable):
 * stamps is a ring of `ring` such launch rows and the trunk writes row *stamp_ctr % ring; the
 * heads launch given the same counter advances it by one (one thread, after the trunk is done),
 * so a replayed graph stamps every launch. */
int32_t rvz_resnet_h2_grid(int32_t board, int32_t filters, int32_t n);
int rvz_resnet_fwd_h2_ex(int32_t board, const float *x, int32_t n, const float *params,
                         const uint16_t *blob, int32_t filters, int32_t blocks, float *work,
                         float *logits, float *value, const int32_t *n_live, void *hip_stream);
int rvz_resnet_trunk_h2_ex(int32_t board, const float *x, int32_t n, const float *params,
                           const uint16_t *blob, int32_t filters, int32_t blocks, float *work,
                           const int32_t *n_live, uint64_t *stamps, const uint32_t *stamp_ctr,
                           int32_t ring, void *hip_stream);
int rvz_resnet_heads_fc_ex(int32_t board, const float *work, int32_t n, const float *params,
                           int32_t filters, int32_t blocks, float *logits, float *value,
                           const int32_t *n_live, uint32_t *stamp_ctr, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RVZ_H */
