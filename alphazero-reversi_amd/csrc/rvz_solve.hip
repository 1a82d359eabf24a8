// rvz_solve.hip — exact endgame solver: batched negamax over the reference's rules for gfx950
// (MI355X), exported as rvz_solve, rvz_solve_window and rvz_solve_moves (include/rvz.h). Its own
// translation unit:
// the code objects of rvz_play.hip (k_play) and rvz_engine.hip (k_step, k_act) do not depend on it.
//
// Definition (DESIGN.md §Exact endgame solver): solve(g) = the disc difference at the end of the
// game from g's side to move, both sides playing the maximum, the children made by make_move<BS>
// (auto-pass included), moves in increasing square order, the first maximum kept.
//
// Shape: one position per LANE, persistent lanes that take the next row from a per-call device
// counter, an explicit stack in LDS laid out [depth][field][lane], no scratch: the head of
// rvz_negamax.hip.h has the reasons. That header holds what this file and rvz_alphabeta.hip have
// in common around their loops (geometry, the stack's size, the row counter, the host side of a
// launch), and says why the loops themselves are two texts.
//
// Per lane, in registers: the current node (mover's discs P, the other side's O, the moves not
// yet tried, alpha / beta / best) and the row's bookkeeping. A frame is what the return needs:
// the moves left (2 dwords), the flip mask of the move being searched (2 dwords: the undo), and
// {square, kept-side flag, alpha, beta, best} packed in one dword: 20 bytes.
//
// Depth: every ply places a disc, and a frame is pushed only when the child has a move, i.e. at
// least one empty square left, so a row with E empties pushes at most E - 1 frames;
// FRAMES = RVZ_SOLVE_MAX_EMPTIES covers it with room, and the push checks it all the same.
// LDS: 128 lanes x 14 frames x 20 B = 35,840 B per workgroup: four workgroups (8 waves, 2 per
// SIMD) fit in a CU's 160 KiB.
//
// Pruning: fail-soft alpha-beta. A root's children are searched with the window (best, +inf)
// in the root's terms: a child whose true value is above the root's best so far comes back
// exact, any other comes back <= best and is dropped by the strict comparison, so the score and
// the first-maximum move equal the unpruned definition (DESIGN.md has the argument). Node counts
// depend on the row alone.
//
// One machine, three kernels: solve_rows<BS, MODE> is the loop; k_solve is MODE_FULL,
// k_solve_window MODE_WINDOW and k_solve_moves MODE_MOVES. WIN (both MODE_WINDOW and MODE_MOVES)
// switches three things: the root window (the caller's (walpha, wbeta), negated under a pass
// root, instead of (-SINF, SINF)), the fail-low move code -6 at the root, and move ordering
// (below). With MODE_FULL those are compiled out.
//
// MODE_MOVES (rvz_solve_moves: the value of every root move) changes the intake and nothing
// below it. The unit a lane takes from the counter is a task (row, j), j < max(1, max_empties)
// >= the row's legal squares: task r is row r % rows, j = r / rows, so every row's first move
// comes before any row's second: neighbouring lanes read neighbouring rows, the tasks that have
// a move are taken first, and the ones that have none (high j) fall where the launch drains.
// Task j of a root with k legal squares makes the move to the j-th set bit of its legal mask
// (j < k) exactly as an open node commits a move, and the child, after its auto-pass never a pass
// root, becomes the lane's depth-0 node: the window negated and the negate flag set when the side
// changed, the caller's window when the child kept the side; a child that ends the game is scored
// in place. The depth-0 return writes that one entry, out_score[row][square], and nothing else.
// A task with j >= k has no move: its lane reads the row, finds that out and asks for the next
// task in the wave's next iteration. Task 0 of every row, which always exists, also writes the
// row's out_count and NOT_A_MOVE / 0 into every entry no task of the row owns (the squares
// outside the legal mask, and the pass entry unless the root is a pass root, which task 0 then
// solves as k_solve_window does and writes itself). So every element has exactly one writer.
//
// Ordering (WIN only): at nodes with at least `order_min` empty squares, the untried move whose
// child leaves the side to move there the fewest legal squares is tried first. It re-scans the
// untried set at every pick and keeps nothing per frame: the frame stays 20 B. The scan is a
// state of the lane's machine, not an inner loop: a scanning lane evaluates ONE candidate per
// iteration of the wave's loop (flips + the opponent's legal mask, exactly what a plain lane
// needs to make its next move), keeps the best so far in registers (square, flip mask, reply
// mask, reply count) and commits it in the iteration that evaluates the last candidate, or at
// once when a candidate leaves no reply (nothing later in index order can beat it). So ordering
// and plain lanes of one wave run the same instructions in every iteration and a scan never holds
// the other lanes up for more than it costs itself. A node with one untried move is not scanned.
// Scans visit no position: `nodes` counts committed moves only.
#include "rvz_negamax.hip.h"

using namespace rvz;

namespace {

constexpr int FRAMES = RVZ_SOLVE_MAX_EMPTIES;
constexpr int FIELDS = 5;
constexpr int SINF = 127;                          // |score| <= 64; fits the packed int8 fields

enum { MODE_FULL = 0, MODE_WINDOW = 1, MODE_MOVES = 2 };

// The state machine of the three kernels (the head of the file has what the modes switch);
// walpha, wbeta and order_min are read only when WIN. MODE_MOVES: n counts tasks over `rows`
// rows; out_score and out_nodes are [rows][NSQ + 1] and out_move is out_count.
template <int BS, int MODE>
__device__ __forceinline__ void solve_rows(
    int n, int rows, const uint64_t* __restrict__ black, const uint64_t* __restrict__ white,
    const int32_t* __restrict__ status, int max_empties, long long node_limit, int walpha,
    int wbeta, int order_min, int32_t* __restrict__ out_score, int32_t* __restrict__ out_move,
    long long* __restrict__ out_nodes, int slot) {
    constexpr bool WIN = MODE != MODE_FULL, MOVES = MODE == MODE_MOVES;
    constexpr int NSQ = Geo<BS>::NSQ;
    constexpr uint64_t FULL = Geo<BS>::FULL;
    __shared__ uint32_t stk[stack_dwords<FRAMES, FIELDS>()];
    uint32_t* const my = stk + threadIdx.x;        // field f of depth d: my[(d * FIELDS + f) * T]

    bool active = false, exhausted = false;
    // row: where emit writes (MOVES: the entry's index in out_score / out_nodes); rootpass: the
    // depth-0 node is the other side's, its score is negated (MOVES: also a child that moved on)
    int row = 0, depth = 0, alpha = 0, beta = 0, best = 0, bestsq = 0, rootpass = 0;
    uint64_t P = 0, O = 0, rem = 0;
    long long nodes = 0;
    // WIN: the scan in progress: candidates not yet evaluated (0: no scan) and the best so far
    uint64_t scan = 0, cf = 0, cMo = 0;
    int csq = 0, ckey = 0;

    auto emit = [&](int score, int move, long long cnt) {
        if constexpr (MOVES) {
            out_score[row] = move == -4 ? RVZ_SOLVE_ABANDONED : score;
        } else {
            out_score[row] = score;
            out_move[row] = move;
        }
        if (out_nodes) out_nodes[row] = cnt;
        active = false;
    };

    for (;;) {
        // ---- an idle lane takes the next row and settles everything that needs no search
        if (!active && !exhausted) {
            const unsigned r = next_row(slot);
            if (r >= (unsigned)n) {
                exhausted = true;
            } else {
                // MOVES: task r is (row src, j); code is the row's out_count, own the legal
                // mask of a root with moves: the entries the row's other tasks write
                const int j = MOVES ? (int)(r / (unsigned)rows) : 0;
                const int src = MOVES ? (int)(r - (unsigned)j * (unsigned)rows) : (int)r;
                int code = 0;
                uint64_t own = 0;
                row = src;
                const uint64_t b = black[row], w = white[row];
                const int side = status[4 * row], over = status[4 * row + 1];
                const int passed = status[4 * row + 3];
                P = side == 1 ? b : w;
                O = side == 1 ? w : b;
                const int diff = __popcll(P) - __popcll(O);
                if ((b & w) || ((b | w) & ~FULL) || (side != 1 && side != 2)) {
                    if constexpr (MOVES) code = -5;
                    else emit(0, -5, 0);
                } else if (over) {
                    if constexpr (MOVES) code = -2;
                    else emit(diff, -2, 1);
                } else if (__popcll(~(b | w) & FULL) > max_empties) {
                    if constexpr (MOVES) code = -3;
                    else emit(0, -3, 0);
                } else {
                    uint64_t M = legal<BS>(P, O);
                    rootpass = 0;
                    nodes = 1;
                    bool mine = true;              // MOVES: the task has an entry to settle
                    if constexpr (MOVES) {
                        own = M;
                        code = M ? __popcll(M) : 1;
                        mine = j < code;
                        row = src * (NSQ + 1) + NSQ;        // a pass root's entry
                        if (M && mine) {
                            // the move to the j-th legal square, as an open node commits one;
                            // its child is this lane's depth-0 node
                            uint64_t m = M;
                            for (int i = 0; i < j; ++i) m &= m - 1;
                            const int sq = __builtin_ctzll(m);
                            row = src * (NSQ + 1) + sq;
                            const uint64_t f = flips<BS>(sq, P, O);
                            const uint64_t nP = P ^ ((1ull << sq) | f), nO = O ^ f;
                            M = legal<BS>(nO, nP);
                            if (M) {               // the other side moves: negated, like a pass
                                P = nO; O = nP;
                                rootpass = 1;
                            } else {               // auto-pass: the root's side keeps the move
                                P = nP; O = nO;
                                M = legal<BS>(nP, nO);
                                if (!M) {          // the move ends the game
                                    emit(__popcll(nP) - __popcll(nO), 0, 1);
                                    mine = false;
                                }
                            }
                        }
                        if (!mine) M = 0;
                    }
                    if (!M && mine) {
                        // the root's only move is the pass (make_move<BS>(g, -1)): the side
                        // flips, passed + 1; two passes in a row end the game
                        const uint64_t M2 = legal<BS>(O, P);
                        if (node_limit < 2) {
                            emit(0, -4, 1);
                        } else if (passed + 1 >= 2) {
                            emit(diff, NSQ, 2);
                        } else if (!M2) {          // the child passes too: the grandchild is over
                            if (node_limit < 3) emit(0, -4, 2);
                            else emit(diff, NSQ, 3);
                        } else {                   // search the child with the negated window;
                            const uint64_t t = P; P = O; O = t;     // the root's score is -its
                            M = M2;
                            rootpass = 1;
                            nodes = 2;
                        }
                    }
                    if (M) {
                        active = true;
                        rem = M;
                        depth = 0;
                        if constexpr (WIN) {
                            alpha = rootpass ? -wbeta : walpha;
                            beta = rootpass ? -walpha : wbeta;
                            scan = 0;
                        } else {
                            alpha = -SINF; beta = SINF;
                        }
                        best = -SINF;
                        bestsq = 0;
                    }
                }
                if constexpr (MOVES) {
                    if (j == 0) {
                        int32_t* const os = out_score + (size_t)src * (NSQ + 1);
                        long long* const on = out_nodes ? out_nodes + (size_t)src * (NSQ + 1) : 0;
                        out_move[src] = code;
                        for (int s = 0; s < NSQ; ++s)
                            if (!((own >> s) & 1)) {
                                os[s] = RVZ_SOLVE_NOT_A_MOVE;
                                if (on) on[s] = 0;
                            }
                        if (code < 0 || own) {
                            os[NSQ] = RVZ_SOLVE_NOT_A_MOVE;
                            if (on) on[NSQ] = 0;
                        }
                    }
                }
            }
        }
        if (__all(exhausted)) break;               // exhausted lanes are never active

        // ---- a finished node returns to its parent (one level per iteration); a scanning node
        // has rem != 0 and best < beta, so it is never here
        if (active && (rem == 0 || best >= beta)) {
            if (depth == 0) {
                // WIN: fail low (-6) is judged on the root's own score, r = best <= alpha
                if (rootpass) emit(-best, NSQ, nodes);
                else emit(best, WIN && best <= walpha ? -6 : bestsq, nodes);
            } else {
                --depth;
                const uint32_t* fr = my + depth * FIELDS * NM_THREADS;
                rem = (uint64_t)fr[0] | ((uint64_t)fr[NM_THREADS] << 32);
                const uint64_t f = (uint64_t)fr[2 * NM_THREADS] |
                                   ((uint64_t)fr[3 * NM_THREADS] << 32);
                const uint32_t pk = fr[4 * NM_THREADS];
                const int sq = pk & 63, keep = (pk >> 6) & 1;
                const int v = keep ? best : -best;
                if (!keep) { const uint64_t t = P; P = O; O = t; }
                P ^= (1ull << sq) | f;             // undo the move
                O ^= f;
                alpha = (int)(int8_t)(pk >> 8);
                beta = (int)(int8_t)(pk >> 16);
                best = (int)(int8_t)(pk >> 24);
                if (v > best) {
                    best = v;
                    if (depth == 0) bestsq = sq;
                }
                if (best > alpha) alpha = best;
            }
        }

        // ---- an open node evaluates one square: its next move, or one candidate of its scan
        if (active && rem != 0 && best < beta) {
            if (nodes >= node_limit) {             // a move will be committed: one node too many
                emit(0, -4, nodes);
            } else {
                const bool ordered = WIN && order_min > 0 && (rem & (rem - 1)) != 0 &&
                                     __popcll(~(P | O) & FULL) >= order_min;
                int sq = __builtin_ctzll(rem);
                if (ordered) {
                    if (!scan) { scan = rem; ckey = 65; }
                    sq = __builtin_ctzll(scan);
                    scan &= scan - 1;
                }
                uint64_t f = flips<BS>(sq, P, O);
                uint64_t Mo = legal<BS>(O ^ f, P ^ ((1ull << sq) | f));
                bool commit = true;
                if (ordered) {
                    const int key = __popcll(Mo);  // 0: the child ends the game or auto-passes
                    if (key < ckey) { ckey = key; csq = sq; cf = f; cMo = Mo; }
                    commit = scan == 0 || ckey == 0;
                    if (commit) { sq = csq; f = cf; Mo = cMo; scan = 0; }
                }
                if (commit) {
                    rem &= ~(1ull << sq);
                    ++nodes;
                    const uint64_t nP = P ^ ((1ull << sq) | f), nO = O ^ f;
                    uint64_t Mm = 0;
                    if (!Mo) Mm = legal<BS>(nP, nO);   // auto-pass: the mover keeps the side
                    if (!(Mo | Mm)) {              // neither side can move: the game is over
                        const int v = __popcll(nP) - __popcll(nO);
                        if (v > best) {
                            best = v;
                            if (depth == 0) bestsq = sq;
                        }
                        if (best > alpha) alpha = best;
                    } else if (depth >= FRAMES) {  // unreachable (see the head of the file)
                        emit(0, -4, nodes);
                    } else {
                        const int keep = Mo ? 0 : 1;
                        uint32_t* fr = my + depth * FIELDS * NM_THREADS;
                        fr[0] = (uint32_t)rem;
                        fr[NM_THREADS] = (uint32_t)(rem >> 32);
                        fr[2 * NM_THREADS] = (uint32_t)f;
                        fr[3 * NM_THREADS] = (uint32_t)(f >> 32);
                        fr[4 * NM_THREADS] = (uint32_t)sq | ((uint32_t)keep << 6) |
                                                ((uint32_t)(alpha & 0xFF) << 8) |
                                                ((uint32_t)(beta & 0xFF) << 16) |
                                                ((uint32_t)(best & 0xFF) << 24);
                        ++depth;
                        if (keep) {
                            P = nP; O = nO; rem = Mm;
                        } else {
                            P = nO; O = nP; rem = Mo;
                            const int a = alpha;
                            alpha = -beta; beta = -a;
                        }
                        best = -SINF;
                    }
                }
            }
        }
    }
}

template <int BS>
__global__ __launch_bounds__(NM_THREADS) void k_solve(
    int n, const uint64_t* __restrict__ black, const uint64_t* __restrict__ white,
    const int32_t* __restrict__ status, int max_empties, long long node_limit,
    int32_t* __restrict__ out_score, int32_t* __restrict__ out_move,
    long long* __restrict__ out_nodes, int slot) {
    solve_rows<BS, MODE_FULL>(n, 0, black, white, status, max_empties, node_limit, 0, 0, 0,
                              out_score, out_move, out_nodes, slot);
}

template <int BS>
__global__ __launch_bounds__(NM_THREADS) void k_solve_window(
    int n, const uint64_t* __restrict__ black, const uint64_t* __restrict__ white,
    const int32_t* __restrict__ status, int max_empties, long long node_limit, int walpha,
    int wbeta, int order_min, int32_t* __restrict__ out_score, int32_t* __restrict__ out_move,
    long long* __restrict__ out_nodes, int slot) {
    solve_rows<BS, MODE_WINDOW>(n, 0, black, white, status, max_empties, node_limit, walpha, wbeta,
                                order_min, out_score, out_move, out_nodes, slot);
}

// tasks = rows * max(1, max_empties) (rvz_solve_moves checks that it fits)
template <int BS>
__global__ __launch_bounds__(NM_THREADS) void k_solve_moves(
    int tasks, int rows, const uint64_t* __restrict__ black,
    const uint64_t* __restrict__ white, const int32_t* __restrict__ status, int max_empties,
    long long node_limit, int walpha, int wbeta, int order_min, int32_t* __restrict__ out_scores,
    int32_t* __restrict__ out_count, long long* __restrict__ out_nodes, int slot) {
    solve_rows<BS, MODE_MOVES>(tasks, rows, black, white, status, max_empties, node_limit,
                               walpha, wbeta, order_min, out_scores, out_count, out_nodes, slot);
}

// What the entry points do before their own launch: the common argument checks (RVZ_EINVAL
// before any HIP call), then for n > 0 negamax_prepare. per_row: the units of work a row makes
// (1; rvz_solve_moves: its tasks per row).
// Returns the grid size, 0 when n == 0 (nothing to launch), or a negative RVZ_E* code.
int solve_prepare(int32_t bs, int32_t n, const uint64_t* black, const uint64_t* white,
                  const int32_t* status, int32_t max_empties, int64_t node_limit,
                  const int32_t* out_score, const int32_t* out_move, hipStream_t s, int* slot,
                  int per_row = 1) {
    if (!board_ok(bs) || n < 0 || max_empties < 0 || max_empties > RVZ_SOLVE_MAX_EMPTIES ||
        node_limit <= 0 || (n > 0 && (!black || !white || !status || !out_score || !out_move)))
        return RVZ_EINVAL;
    return n == 0 ? 0 : negamax_prepare((int64_t)n * per_row, s, slot);
}

}  // namespace

extern "C" int rvz_solve(int32_t bs, int32_t n, const uint64_t* black, const uint64_t* white,
                         const int32_t* status, int32_t max_empties, int64_t node_limit,
                         int32_t* out_score, int32_t* out_move, int64_t* out_nodes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    int slot = 0;
    const int wgs = solve_prepare(bs, n, black, white, status, max_empties, node_limit, out_score,
                                  out_move, s, &slot);
    if (wgs <= 0) return wgs;                      // an error code, or RVZ_OK for n == 0
    return launch_bs(bs, k_solve<8>, k_solve<6>, dim3(wgs), dim3(NM_THREADS), s, n, black, white,
                     status, max_empties, (long long)node_limit, out_score, out_move,
                     (long long*)out_nodes, slot);
}

extern "C" int rvz_solve_window(int32_t bs, int32_t n, const uint64_t* black,
                                const uint64_t* white, const int32_t* status, int32_t max_empties,
                                int64_t node_limit, int32_t alpha, int32_t beta,
                                int32_t order_min_empties, int32_t* out_score, int32_t* out_move,
                                int64_t* out_nodes, void* stream) {
    if (alpha < -64 || alpha >= beta || beta > 64 || order_min_empties < 0) return RVZ_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    int slot = 0;
    const int wgs = solve_prepare(bs, n, black, white, status, max_empties, node_limit, out_score,
                                  out_move, s, &slot);
    if (wgs <= 0) return wgs;                      // an error code, or RVZ_OK for n == 0
    return launch_bs(bs, k_solve_window<8>, k_solve_window<6>, dim3(wgs), dim3(NM_THREADS), s, n,
                     black, white, status, max_empties, (long long)node_limit, alpha, beta,
                     order_min_empties, out_score, out_move, (long long*)out_nodes, slot);
}

extern "C" int rvz_solve_moves(int32_t bs, int32_t n, const uint64_t* black, const uint64_t* white,
                               const int32_t* status, int32_t max_empties, int64_t node_limit,
                               int32_t alpha, int32_t beta, int32_t order_min_empties,
                               int32_t* out_scores, int32_t* out_count, int64_t* out_nodes,
                               void* stream) {
    if (alpha < -64 || alpha >= beta || beta > 64 || order_min_empties < 0) return RVZ_EINVAL;
    if (board_ok(bs) && n > 0 && (int64_t)n * (bs * bs + 1) > INT32_MAX) return RVZ_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int per_row = max_empties > 1 ? max_empties : 1;
    int slot = 0;
    const int wgs = solve_prepare(bs, n, black, white, status, max_empties, node_limit, out_scores,
                                  out_count, s, &slot, per_row);
    if (wgs <= 0) return wgs;                      // an error code, or RVZ_OK for n == 0
    const int tasks = n * per_row;                 // per_row <= 14 < S*S + 1: fits
    return launch_bs(bs, k_solve_moves<8>, k_solve_moves<6>, dim3(wgs), dim3(NM_THREADS), s, tasks,
                     n, black, white, status, max_empties, (long long)node_limit, alpha, beta,
                     order_min_empties, out_scores, out_count, (long long*)out_nodes, slot);
}
