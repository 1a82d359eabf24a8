// rvz_alphabeta.hip — depth-limited heuristic search: batched negamax to a fixed depth over the
// reference's rules for gfx950 (MI355X), exported as rvz_alphabeta (include/rvz.h). Its own
// translation unit: neither the engine's nor the solver's code objects depend on it.
//
// Definition (include/rvz.h, DESIGN.md §Depth-limited alpha-beta): value(g, d) = T(g) when g is
// over, h(g) when d == 0, else the maximum over g's legal squares in increasing index of the
// child made by make_move<BS> (auto-pass included, at no depth), negated when the side changed;
// the first maximum kept. h is the caller's square table plus a mobility term, T the final disc
// difference pushed beyond every h by RVZ_AB_WIN.
//
// Shape: rvz_solve.hip's: one position per LANE, persistent lanes that take the next row from a
// per-call device counter in the iteration that finishes a row, an explicit stack in LDS laid
// out [depth][field][lane] in dwords, no recursion, no run-time-indexed register array, no
// scratch. The head of rvz_negamax.hip.h has the reasons; that header holds what the two files
// have in common around their loops (geometry, the stack's size, the row counter, of which this
// translation unit has a copy of its own, and the host side of a launch) and says why the loops
// are two texts. This one is its own state machine and not a mode of solve_rows: the solver
// bounds its stack by the empty squares and packs alpha / beta / best as int8; here the bound is
// the caller's depth, and a score needs 16 bits.
//
// Frame (what the return needs), 6 dwords = 24 B: the moves left (2), the flip mask of the move
// being searched (2: the undo), {square, kept-side flag, best} and {alpha, beta} with the three
// scores as int16. A frame is pushed only under a child that is searched on, i.e. that has at
// least one ply of depth left and a move; every ply places a disc and costs one of `depth`, and
// the root has none above it, so a row pushes at most depth - 1 frames:
// FRAMES = RVZ_AB_MAX_DEPTH covers it with room, and the push checks it all the same.
// LDS: 128 lanes x 12 frames x 24 B = 36,864 B per workgroup: four workgroups (8 waves, 2 per
// SIMD) fit in a CU's 160 KiB.
//
// The frontier: a child with no depth left is scored in place, in the iteration that makes the
// move. h needs both sides' legal masks there; the reply mask is computed anyway (it decides
// auto-pass and game end), the mover's own is added. h is antisymmetric in the two sides, so one
// expression in the parent's terms serves the child that moved on and the one that auto-passed.
// The weights travel by value in the kernel's arguments (SGPRs, constant indices in an unrolled
// loop): no table in memory, nothing to copy, and a captured launch keeps its weights.
//
// Pruning: fail-soft alpha-beta. A root's children are searched with the window (best, +inf)
// in the root's terms: a child whose true value is above the root's best so far comes back
// exact, any other comes back <= best and is dropped by the strict comparison, so the score and
// the first-maximum move equal the unpruned definition. The argument is the solver's
// and does not look at what a leaf is: h(leaf) and T(leaf) are numbers that depend on the leaf
// alone, never on the window. Node counts depend on the row and the arguments alone.
#include "rvz_negamax.hip.h"

using namespace rvz;

namespace {

constexpr int AB_FRAMES = RVZ_AB_MAX_DEPTH;
constexpr int AB_FIELDS = 6;
constexpr int AB_INF = 32000;                      // |score| <= RVZ_AB_WIN + 64; fits int16
static_assert(RVZ_AB_WIN + 64 < AB_INF && AB_INF <= INT16_MAX, "scores are packed as int16");
static_assert(RVZ_AB_HEUR_MAX < RVZ_AB_WIN - 64, "a proven result outranks a heuristic one");

// weights[s] for s < NSQ, the mobility weight at [NSQ] (8x8: all 65; 6x6: the first 37)
struct ab_weights {
    int32_t w[65];
};

// T of a finished game from the side whose disc difference is diff
__device__ __forceinline__ int terminal(int diff) {
    return diff > 0 ? RVZ_AB_WIN + diff : (diff < 0 ? diff - RVZ_AB_WIN : 0);
}

// h from the side that owns P: the square table over both sides' discs plus the mobility term;
// MP / MO are the legal masks of P's and O's side
template <int BS>
__device__ __forceinline__ int heuristic(const ab_weights& wt, uint64_t P, uint64_t O,
                                         uint64_t MP, uint64_t MO) {
    constexpr int NSQ = Geo<BS>::NSQ;
    int acc = wt.w[NSQ] * (__popcll(MP) - __popcll(MO));
#pragma unroll
    for (int s = 0; s < NSQ; ++s)
        acc += wt.w[s] * ((int)((P >> s) & 1) - (int)((O >> s) & 1));
    return acc;
}

template <int BS>
__global__ __launch_bounds__(NM_THREADS) void k_alphabeta(
    int n, const uint64_t* __restrict__ black, const uint64_t* __restrict__ white,
    const int32_t* __restrict__ status, int max_depth, const ab_weights wt, long long node_limit,
    int32_t* __restrict__ out_score, int32_t* __restrict__ out_move,
    long long* __restrict__ out_nodes, int slot) {
    constexpr int NSQ = Geo<BS>::NSQ;
    constexpr uint64_t FULL = Geo<BS>::FULL;
    __shared__ uint32_t stk[stack_dwords<AB_FRAMES, AB_FIELDS>()];
    uint32_t* const my = stk + threadIdx.x;        // field f of depth d: my[(d * FIELDS + f) * T]

    bool active = false, exhausted = false;
    // rootpass: the depth-0 node is the other side's (the root passed), its score is negated
    int row = 0, depth = 0, alpha = 0, beta = 0, best = 0, bestsq = 0, rootpass = 0;
    uint64_t P = 0, O = 0, rem = 0;
    long long nodes = 0;

    auto emit = [&](int score, int move, long long cnt) {
        out_score[row] = score;
        out_move[row] = move;
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
                row = (int)r;
                const uint64_t b = black[row], w = white[row];
                const int side = status[4 * row], over = status[4 * row + 1];
                const int passed = status[4 * row + 3];
                P = side == 1 ? b : w;
                O = side == 1 ? w : b;
                const int diff = __popcll(P) - __popcll(O);
                if ((b & w) || ((b | w) & ~FULL) || (side != 1 && side != 2)) {
                    emit(0, -5, 0);
                } else if (over) {
                    emit(terminal(diff), -2, 1);
                } else {
                    uint64_t M = legal<BS>(P, O);
                    rootpass = 0;
                    nodes = 1;
                    if (!M) {
                        // the root's only move is the pass (make_move<BS>(g, -1)): the side
                        // flips, passed + 1; two passes in a row end the game. No depth is spent
                        const uint64_t M2 = legal<BS>(O, P);
                        if (node_limit < 2) {
                            emit(0, -4, 1);
                        } else if (passed + 1 >= 2) {
                            emit(terminal(diff), NSQ, 2);
                        } else if (!M2) {          // the child passes too: the grandchild is over
                            if (node_limit < 3) emit(0, -4, 2);
                            else emit(terminal(diff), NSQ, 3);
                        } else {                   // search the child at the root's depth;
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
                        alpha = -AB_INF; beta = AB_INF;
                        best = -AB_INF;
                        bestsq = 0;
                    }
                }
            }
        }
        if (__all(exhausted)) break;               // exhausted lanes are never active

        // ---- a finished node returns to its parent (one level per iteration)
        if (active && (rem == 0 || best >= beta)) {
            if (depth == 0) {
                if (rootpass) emit(-best, NSQ, nodes);
                else emit(best, bestsq, nodes);
            } else {
                --depth;
                const uint32_t* fr = my + depth * AB_FIELDS * NM_THREADS;
                rem = (uint64_t)fr[0] | ((uint64_t)fr[NM_THREADS] << 32);
                const uint64_t f = (uint64_t)fr[2 * NM_THREADS] |
                                   ((uint64_t)fr[3 * NM_THREADS] << 32);
                const uint32_t pk = fr[4 * NM_THREADS], ab = fr[5 * NM_THREADS];
                const int sq = pk & 63, keep = (pk >> 6) & 1;
                const int v = keep ? best : -best;
                if (!keep) { const uint64_t t = P; P = O; O = t; }
                P ^= (1ull << sq) | f;             // undo the move
                O ^= f;
                best = (int)(int16_t)(pk >> 16);
                alpha = (int)(int16_t)ab;
                beta = (int)(int16_t)(ab >> 16);
                if (v > best) {
                    best = v;
                    if (depth == 0) bestsq = sq;
                }
                if (best > alpha) alpha = best;
            }
        }

        // ---- an open node makes its next move; the child is scored in place when the game ends
        // there or no depth is left, and searched on otherwise
        if (active && rem != 0 && best < beta) {
            if (nodes >= node_limit) {             // a move will be committed: one node too many
                emit(0, -4, nodes);
            } else {
                const int sq = __builtin_ctzll(rem);
                const bool frontier = depth + 1 >= max_depth;
                const uint64_t f = flips<BS>(sq, P, O);
                const uint64_t nP = P ^ ((1ull << sq) | f), nO = O ^ f;
                const uint64_t Mo = legal<BS>(nO, nP);
                uint64_t Mm = 0;
                // auto-pass: the mover keeps the side; the frontier's h wants both masks
                if (!Mo || frontier) Mm = legal<BS>(nP, nO);
                rem &= ~(1ull << sq);
                ++nodes;
                if (!(Mo | Mm) || frontier) {
                    // in the parent's terms, whichever side is to move in the child
                    const int v = (Mo | Mm) ? heuristic<BS>(wt, nP, nO, Mm, Mo)
                                            : terminal(__popcll(nP) - __popcll(nO));
                    if (v > best) {
                        best = v;
                        if (depth == 0) bestsq = sq;
                    }
                    if (best > alpha) alpha = best;
                } else if (depth >= AB_FRAMES) {   // unreachable (see the head of the file)
                    emit(0, -4, nodes);
                } else {
                    const int keep = Mo ? 0 : 1;
                    uint32_t* fr = my + depth * AB_FIELDS * NM_THREADS;
                    fr[0] = (uint32_t)rem;
                    fr[NM_THREADS] = (uint32_t)(rem >> 32);
                    fr[2 * NM_THREADS] = (uint32_t)f;
                    fr[3 * NM_THREADS] = (uint32_t)(f >> 32);
                    fr[4 * NM_THREADS] = (uint32_t)sq | ((uint32_t)keep << 6) |
                                         ((uint32_t)(best & 0xFFFF) << 16);
                    fr[5 * NM_THREADS] = (uint32_t)(alpha & 0xFFFF) |
                                         ((uint32_t)(beta & 0xFFFF) << 16);
                    ++depth;
                    if (keep) {
                        P = nP; O = nO; rem = Mm;
                    } else {
                        P = nO; O = nP; rem = Mo;
                        const int a = alpha;
                        alpha = -beta; beta = -a;
                    }
                    best = -AB_INF;
                }
            }
        }
    }
}

}  // namespace

extern "C" int rvz_alphabeta(int32_t bs, int32_t n, const uint64_t* black, const uint64_t* white,
                             const int32_t* status, int32_t depth, const int32_t* weights,
                             int64_t node_limit, int32_t* out_score, int32_t* out_move,
                             int64_t* out_nodes, void* stream) {
    if (!board_ok(bs) || n < 0 || depth < 1 || depth > RVZ_AB_MAX_DEPTH ||
        node_limit <= 0 || !weights ||
        (n > 0 && (!black || !white || !status || !out_score || !out_move)))
        return RVZ_EINVAL;
    const int nsq = bs * bs;
    ab_weights wt = {};
    int64_t bound = 0;
    for (int s = 0; s <= nsq; ++s) {
        const int64_t a = weights[s] < 0 ? -(int64_t)weights[s] : (int64_t)weights[s];
        bound += s < nsq ? a : a * nsq;
        wt.w[s] = weights[s];
    }
    if (bound > RVZ_AB_HEUR_MAX) return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    hipStream_t s = (hipStream_t)stream;
    int slot = 0;
    const int wgs = negamax_prepare(n, s, &slot);
    if (wgs < 0) return wgs;
    return launch_bs(bs, k_alphabeta<8>, k_alphabeta<6>, dim3(wgs), dim3(NM_THREADS), s, n, black,
                     white, status, depth, wt, (long long)node_limit, out_score, out_move,
                     (long long*)out_nodes, slot);
}
