// rvz_search.hip.h — the search's device code: the tree (Node, the meta and link words), the kernel
// argument (View), and the per-game phases every search kernel is made of, one wavefront per game:
// expand + backup, select, act, reset. The pull-style kernels (csrc/rvz_engine.hip: k_step, k_act,
// k_reset, ...) and the fused self-play kernel (csrc/rvz_play.hip.h: k_play) are these functions
// under different launches; the layout and the exactness notes are in csrc/rvz_engine.hip's header.
// Device code only. Node and View are types of namespace rvz (struct rvz_engine holds a View and
// is seen by two translation units); the functions are internal to each unit that includes them.
//
// The instrumented builds' device arrays (g_walk, g_wtime, g_ftime below) exist once per
// translation unit (no -fgpu-rdc): a reader has to sit in the unit whose kernels wrote the words.
//   rvz_walk_stats, rvz_walk_times   g_walk, g_wtime     written by k_step   csrc/rvz_engine.hip
//   rvz_play_walk_read               g_wtime, g_ftime    written by k_play   csrc/rvz_play.hip
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rvz.h"
#include "rvz_dirichlet.hip.h"
#include "rvz_openings.hip.h"
#include "rvz_philox.hip.h"
#include "rvz_pow.hip.h"
#include "rvz_rules.hip.h"
#include "rvz_wave_dpp.hip.h"

namespace rvz {
namespace {

constexpr int WAVE = 64;
constexpr int WPB = 4;            // waves (games) per 256-thread workgroup
constexpr int PATH_CAP = 64;      // path length limit: ceil(sims / batch) <= 64
constexpr int RNG_DRAWS = 64;     // random_sample() values per seed (a game has <= 60 plies)

}  // namespace

struct Node {
    int32_t n;   // visit_count
    float w;     // value_sum
    float p;     // prior
    float c;     // cached_ucb; NaN = not cached
};
static_assert(sizeof(Node) == 16, "node is one 16-byte load");

namespace {

// meta word: sq[0:6) turn[6:8) terminal[8] tv[9:11) (0: 0.0, 1: +1.0, 2: -1.0) nchild[11:18) block[18:32)
__host__ __device__ constexpr uint32_t meta_pack(int sq, int turn) {
    return (uint32_t)(sq & 63) | ((uint32_t)(turn & 3) << 6);
}
__device__ __forceinline__ int m_sq(uint32_t m) { return (int)(m & 63u); }
__device__ __forceinline__ int m_turn(uint32_t m) { return (int)((m >> 6) & 3u); }
__device__ __forceinline__ bool m_term(uint32_t m) { return (m >> 8) & 1u; }
__device__ __forceinline__ float m_tv(uint32_t m) {
    const uint32_t t = (m >> 9) & 3u;
    return t == 1u ? 1.0f : (t == 2u ? -1.0f : 0.0f);
}
__device__ __forceinline__ int m_nchild(uint32_t m) { return (int)((m >> 11) & 127u); }
__device__ __forceinline__ int m_block(uint32_t m) { return (int)(m >> 18); }

}  // namespace

struct View {  // kernel argument: device pointers + sizes
    int G, M;
    float cpuct;
    uint64_t* black;
    uint64_t* white;
    int32_t* status;  // [G][4]
    Node* nodes;
    uint32_t* meta;
    int32_t* path;  // [G][PATH_CAP]
    int32_t* pend;
    int32_t* plen;
    uint64_t* leaf_legal;
    uint64_t* root_legal;  // [G] legal mask of the current search's root (its children's squares)
    uint32_t* leaf_meta;   // [G] meta word of the queued leaf (written by select, read by expand)
    int32_t* nexp;
    double* rng_u;          // [G][RNG_DRAWS]
    int32_t* rng_pos;
    int32_t* err;
    unsigned long long* stats;  // [3][G] algorithmic bytes per game: k_step, k_act, k_expand_backup; or null
    // compacted leaf batches (rvz_search_compact), or null: live[(e * NS + s) * PITCH] = live
    // leaves of stripe s (games [s*STRIPE, (s+1)*STRIPE)) in batch e of the current search, at
    // rows [s*STRIPE, s*STRIPE + count) of leaf_x; row_of[g] = game g's row
    int32_t* live;   // [E][NS][PITCH]
    int32_t* row_of;  // [G]
    unsigned long long* live_total;  // running sum of the live counts (rows handed out)
    int E, NS;
    // NN-output memo across consecutive searches (rvz_search_memo; memo = 0: off). The pool has
    // two halves of E expansion blocks; a search writes one half while the previous search's
    // tree stays readable in the other. bval[g][b]: the NN value of the node expanded into block
    // b; carry[g]: the link (LINK_* below) of the child the last move went to, or LINK_NONE.
    int memo;
    uint32_t* carry;  // [G]
    float* bval;      // [G][2E]
    // Dirichlet noise on the priors of a root's children (rvz_search_root_noise; noise_eps = 0:
    // off): P' = fl(fl(noise_om * P) + fl(noise_eps * eta)), eta from csrc/rvz_dirichlet.hip.h.
    // seed32[g]: the seed game g's MT19937 stream was last seeded with (reset_game), the key of
    // its noise
    float noise_eps, noise_om, noise_alpha;
    uint32_t noise_salt;
    uint32_t* seed32;  // [G]
    float* eta;        // [G][64] the current root's eta per square (written when the root is created)
    // Temperature schedule of the act (rvz_act_schedule; sched_from = 0: off): a game whose
    // position before the move has at least sched_from discs acts at sched_late instead of the
    // call's temperature
    int sched_from;
    double sched_late;
    // Opening pool (rvz_env_openings; open_n = 0: off): a game reset with seed s starts from row
    // opening_index(s, open_salt, open_n) of the engine's own copy of the pool, with black or
    // white (open_side: 1 | 2) to move
    int open_n;
    uint32_t open_salt;
    const uint64_t* open_black;
    const uint64_t* open_white;
    const int32_t* open_side;
};

namespace {

// A link names an expanded node of the previous search's tree (the same position as the new
// node it is attached to): its index, child count and block. Stored in the `c` (cached UCB) field
// of an unvisited node, which the reference formula never reads while N == 0 (mcts.py:96-97;
// the first backup overwrites it with "not cached"), and in carry[g] for the next root.
// LINK_NONE is the "not cached" NaN every other node carries; a link is < 2^28, never a NaN.
constexpr uint32_t LINK_NONE = 0x7fc00000u;
__host__ __device__ constexpr uint32_t link_pack(int node, int nchild, int block) {
    return (uint32_t)node | ((uint32_t)nchild << 14) | ((uint32_t)block << 21);
}
__device__ __forceinline__ bool link_ok(uint32_t l) { return l < (1u << 28); }
__device__ __forceinline__ int link_node(uint32_t l) { return (int)(l & 0x3fffu); }
__device__ __forceinline__ int link_nchild(uint32_t l) { return (int)((l >> 14) & 127u); }
__device__ __forceinline__ int link_block(uint32_t l) { return (int)((l >> 21) & 127u); }

// ERR_NN: an evaluator handed the expand a non-finite value or probability (an overflowed or
// broken leaf evaluator must not feed the tree silently; the reference would play on with NaN)
enum : int32_t { ERR_RNG = 1, ERR_POOL = 2, ERR_PATH = 4, ERR_NN = 8 };

// Walk counters of the select phase per game (instrumented builds only, -DRVZ_WALK_STATS:
// tools/exp_walks.py): [0] walks from the root, [1] tree levels read, [2] known-terminal hits
// backed up in memory, [3] hits taken by the register fast path, [4] new terminals found
#ifdef RVZ_WALK_STATS
constexpr int WALK_STATS_MAX = 1 << 16;
__device__ unsigned int g_walk[WALK_STATS_MAX][5];
#define WALK_STAT(i, k) \
    if (lane == 0 && g < WALK_STATS_MAX) g_walk[g][i] += (k)
// shader-clock split of a game's k_step work: [0] expand phase (k_play: the cross-game table
// lookups), [1] walk levels, [2] memory backups of known terminals, [3] register fast path,
// [4] leaf (position, legal moves, queue)
__device__ unsigned long long g_wtime[WALK_STATS_MAX][5];
#define WT_NOW(t) const uint64_t t = __builtin_amdgcn_s_memtime()
#define WT_ADD(i, t0) \
    if (lane == 0 && g < WALK_STATS_MAX) g_wtime[g][i] += __builtin_amdgcn_s_memtime() - (t0)
// the fused kernel's game steps (k_play, tools/exp_play_walks.py): [0] expand, [1] act +
// autoreset, [2] the whole step (a game's turn in one search phase), [3] steps
__device__ unsigned long long g_ftime[WALK_STATS_MAX][4];
#define FT_ADD(i, t0) \
    if (lane == 0 && g < WALK_STATS_MAX) g_ftime[g][i] += __builtin_amdgcn_s_memtime() - (t0)
#define FT_CNT() \
    if (lane == 0 && g < WALK_STATS_MAX) g_ftime[g][3] += 1
#else
#define FT_ADD(i, t0)
#define FT_CNT()
#define WALK_STAT(i, k)
#define WT_NOW(t)
#define WT_ADD(i, t0)
#endif

__device__ __forceinline__ GameS load_game(const View& v, int g) {
    GameS s;
    s.black = v.black[g];
    s.white = v.white[g];
    const int4 st = reinterpret_cast<const int4*>(v.status)[g];
    s.side = st.x; s.over = st.y; s.winner = st.z; s.passed = st.w;
    return s;
}
__device__ __forceinline__ void store_game(const View& v, int g, const GameS& s) {
    v.black[g] = s.black;
    v.white[g] = s.white;
    reinterpret_cast<int4*>(v.status)[g] = make_int4(s.side, s.over, s.winner, s.passed);
}

// ---- backup (mcts.py:625-640): lane j updates path node plen-1-j; `copies` sequential adds ----
// path_reg: lane i holds the i-th node of the path (root = lane 0). Returns the updated visit
// count of the root in every lane.
__device__ __forceinline__ int backup_path(Node* nodes, int path_reg, int plen, float value,
                                           int copies, int lane, bool order_before) {
    // order this wave's earlier stores to path nodes (UCB caches) before the read-modify-write
    if (order_before) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    // lane d holds the path node at depth d (the root in lane 0): each lane updates its own node
    const int nid = path_reg;
    int n_after = 0;
    if (lane < plen) {
        // sign = +1 at the leaf (depth plen - 1), then alternates toward the root
        const float sv = ((plen - 1 - lane) & 1) ? -value : value;
        Node nd = nodes[nid];
        float w = nd.w;
        for (int k = 0; k < copies; ++k) w = w + sv;
        nd.n += copies;
        nd.w = w;
        nd.c = __int_as_float(0x7fc00000);  // del cached_ucb
        nodes[nid] = nd;
        n_after = nd.n;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    return __builtin_amdgcn_readlane(n_after, 0);  // the root's lane
}

// UCB of an expanded child whose score is not cached (mcts.py:102-114); turn_c = child's turn.
// sqrt_np = sqrt_count(parent N): exactly `np.float32(math.sqrt(parent_visit_count))` as the
// reference's NumPy promotion takes it.
// np.float32(math.sqrt(n)) for a visit count n < 2^24: math.sqrt rounds the exact root to 53
// bits, the cast to 24; rounding twice through p' >= 2p + 2 bits (53 >= 50) equals rounding once
// for sqrt (Figueroa), so the correctly rounded f32 sqrt of (float)n (exact for n < 2^24) is the
// same value (-fhip-fp32-correctly-rounded-divide-sqrt; tests/test_gpu_numerics.py)
__device__ __forceinline__ float sqrt_count(int n) { return __builtin_sqrtf((float)n); }

__device__ __forceinline__ float ucb_score(const Node& c, float sqrt_np, int turn_c, float cpuct) {
    float u = cpuct * c.p;
    u = u * sqrt_np;
    u = u / (float)(1 + c.n);
    float q = c.w / (float)(c.n > 1 ? c.n : 1);
    if (turn_c != 1) q = -q;
    return q + u;
}

// Root noise in two steps, both behind wave-uniform branches on v.noise_eps > 0 (nothing of it
// runs with the noise off). root_noise_sample: when a search creates its root (select_phase,
// first batch; few registers are live there) eta goes to the game's row of v.eta, one lane per
// square; `root` is the root's position, its disc count the root's tag (every ply places a disc,
// so a game never has two roots with one count), V its legal mask. root_noise_mix: wherever the
// root is expanded later (the next launch's expand phase, the memo, a table hit) the prior of
// square sq becomes P' = fl(fl((1 - eps) P) + fl(eps eta)), each operation rounded on its own,
// at the cost of one load: the sampler's registers never meet the walk's or the act's.
__device__ __forceinline__ void root_noise_sample(const View& v, int g, int lane,
                                                  const GameS& root, uint64_t V) {
    const float eta = dirichlet_eta(v.seed32[g], v.noise_salt,
                                    (uint32_t)__popcll(root.black | root.white), v.noise_alpha,
                                    V, lane, v.err);
    v.eta[(size_t)g * WAVE + lane] = eta;
    // the memo may expand the root later in this launch, reading other lanes' squares
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}
__device__ __forceinline__ float root_noise_mix(const View& v, int g, int sq, float prob) {
    const float eta = v.eta[(size_t)g * WAVE + sq];
    return __fadd_rn(__fmul_rn(v.noise_om, prob), __fmul_rn(v.noise_eps, eta));
}

// Inputs of the pending expand + backup, all loaded at the head of a launch (no dependent loads:
// the leaf's meta word is kept in per-game scratch by the select that queued it).
struct ExpIn {
    int copies, plen, path_reg, e;
    uint64_t V;
    uint32_t lm;
    float val, prob, xpass;
};

template <int BS>
__device__ __forceinline__ ExpIn expand_load(const View& v, int g, int lane,
                                             const float* __restrict__ policy,
                                             const float* __restrict__ value) {
    constexpr int NSQ = Geo<BS>::NSQ, NPOL = Geo<BS>::NPOL;
    ExpIn x;
    x.copies = v.pend[g];
    x.plen = v.plen[g];
    x.path_reg = v.path[g * PATH_CAP + lane];
    x.V = v.leaf_legal[g];
    x.e = v.nexp[g];
    x.lm = v.leaf_meta[g];
    const int r = v.live ? v.row_of[g] : g;
    x.val = value[r];
    const float* row = policy + (size_t)r * NPOL;
    x.prob = lane < NSQ ? row[lane] : 0.0f;
    x.xpass = row[NSQ];
    return x;
}

// F.softmax(policy_logits, dim=1) over all S*S+1 outputs (mcts.py:596), one row per wave: lane
// s < NSQ holds logit s, every lane the pass logit; returns (lane s's probability, 0 for lanes
// >= NSQ; the pass probability). The expand's fused softmax and rvz_policy_softmax are this one
// function (the expand uses .x only: no pass child is ever created).
template <int NSQ>
__device__ __forceinline__ float2 policy_softmax(float logit, float xpass, int lane) {
    const float mx = fmaxf(wave_max_f(lane < NSQ ? logit : -INFINITY), xpass);
    const float ex = lane < NSQ ? expf(logit - mx) : 0.0f;
    const float ep = expf(xpass - mx);
    const float denom = wave_sum_f(ex) + ep;
    return make_float2(ex / denom, ep / denom);
}

// expand + backup of the queued leaf: _process_batch pass 2 (mcts.py:600-623) and
// MCTSNode.expand (:141-161). Returns the root's visit count after the backup (-1: nothing to
// do) and, when the expanded leaf is the root, its new meta word in *root_meta.
template <int BS>
__device__ __forceinline__ int expand_backup_phase(const View& v, int g, int lane, ExpIn x,
                                                   int is_logits, uint32_t* root_meta,
                                                   unsigned long long& ab) {
    constexpr int NSQ = Geo<BS>::NSQ, NPOL = Geo<BS>::NPOL;
    if (x.copies == 0) return -1;
    const int path_reg = lane < x.plen ? x.path_reg : 0;
    const int leaf = __builtin_amdgcn_readlane(path_reg, x.plen - 1);
    Node* nodes = v.nodes + (size_t)g * v.M;
    uint32_t* meta = v.meta + (size_t)g * v.M;
    float prob = x.prob;
    if (is_logits) prob = policy_softmax<NSQ>(prob, x.xpass, lane).x;
    {   // non-finite NN output (any of the 65 probabilities or the value): device error word
        const bool bad = !__builtin_isfinite(x.val) || !__builtin_isfinite(x.xpass) ||
                         (lane < NSQ && !__builtin_isfinite(prob));
        if (__builtin_amdgcn_ballot_w64(bad) && lane == 0) atomicOr(v.err, ERR_NN);
    }
    if (leaf == 0 && v.noise_eps > 0.0f)   // the root's children: Dirichlet noise on the priors
        prob = root_noise_mix(v, g, lane, prob);
    const int base = 1 + x.e * NSQ;
    if (base + NSQ > v.M) {
        if (lane == 0) atomicOr(v.err, ERR_POOL);
        return -1;
    }
    const uint64_t V = x.V;
    if (lane < NSQ && ((V >> lane) & 1ull)) {
        const int idx = __popcll(V & ((1ull << lane) - 1ull));
        Node c;
        c.n = 0; c.w = 0.0f; c.p = prob; c.c = __int_as_float(0x7fc00000);
        nodes[base + idx] = c;
        meta[base + idx] = meta_pack(lane, 3 - m_turn(x.lm));
    }
    const uint32_t nlm = x.lm | ((uint32_t)__popcll(V) << 11) | ((uint32_t)x.e << 18);
    if (lane == 0) {
        meta[leaf] = nlm;
        v.nexp[g] = x.e + 1;
        v.pend[g] = 0;
        if (v.memo) v.bval[(size_t)g * 2 * v.E + x.e] = x.val;   // the next search's memo
    }
    if (leaf == 0 && root_meta) *root_meta = nlm;
    // the path nodes are not among the nodes written above: no ordering needed before the RMW
    const int root_n = backup_path(nodes, path_reg, x.plen, x.val, x.copies, lane, false);
    if (v.stats) {
        // pend/plen/path/legal/nexp/leaf-meta reads, policy row + value, leaf meta w, children,
        // backup
        const unsigned long long nch = (unsigned long long)__popcll(V);
        ab += 8ull + 4ull * x.plen + 8 + 4 + 4 + 4ull * NPOL + 4 + 4 + 20ull * nch +
              32ull * x.plen + 8;
    }
    return root_n;
}

// rvz_search_skip: the last batch's leaf is not evaluated. Its evaluation would only set the
// leaf's children priors and add the value to W along the path — state the discarded tree never
// reads again — while the visit counts grow by the queued copies regardless (mcts.py:625-640), so
// N alone is backed up here and the visits, p and the move are those of the evaluated search.
__device__ __forceinline__ void backup_visits_only(const View& v, int g, int lane,
                                                   unsigned long long& ab) {
    const int copies = v.pend[g], plen = v.plen[g];
    if (copies == 0) return;
    const int path_reg = lane < plen ? v.path[g * PATH_CAP + lane] : 0;
    Node* nodes = v.nodes + (size_t)g * v.M;
    if (lane < plen) nodes[path_reg].n += copies;   // lane d: the path node at depth d
    if (lane == 0) v.pend[g] = 0;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (v.stats) ab += 8ull + 4ull * plen + 8ull * plen;
}

// A leaf whose position the previous search of this game already expanded (link lk: that node
// of the previous tree, kept in the other half of the pool): _process_batch pass 2 (mcts.py:
// 600-623) with that expansion's NN output instead of a new evaluation. An h2 row's outputs
// depend only on the position (test_h2_live_rows), so the priors (the softmax of the row at the
// legal squares, which are the old node's children in row-major order, exactly the squares the
// same position yields here) and the value are bitwise what the evaluator would return for this
// leaf now. The children get their own links (the old children that were expanded too); the
// value is backed up `copies` times at once, where the evaluated leaf's backup would run at the
// head of the next launch — the same point of the batch (after its terminal backups).
template <int BS>
__device__ __forceinline__ int memo_expand_backup(const View& v, int g, int lane, int leaf,
                                                  uint32_t lm, int path_reg, int plen,
                                                  uint32_t lk, int copies,
                                                  unsigned long long& ab) {
    constexpr int NSQ = Geo<BS>::NSQ;
    Node* nodes = v.nodes + (size_t)g * v.M;
    uint32_t* meta = v.meta + (size_t)g * v.M;
    const int nch = link_nchild(lk), ob = 1 + link_block(lk) * NSQ;
    // one round trip: the old children rows, the old node's value and the expansion counter
    Node oc;
    uint32_t ocm = 0;
    if (lane < nch) {
        oc = nodes[ob + lane];
        ocm = meta[ob + lane];
    }
    const float val = v.bval[(size_t)g * 2 * v.E + link_block(lk)];
    const int e = v.nexp[g];
    const int base = 1 + e * NSQ;
    if (base + NSQ > v.M) {
        if (lane == 0) atomicOr(v.err, ERR_POOL);
        return -1;
    }
    float prior = lane < nch ? oc.p : 0.0f;
    if (leaf == 0 && v.noise_eps > 0.0f) {
        // the new root takes the carried node's clean priors (a node the memo links to is never a
        // root: the carried node was a child of the previous root, expanded from its own NN
        // row); the noise goes into the new root's copy. Child i sits in lane i, its square is
        // m_sq(ocm)
        if (lane < nch) prior = root_noise_mix(v, g, m_sq(ocm), prior);
    }
    if (lane < nch) {
        Node c;
        c.n = 0; c.w = 0.0f; c.p = prior;
        const bool expd = m_nchild(ocm) > 0 && !m_term(ocm);
        c.c = __uint_as_float(expd ? link_pack(ob + lane, m_nchild(ocm), m_block(ocm))
                                   : LINK_NONE);
        nodes[base + lane] = c;
        meta[base + lane] = meta_pack(m_sq(ocm), 3 - m_turn(lm));
    }
    if (lane == 0) {
        meta[leaf] = lm | ((uint32_t)nch << 11) | ((uint32_t)e << 18);
        v.nexp[g] = e + 1;
        v.bval[(size_t)g * 2 * v.E + e] = val;
    }
    ab += 20ull * nch + 8 + 20ull * nch + 12 + 32ull * plen;
    // this walk's UCB-cache stores to path nodes come before the read-modify-write
    return backup_path(nodes, path_reg, plen, val, copies, lane, true);
}

// k_play's forced searches (rvz_play_args.skip_forced_roots): the search's
// batches E (0: the path is off), simulations S and batch size B
struct Forced {
    int E, S, B;
};

// A search whose root (not over) has L >= E - 1 legal moves, whole, in one step: batch 0 ends on
// the root, batch k >= 1 goes whole to child k - 1 (N == 0 scores inf, mcts.py:96-97; §2.13), so
// the visit counts are known before any NN output: min(B, S - k B) on child k - 1 for
// k = 1 .. E - 1, S on the root. The act reads the children's N, the root's meta word and
// root_legal only, and the tree is dropped after it: the priors (0 here) and every W stay unread,
// so neither the root's NN row nor the root noise is needed. Lane s = square s writes child
// popcount(rl below s), the order expand_backup_phase gives the children. With a carried root
// the children take the links memo_expand_backup would give them, and a visited child with a
// link is expanded from the previous tree as select_phase's walk would (its block, its value in
// bval), so that the act's carry names it and the next search gets its output without a row;
// blocks e0 .. e0 + E - 1 at most, this search's half of the pool.
// Returns the rows the search left out, counted as the batch-by-batch search would have met
// them: the children's rows between the first and the last batch, + 256 for the root's own row.
// Out of line, arguments by value: the callers' register allocation is that of the code
// without it.
template <int BS>
__device__ __noinline__ int forced_search(const View& v, int g, int lane, int side,
                                          uint32_t root_meta, uint64_t rl, int half,
                                          uint32_t carry, Forced fz) {
    constexpr int NSQ = Geo<BS>::NSQ;
    Node* nodes = v.nodes + (size_t)g * v.M;
    uint32_t* meta = v.meta + (size_t)g * v.M;
    const int L = __popcll(rl), nv = fz.E - 1;   // children; visited children (nv <= L)
    const int e0 = half * v.E, base = 1 + e0 * NSQ;
    const bool linked_root = v.memo && link_ok(carry);
    const bool mine = lane < NSQ && ((rl >> lane) & 1ull);
    const int idx = __popcll(rl & ((1ull << lane) - 1ull));
    if (base + NSQ > v.M) {
        if (lane == 0) atomicOr(v.err, ERR_POOL);
        return 0;
    }
    uint32_t lk = LINK_NONE;   // the child's node in the previous tree, if expanded there
    if (linked_root && mine) {
        const int oc = 1 + link_block(carry) * NSQ + idx;
        const uint32_t ocm = meta[oc];
        if (m_nchild(ocm) > 0 && !m_term(ocm)) lk = link_pack(oc, m_nchild(ocm), m_block(ocm));
    }
    const bool visited = mine && idx < nv;
    uint64_t lmask = __ballot(visited && link_ok(lk));
    if (1 + (e0 + 1 + __popcll(lmask)) * NSQ > v.M) {
        if (lane == 0) atomicOr(v.err, ERR_POOL);
        lmask = 0ull;
    }
    const bool expd = (lmask >> lane) & 1ull;
    const int ce = e0 + 1 + __popcll(lmask & ((1ull << lane) - 1ull));   // an expanded child's block
    if (mine) {
        Node c;
        c.n = visited ? min(fz.B, fz.S - (idx + 1) * fz.B) : 0;
        c.w = 0.0f; c.p = 0.0f; c.c = __uint_as_float(LINK_NONE);
        nodes[base + idx] = c;
        uint32_t cm = meta_pack(lane, 3 - side);
        if (expd) cm |= ((uint32_t)link_nchild(lk) << 11) | ((uint32_t)ce << 18);
        meta[base + idx] = cm;
    }
    int e = e0 + 1;
    for (uint64_t rest = lmask; rest != 0ull; rest &= rest - 1ull, ++e) {
        // memo_expand_backup's expansion of the child at square s into block e
        const int s = __ffsll((unsigned long long)rest) - 1;
        const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)lk, s);
        const int nch = link_nchild(l), ob = 1 + link_block(l) * NSQ, nb = 1 + e * NSQ;
        if (lane < nch) {
            const Node oc = nodes[ob + lane];
            const uint32_t ocm = meta[ob + lane];
            Node c;
            c.n = 0; c.w = 0.0f; c.p = oc.p;
            c.c = __uint_as_float(m_nchild(ocm) > 0 && !m_term(ocm)
                                      ? link_pack(ob + lane, m_nchild(ocm), m_block(ocm))
                                      : LINK_NONE);
            nodes[nb + lane] = c;
            meta[nb + lane] = meta_pack(m_sq(ocm), side);
        }
        if (lane == 0)
            v.bval[(size_t)g * 2 * v.E + e] = v.bval[(size_t)g * 2 * v.E + link_block(l)];
    }
    if (lane == 0) {
        Node r;
        r.n = fz.S; r.w = 0.0f; r.p = 1.0f; r.c = __int_as_float(0x7fc00000);
        nodes[0] = r;
        meta[0] = root_meta | ((uint32_t)L << 11) | ((uint32_t)e0 << 18);
        v.nexp[g] = e;
        v.pend[g] = 0;
        v.plen[g] = 0;
    }
    // the act reads the root, its children and their meta words back in this wave
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    return __popcll(__ballot(mine && idx < nv - 1 && !link_ok(lk))) + (linked_root ? 0 : 256);
}

// select: mcts.py:348-386 for one batch of `bsz` traversals + _process_batch pass 1 (:561-585).
// root / root_meta / root_n were loaded (or produced by the expand phase) by the caller.
// fz (k_play; fz.E > 0 at a search's first batch only): a root with at least fz.E - 1 legal
// moves is searched whole by forced_search; returns -2 - its count, nothing is queued.
template <int BS, typename XT>
__device__ __forceinline__ int select_phase(const View& v, int g, int lane, int first, int bsz,
                                             int eb,
                                             const GameS& root, uint32_t root_meta, int root_n,
                                             uint32_t carry,
                                             XT* __restrict__ leaf_x, int32_t* __restrict__ need,
                                             unsigned long long& ab,
                                             uint64_t* leaf_bits = nullptr,
                                             bool unread = false, Forced fz = Forced{0, 0, 0}) {
    constexpr int NSQ = Geo<BS>::NSQ;
    Node* nodes = v.nodes + (size_t)g * v.M;
    uint32_t* meta = v.meta + (size_t)g * v.M;
    if (first) {  // new root (mcts.py:334-341): prior 1.0, turn = side to move
        root_meta = meta_pack(0, root.side);
        root_n = 0;
        // memo: this search's blocks go to the half the previous tree (where the carried node
        // lives) does not use; without a carried node, half 0
        const int half = (v.memo && link_ok(carry) && (link_node(carry) - 1) / NSQ < v.E) ? 1 : 0;
        if (lane == 0) {
            Node r;
            r.n = 0; r.w = 0.0f; r.p = 1.0f; r.c = __int_as_float(0x7fc00000);
            nodes[0] = r;
            meta[0] = root_meta;
            v.nexp[g] = half * v.E;
        }
        const uint64_t rl = root.over ? 0ull : legal_wave<BS>(mine(root), theirs(root), lane);
        if (lane == 0) v.root_legal[g] = rl;
        if (fz.E > 0 && !root.over && __popcll(rl) >= fz.E - 1)
            return -2 - forced_search<BS>(v, g, lane, root.side, root_meta, rl, half, carry, fz);
        if (v.noise_eps > 0.0f && rl != 0ull) root_noise_sample(v, g, lane, root, rl);
        ab += 20 + 8;
    }
    ab += 32 + 8;  // game state, root meta + N
    int copies = 0, plen = 0, path_reg = 0;
    if (!root.over) {
        int remaining = bsz;
        for (;;) {
            WALK_STAT(0, 1);
            WT_NOW(tw0);
            GameS sim = root;
            int depth = 0, node = 0, parent_n = root_n;
            uint32_t m = root_meta;
            // memo link of the node the walk ends on (the root's: the carried node)
            uint32_t lk = first ? carry : LINK_NONE;
            path_reg = 0;  // lane 0 holds the root
            // per level d (in lane d): the chosen child's index, its turn for scoring, the best
            // other child's score and index (-1: none) — the terminal fast path below
            int fp_ci = 0, fp_b = -1, fp_turn = 0;
            float fp_sb = 0.0f;
            bool truncated = false;
            // the move of level d (lane d): replayed on `sim` only if the walk ends on a leaf
            // that needs the position (a known terminal does not)
            int fp_sq = 0;
            for (;;) {
                const int nch = m_nchild(m);
                if (m_term(m) || nch == 0) break;  // while node.expanded() and not terminal
                const int base = 1 + m_block(m) * NSQ;
                // one round trip per level: the children's node rows and meta words together
                Node c;
                uint32_t cm = 0;
                if (lane < nch) {
                    c = nodes[base + lane];
                    cm = meta[base + lane];
                } else {
                    c.n = 0; c.w = 0.0f; c.p = 0.0f; c.c = 0.0f;
                }
                float score = 0.0f;
                bool wrote = false;
                if (lane < nch) {
                    if (c.n == 0) {
                        score = INFINITY;
                    } else if (!isnan(c.c)) {
                        score = c.c;
                    } else {
                        const float sq_np = sqrt_count(parent_n);
                        score = ucb_score(c, sq_np, 3 - m_turn(m), v.cpuct);
                        nodes[base + lane].c = score;
                        wrote = true;
                    }
                }
                WALK_STAT(1, 1);
                const int ci = wave_argmax_first(score, lane < nch, lane);
                const int bsib = wave_argmax_first(score, lane < nch && lane != ci, lane);
                const float sbs = lane_bcast(score, bsib);
                const int turn_c = 3 - m_turn(m);
                if (v.stats) ab += 16ull * nch + 4ull * nch + 4ull * __popcll(__ballot(wrote));
                node = base + ci;
                m = (uint32_t)lane_bcast((int)cm, ci);
                parent_n = lane_bcast(c.n, ci);
                if (v.memo) lk = (uint32_t)lane_bcast(__float_as_int(c.c), ci);
                ++depth;
                if (depth >= PATH_CAP) {  // unreachable when ceil(sims/batch) <= 64 (checked)
                    if (lane == 0) atomicOr(v.err, ERR_PATH);
                    depth = PATH_CAP - 1;
                    truncated = true;
                    break;
                }
                if (lane == depth) {
                    path_reg = node;
                    fp_sq = m_sq(m);
                    fp_ci = ci;
                    fp_b = nch > 1 ? bsib : -1;
                    fp_sb = sbs;
                    fp_turn = turn_c;
                }
            }
            WT_ADD(1, tw0);
            if (m_term(m)) {  // known terminal: back up its value at once (mcts.py:364-366)
                WT_NOW(tb0);
                root_n = backup_path(nodes, path_reg, depth + 1, m_tv(m), 1, lane, true);
                WALK_STAT(2, 1);
                WT_ADD(2, tb0);
                ab += 32ull * (depth + 1);
                if (--remaining == 0) break;
                if (truncated) continue;
                // Fast path for the next traversals while they provably reach the same terminal.
                // A backup invalidates only the path nodes' cached scores (mcts.py:639-640), so
                // every other child on the path keeps the score this walk saw; the next walk
                // takes the same child at level d iff the path child's fresh score (the reference
                // formula on its backed-up N, W and its parent's N) beats the best other child
                // under the first-index tie-break. Register copies of the path nodes replace the
                // re-walk and its backup; the path is written back once (N, W, cache invalid)
                // before the walk resumes at the first divergence or the batch ends.
                WT_NOW(tf0);
                const float tv = m_tv(m);
                Node pn;
                if (lane <= depth) pn = nodes[path_reg];
                int fn = lane <= depth ? pn.n : 0;
                float fw = lane <= depth ? pn.w : 0.0f;
                const float fpr = lane <= depth ? pn.p : 0.0f;
                int hits = 0;
                for (;;) {
                    const int par_n = __shfl_up(fn, 1);
                    bool hold = true;
                    if (lane >= 1 && lane <= depth && fp_b >= 0) {
                        Node cn;
                        cn.n = fn; cn.w = fw; cn.p = fpr; cn.c = 0.0f;
                        const float sc = ucb_score(cn, sqrt_count(par_n), fp_turn,
                                                   v.cpuct);
                        const uint32_t ks = score_key(sc), kb = score_key(fp_sb);
                        hold = ks > kb || (ks == kb && fp_ci < fp_b);
                    }
                    if (__ballot(!hold) != 0ull) break;
                    if (lane <= depth) {   // _backpropagate_path of the same terminal value
                        fw = fw + (((depth - lane) & 1) ? -tv : tv);
                        fn += 1;
                    }
                    ++hits;
                    WALK_STAT(3, 1);
                    if (--remaining == 0) break;
                }
                if (hits) {
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                    if (lane <= depth) {
                        Node nd;
                        nd.n = fn; nd.w = fw; nd.p = fpr; nd.c = __int_as_float(0x7fc00000);
                        nodes[path_reg] = nd;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                    root_n = __builtin_amdgcn_readlane(fn, 0);
                }
                ab += 32ull * (depth + 1);
                WT_ADD(3, tf0);
                if (remaining == 0) break;
                continue;
            }
            if (v.memo && link_ok(lk) && !truncated) {
                // the previous search evaluated this position: expand it from that output, no
                // NN row (the position has legal moves, so it is not terminal)
                const int rn = memo_expand_backup<BS>(v, g, lane, node, m, path_reg, depth + 1,
                                                      lk, remaining, ab);
                if (rn >= 0) root_n = rn;
                break;
            }
            if (unread && depth == 1 && parent_n == 0) {
                // k_play's unread row: a fresh child of a root with at least as many legal moves
                // as the search has batches after the first. Every one of those batches goes
                // whole to the next unvisited child (N == 0 scores inf, mcts.py:96-97), so no
                // selection of this search reads the child's value or its children's priors, and
                // the tree is dropped after the act: the visits alone are backed up
                // (backup_visits_only's arithmetic, now; lane 0 the root, lane 1 the child) and
                // no row is queued. pend stays 0 (the caller's expand cleared it).
                if (lane <= 1) nodes[path_reg].n += remaining;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                return -1;
            }
            WT_NOW(tl0);
            // the leaf's position: the path's moves on the root's game (a truncated path, an
            // error already flagged, replays its first PATH_CAP - 1 moves)
            for (int d = 1; d <= depth; ++d)
                make_move_wave<BS>(sim, __builtin_amdgcn_readlane(fp_sq, d), lane);
            // pass 1: valid moves of the leaf's simulated game
            const uint64_t V = legal_wave<BS>(mine(sim), theirs(sim), lane);
            if (V == 0ull) {  // terminal, BLACK-absolute value from get_winner() (mcts.py:567-579)
                const int w = sim.over ? sim.winner : -1;
                const uint32_t code = w == 1 ? 1u : (w == 2 ? 2u : 0u);
                if (lane == 0) meta[node] = m | (1u << 8) | (code << 9);
                WALK_STAT(4, 1);
                backup_path(nodes, path_reg, depth + 1, w == 1 ? 1.0f : (w == 2 ? -1.0f : 0.0f),
                            remaining, lane, true);
                ab += 4 + 32ull * (depth + 1);
                break;
            }
            // queue `remaining` identical copies for the NN: encode get_canonical_state() planes
            copies = remaining;
            plen = depth + 1;
            // compacted batch: the next free row of batch eb (one atomic per live game)
            int r = g;
            if (v.live) {   // striped counters: at most STRIPE contending waves per address
                const int s = g / RVZ_LIVE_STRIPE;
                if (lane == 0)
                    r = s * RVZ_LIVE_STRIPE +
                        atomicAdd(v.live + ((size_t)eb * v.NS + s) * RVZ_LIVE_PITCH, 1);
                r = __builtin_amdgcn_readlane(r, 0);
                if (lane == 0) v.row_of[g] = r;
            }
            if (leaf_bits) {   // k_play: the planes as bitboards (P, O, V) in LDS
                if (lane == 0) {
                    leaf_bits[0] = mine(sim);
                    leaf_bits[1] = theirs(sim);
                    leaf_bits[2] = V;
                }
            } else if (lane < NSQ) {
                XT* row = leaf_x + (size_t)r * 3 * NSQ;
                const uint64_t P = mine(sim), O = theirs(sim);
                row[lane] = (XT)(float)((P >> lane) & 1ull);
                row[NSQ + lane] = (XT)(float)((O >> lane) & 1ull);
                row[2 * NSQ + lane] = (XT)(float)((V >> lane) & 1ull);
            }
            if (lane < plen) v.path[g * PATH_CAP + lane] = path_reg;
            if (lane == 0) {
                v.leaf_legal[g] = V;
                v.leaf_meta[g] = m;
            }
            WT_ADD(4, tl0);
            ab += 3ull * NSQ * sizeof(XT) + 4ull * plen + 12;
            break;
        }
    }
    if (lane == 0) {
        need[g] = copies;
        v.pend[g] = copies;
        v.plen[g] = plen;
    }
    ab += 12;
    return copies;   // the queued copies of the batch's NN row (0: no row; -1: a row left unread)
}

// k_play's ahead rows: the next NN row game g's search will ask for after the one
// it has queued, when that is known now. The game has selected batches 0 .. k - 1 of E. With an
// expanded root of fewer than E - 1 children, batch b = 1 .. nchild goes whole to child b - 1
// (N == 0 scores inf and select_phase's argmax takes the first, mcts.py:96-97), whatever the
// earlier children's values were; a child the memo links needs no row (memo_expand_backup) and a
// terminal one none either, and both take their batch whole. So the row is that of the first
// child at index >= k - 1 that is unvisited, unlinked and has legal moves: the children's rows are
// read as select_phase's level reads them, the move and the legal mask are select_phase's leaf
// code on the root's game. Returns false when there is no such child; else the child's canonical
// (P, O, V), the key of its row. Nothing is written: a wrong answer costs a row, never a result.
template <int BS>
__device__ __forceinline__ bool ahead_child(const View& v, int g, int k, int E, int lane,
                                            uint64_t& P, uint64_t& O, uint64_t& V) {
    constexpr int NSQ = Geo<BS>::NSQ;
    const Node* nodes = v.nodes + (size_t)g * v.M;
    const uint32_t* meta = v.meta + (size_t)g * v.M;
    const uint32_t m0 = meta[0];
    const int nch = m_nchild(m0);
    if (m_term(m0) || nch == 0 || nch >= E - 1 || k < 1 || k > nch) return false;
    const int base = 1 + m_block(m0) * NSQ;
    Node c;
    uint32_t cm = 0;
    c.n = 1; c.c = 0.0f;
    if (lane < nch) {
        c = nodes[base + lane];
        cm = meta[base + lane];
    }
    const bool fresh = lane < nch && lane >= k - 1 && c.n == 0 &&
                       !(v.memo && link_ok(__float_as_uint(c.c)));
    const GameS root = load_game(v, g);
    if (root.over) return false;
    for (uint64_t rest = __ballot(fresh); rest != 0ull; rest &= rest - 1ull) {
        const int ci = __ffsll((unsigned long long)rest) - 1;
        GameS sim = root;
        make_move_wave<BS>(sim, m_sq((uint32_t)lane_bcast((int)cm, ci)), lane);
        V = legal_wave<BS>(mine(sim), theirs(sim), lane);
        if (V != 0ull) {
            P = mine(sim);
            O = theirs(sim);
            return true;
        }
    }
    return false;
}

// Dense visit count of square `lane` at the root: the root's children are the set bits of the
// search root's legal mask in ascending order (expand inserts them row-major).
template <int BS>
__device__ __forceinline__ int root_visits(const View& v, int g, int lane) {
    constexpr int NSQ = Geo<BS>::NSQ;
    const Node* nodes = v.nodes + (size_t)g * v.M;
    const uint32_t m0 = v.meta[(size_t)g * v.M];
    const uint64_t V = v.root_legal[g];
    const int nch = m_nchild(m0);
    if (nch == 0 || lane >= NSQ) return 0;
    if (!((V >> lane) & 1ull)) return 0;
    const int idx = __popcll(V & ((1ull << lane) - 1ull));
    return nodes[1 + m_block(m0) * NSQ + idx].n;
}

// numpy `arr ** e` for float64 (fast_scalar_power paths, else the correctly rounded power; NumPy's
// general power is host-dependent, csrc/rvz_pow.hip.h)
__device__ __forceinline__ double np_power(double x, double e) {
    if (e == 1.0) return x;
    if (e == 2.0) return x * x;
    if (e == 0.5) return sqrt(x);
    if (e == -1.0) return 1.0 / x;
    if (e == 0.0) return 1.0;
    return rvz_pow::pow_cr(x, e);
}

// get_action_probs' tail (mcts.py:656-692) for one row of visit counts, one wave: n = the count of
// square `lane` (lanes >= NSQ: ignored), npass the pass index's count (total below 2^31).
// Normalise, p ** (1 / temperature) renormalised in numpy's pairwise order, then the first maximum
// (temperature 0 or an all-zero row) or np.random.choice's cdf / searchsorted with one uniform
// value. draw() is called (by every lane, wave-uniformly) only when the row needs that value, so
// a row acting at temperature 0 reads and consumes none. s: NPOL doubles of this wave's LDS.
// Returns idx (wave-uniform); p (lane's square) and ppass are the row of get_action_probs.
// act_game (k_act, k_play) and k_action_probs (rvz_action_probs) both select through it.
template <int BS, class Draw>
__device__ __forceinline__ int select_action(int n, int npass, int lane, double* s,
                                             double temperature, Draw&& draw, double& p,
                                             double& ppass, int& drew) {
    constexpr int NSQ = Geo<BS>::NSQ, NPOL = Geo<BS>::NPOL;
    constexpr int NMAIN = NPOL - NPOL % 8;
    const int total = wave_sum_i(lane < NSQ ? n : 0) + npass;
    p = (lane < NSQ && total > 0) ? (double)n / (double)total : 0.0;
    ppass = npass != 0 ? (double)npass / (double)total : 0.0;
    if (temperature > 0.0 && (__any(p != 0.0) || ppass != 0.0)) {
        const double ex = 1.0 / temperature;
        const double t = lane < NSQ ? np_power(p, ex) : 0.0;
        const double tp = np_power(ppass, ex);
        // np.sum in numpy's pairwise order: 8 accumulators over the first NMAIN entries, then tail
        if (lane < NSQ) s[lane] = t;
        if (lane == 0) s[NSQ] = tp;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
        double r = 0.0;
        if (lane < 8) {
            r = s[lane];
            for (int i = 8 + lane; i < NMAIN; i += 8) r += s[i];
        }
        const double r0 = __shfl(r, 0), r1 = __shfl(r, 1), r2 = __shfl(r, 2), r3 = __shfl(r, 3);
        const double r4 = __shfl(r, 4), r5 = __shfl(r, 5), r6 = __shfl(r, 6), r7 = __shfl(r, 7);
        double sum = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        for (int i = NMAIN; i < NPOL; ++i) sum += s[i];
        p = t / sum;
        ppass = tp / sum;
        __builtin_amdgcn_wave_barrier();
    }
    const bool all_zero = !__any(lane < NSQ && p != 0.0) && ppass == 0.0;
    if (lane < NSQ) s[lane] = p;
    if (lane == 0) s[NSQ] = ppass;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
    int idx = 0;
    drew = 0;
    if (temperature == 0.0 || all_zero) {  // np.argmax: first maximum
        if (lane == 0) {
            double best = s[0];
            for (int i = 1; i < NPOL; ++i)
                if (s[i] > best) { best = s[i]; idx = i; }
        }
    } else {  // np.random.choice(NPOL, p=p): cumsum, /= last, searchsorted(u, 'right')
        const double u = draw();
        drew = 1;
        if (lane == 0) {
            double acc = 0.0;  // cdf[-1]: the same sequential adds as p.cumsum()
            for (int i = 0; i < NPOL; ++i) acc += s[i];
            const double last = acc;
            acc = 0.0;
            for (int i = 0; i < NPOL; ++i) {
                acc += s[i];
                if (acc / last <= u) idx = i + 1;  // count of cdf entries <= u
            }
        }
    }
    return __shfl(idx, 0);
}

// act for one game (one wave): the search's pending expand (expand 1) or visit-count backup
// (expand 2), then get_action_probs' tail and the move; returns the sampled index (-2: the game
// was over). s: NPOL + 7 doubles of this wave's LDS.
template <int BS>
__device__ __forceinline__ int act_game(const View& v, int g, int lane, double* s, int expand,
                                        const float* __restrict__ policy, int is_logits,
                                        const float* __restrict__ value, double temperature,
                                        const double* __restrict__ uo, int apply,
                                        int32_t* __restrict__ out_idx, double* __restrict__ out_p,
                                        bool* over_after = nullptr) {
    constexpr int NSQ = Geo<BS>::NSQ, NPOL = Geo<BS>::NPOL;
    unsigned long long ab = 0;
    if (expand == 1) {
        const ExpIn x = expand_load<BS>(v, g, lane, policy, value);
        expand_backup_phase<BS>(v, g, lane, x, is_logits, nullptr, ab);
    } else if (expand == 2) {
        backup_visits_only(v, g, lane, ab);
    }
    GameS gm = load_game(v, g);
    double* prow = out_p + (size_t)g * NPOL;
    if (gm.over) {
        if (lane < NSQ) prow[lane] = 0.0;
        if (lane == 0) {
            prow[NSQ] = 0.0;
            out_idx[g] = -2;
            if (v.memo) v.carry[g] = LINK_NONE;
            if (v.stats) v.stats[(size_t)v.G + g] += ab + 32 + 8ull * NPOL + 4;
        }
        if (over_after) *over_after = true;
        return -2;
    }
    // the schedule, keyed by the root's disc count: wave-uniform (one wave, one game), and
    // nothing of it runs with the schedule off
    if (v.sched_from > 0 && __popcll(gm.black | gm.white) >= v.sched_from)
        temperature = v.sched_late;
    const int n = root_visits<BS>(v, g, lane);
    double p, ppass;
    int drew;
    const int idx = select_action<BS>(n, 0, lane, s, temperature, [&]() -> double {
        if (uo) return uo[g];
        const int pos = v.rng_pos[g];
        double u = 0.0;
        if (pos >= RNG_DRAWS) {
            if (lane == 0) atomicOr(v.err, ERR_RNG);
        } else {
            u = v.rng_u[(size_t)g * RNG_DRAWS + pos];
        }
        if (lane == 0) v.rng_pos[g] = pos + 1;
        return u;
    }, p, ppass, drew);
    if (lane < NSQ) prow[lane] = p;
    if (lane == 0) {
        prow[NSQ] = ppass;
        out_idx[g] = idx;
    }
    if (apply) {
        make_move_wave<BS>(gm, idx == NSQ ? -1 : idx, lane);  // (-1, -1) for the pass index
        if (lane == 0) store_game(v, g, gm);
    }
    if (over_after) *over_after = gm.over != 0;
    if (v.memo && lane == 0) {
        // the child the move went to (its position is the next search's root), if this search
        // expanded it: the next search's root takes that expansion's NN output (memo_expand_backup)
        uint32_t cl = LINK_NONE;
        const uint32_t m0 = v.meta[(size_t)g * v.M];
        const uint64_t V = v.root_legal[g];
        if (apply && idx < NSQ && m_nchild(m0) > 0 && ((V >> idx) & 1ull)) {
            const int c = 1 + m_block(m0) * NSQ + __popcll(V & ((1ull << idx) - 1ull));
            const uint32_t cm = v.meta[(size_t)g * v.M + c];
            if (m_nchild(cm) > 0 && !m_term(cm)) cl = link_pack(c, m_nchild(cm), m_block(cm));
        }
        v.carry[g] = cl;
    }
    if (v.stats && lane == 0)  // state r/(w), root meta + children N, p row + idx, rng
        v.stats[(size_t)v.G + g] += ab + 32ull + (apply ? 32 : 0) + 12 +
                                    4ull * m_nchild(v.meta[(size_t)g * v.M]) + 8ull * NPOL + 4 + 16;
    return idx;
}

// reset: new game (board.py:25-39) + np.random.seed(seed) random_sample() stream.
// a fresh game g seeded with `seed` (np.random.seed semantics): MT19937 init, its first draws,
// the start position, or with an opening pool set (rvz_env_openings) the pool row the seed picks
// (one wave; k is the wave's 624-word key scratch in LDS)
template <int BS>
__device__ __forceinline__ void reset_game(const View& v, int g, int lane, uint32_t seed,
                                           uint32_t* k) {
    if (lane == 0) {  // mt19937_seed (init_genrand): inherently sequential
        v.seed32[g] = seed;   // the key of the game's root noise (rvz_search_root_noise)
        uint32_t sd = seed;
        for (int pos = 0; pos < 624; ++pos) {
            k[pos] = sd;
            sd = 1812433253u * (sd ^ (sd >> 30)) + (uint32_t)(pos + 1);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // First generation: words 0..127 only need the initial key (i + 397 < 624 for i < 227).
    auto word = [&](int i) -> uint32_t {
        const uint32_t y = (k[i] & 0x80000000u) | (k[i + 1] & 0x7fffffffu);
        uint32_t x = k[i + 397] ^ (y >> 1) ^ ((0u - (y & 1u)) & 0x9908b0dfu);
        x ^= (x >> 11);
        x ^= (x << 7) & 0x9d2c5680u;
        x ^= (x << 15) & 0xefc60000u;
        x ^= (x >> 18);
        return x;
    };
    const uint32_t a = word(2 * lane) >> 5, b = word(2 * lane + 1) >> 6;
    v.rng_u[(size_t)g * RNG_DRAWS + lane] = ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
    if (lane == 0) {
        GameS st;
        st.black = Geo<BS>::START_BLACK;
        st.white = Geo<BS>::START_WHITE;
        st.side = 1; st.over = 0; st.winner = -1; st.passed = 0;
        if (v.open_n > 0) {   // a row of the opening pool, picked by the seed (no draw consumed)
            const int i = opening_index(seed, v.open_salt, v.open_n);
            st.black = v.open_black[i];
            st.white = v.open_white[i];
            st.side = v.open_side[i];
        }
        store_game(v, g, st);
        v.rng_pos[g] = 0;
        v.pend[g] = 0;
        v.carry[g] = LINK_NONE;   // a new game: nothing to carry into its first search
    }
}

}  // namespace
}  // namespace rvz
