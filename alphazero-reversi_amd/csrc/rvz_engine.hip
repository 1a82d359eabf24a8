// rvz_engine.hip — batched Reversi env + lockstep reference-semantics PUCT for gfx950 (MI355X),
// exported through the C-ABI in include/rvz.h. This unit: the pull-style kernels and the C-ABI but
// for the fused play (csrc/rvz_play.hip); the search's device code is csrc/rvz_search.hip.h.
//
// Layout (HBM, per engine of G games):
//   env    black[G], white[G] (u64), status[G][4] (side, over, winner, passed)
//   tree   nodes[G][M] {N i32, W f32, P f32, C f32}, meta[G][M] u32, M = 1 + E*S*S,
//          E = ceil(sims / batch) = expansions per search; node 0 = root, expansion e of a search
//          owns the child block [1 + e*S*S, 1 + (e+1)*S*S), children in row-major square order.
//   search path[G][64] i32, pend[G] (queued copies), plen[G], leaf_legal[G] u64, nexp[G]
//   rng    u[G][64] f64: np.random.random_sample() stream of each game's seed, pos[G]
//
// One wavefront per game in every search kernel: lane i owns child i (UCB, expansion) or
// square i (planes, visits, policy), so a 64-square board is exactly one wave.
//
// Exactness notes (mirrored and checked by oracle/rvz_oracle.c, which keeps the literal rules):
//  * Within a batch every traversal of a game follows the same path (UCB scores are cached and only
//    invalidated by a backup of that node, mcts.py:99-113,639-640; unvisited children score +inf,
//    mcts.py:96-97), unless a traversal ends on an already-known terminal, which is backed up at
//    once (mcts.py:364-366). select therefore walks once per terminal hit plus once for the
//    queued leaf, and backs the NN value up `copies` times (B sequential fp32 adds).
//  * Virtual loss is always 0 when a score is computed (every traversal that scores starts from a
//    balanced tree), so u = c*P*sqrt(Np) / (1 + N).
//  * value_sum is float32 (NumPy>=2 promotion of the np.float32 NN value); terminal values are
//    small integers, exact in float32, so one float32 accumulator reproduces the Python mix.
//  * sqrt(Np) is the correctly rounded f32 sqrt of (float)n (sqrt_count): equal to math.sqrt in
//    double then the float32 cast (double rounding through >= 2p + 2 bits is innocuous for
//    sqrt; tests/test_gpu_numerics.py checks every n <= 4,000,000), at f32 cost.
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <vector>

#include "../../include/rvz.h"
#include "rvz_dirichlet.hip.h"
#include "rvz_engine_host.h"
#include "rvz_host.hip.h"
#include "rvz_philox.hip.h"
#include "rvz_rules.hip.h"
#include "rvz_search.hip.h"
#include "rvz_trace.h"

using namespace rvz;

namespace {

// rvz_policy_softmax: one wave per row, WPB rows per workgroup
template <int BS>
__global__ __launch_bounds__(256) void k_policy_softmax(int n, const float* __restrict__ logits,
                                                        float* __restrict__ probs) {
    constexpr int NSQ = Geo<BS>::NSQ, NPOL = Geo<BS>::NPOL;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (r >= n) return;
    const float* row = logits + (size_t)r * NPOL;
    const float2 p = policy_softmax<NSQ>(lane < NSQ ? row[lane] : 0.0f, row[NSQ], lane);
    if (lane < NSQ) probs[(size_t)r * NPOL + lane] = p.x;
    if (lane == 0) probs[(size_t)r * NPOL + NSQ] = p.y;
}

// One search round: the previous batch's expand + backup (when a submit is pending), then the
// next batch's selection, in one launch (one wave per game). Every load that does not depend on
// another is issued at the head.
// RVZ_STEP_WPE (experiments): amdgpu_waves_per_eu cap of k_step (e.g. 7 = 72 VGPRs)
#ifdef RVZ_STEP_WPE
#define RVZ_STEP_ATTR __attribute__((amdgpu_waves_per_eu(RVZ_STEP_WPE)))
#else
#define RVZ_STEP_ATTR
#endif
template <int BS, typename XT>
__global__ __launch_bounds__(256) RVZ_STEP_ATTR void k_step(View v, int expand, const float* __restrict__ policy,
                                              int is_logits, const float* __restrict__ value,
                                              int first, int bsz, int eb,
                                              XT* __restrict__ leaf_x,
                                              int32_t* __restrict__ need) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (g >= v.G) return;
    const GameS root = load_game(v, g);
    uint32_t root_meta = 0, carry = LINK_NONE;
    int root_n = 0;
    if (!first) {
        root_meta = v.meta[(size_t)g * v.M];
        root_n = v.nodes[(size_t)g * v.M].n;
    } else if (v.memo) {
        carry = v.carry[g];
    }
    unsigned long long ab_e = 0, ab_s = 0;
    WT_NOW(te0);
    if (expand) {
        const ExpIn x = expand_load<BS>(v, g, lane, policy, value);
        const int rn = expand_backup_phase<BS>(v, g, lane, x, is_logits, &root_meta, ab_e);
        if (rn >= 0) root_n = rn;
    }
    WT_ADD(0, te0);
    select_phase<BS, XT>(v, g, lane, first, bsz, eb, root, root_meta, root_n, carry, leaf_x, need,
                         ab_s);
    if (v.stats && lane == 0) v.stats[g] += ab_s + ab_e;  // per-game slot: no contention
}

template <int BS>
__global__ __launch_bounds__(256) void k_expand_backup(View v, int mode,
                                                       const float* __restrict__ policy,
                                                       int is_logits,
                                                       const float* __restrict__ value) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (g >= v.G) return;
    unsigned long long ab = 0;
    if (mode == 2) {
        backup_visits_only(v, g, lane, ab);
    } else {
        const ExpIn x = expand_load<BS>(v, g, lane, policy, value);
        expand_backup_phase<BS>(v, g, lane, x, is_logits, nullptr, ab);
    }
    if (v.stats && lane == 0) v.stats[2 * (size_t)v.G + g] += ab;
}

template <int BS>
__global__ __launch_bounds__(256) void k_visits(View v, int32_t* __restrict__ out) {
    constexpr int NSQ = Geo<BS>::NSQ, NPOL = Geo<BS>::NPOL;
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (g >= v.G) return;
    const int n = root_visits<BS>(v, g, lane);
    if (lane < NSQ) out[(size_t)g * NPOL + lane] = n;
    if (lane == 0) out[(size_t)g * NPOL + NSQ] = 0;  // no pass child is ever created
}

#ifndef RVZ_ACT_WPE
#define RVZ_ACT_WPE 6
#endif
// act: mcts.py:656-692 + self_play.py:98 (make_move of the sampled action); optionally preceded
// by the last batch's pending expand + backup.
template <int BS>
// 8x8: <= 80 VGPRs (6 waves per SIMD), so a k_act wave fits on a SIMD beside two trunk waves
// (2 x 216); the 6x6 form would spill under that cap
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(BS == 8 ? RVZ_ACT_WPE : 1))) void k_act(View v, int expand, const float* __restrict__ policy,
                                             int is_logits, const float* __restrict__ value,
                                             double temperature, const double* __restrict__ uo,
                                             int apply, int32_t* __restrict__ out_idx,
                                             double* __restrict__ out_p) {
    constexpr int NPOL = Geo<BS>::NPOL;
    __shared__ double sp[WPB][NPOL + 7];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int g = blockIdx.x * WPB + wid;
    if (g >= v.G) return;
    // the search's leaf batches are all consumed (their NN calls precede this launch); the rows
    // of a skipped last batch (expand == 2, rvz_search_skip) were handed out but not evaluated
    if (v.live && lane == 0) {
        const int counted = expand == 2 ? (v.E - 1) * v.NS : v.E * v.NS;
        for (int i = g; i < v.E * v.NS; i += v.G) {
            const int c = v.live[(size_t)i * RVZ_LIVE_PITCH];
            if (c && i < counted) atomicAdd(v.live_total, (unsigned long long)c);
            v.live[(size_t)i * RVZ_LIVE_PITCH] = 0;
        }
    }
    act_game<BS>(v, g, lane, sp[wid], expand, policy, is_logits, value, temperature, uo, apply,
                 out_idx, out_p);
}

// rvz_action_probs: select_action on caller arrays, one wave per row. A row holding a negative
// count writes out_idx = -3 and a zero row (drew 0).
template <int BS>
__global__ __launch_bounds__(256) void k_action_probs(int n_rows, const int32_t* __restrict__ visits,
                                                      const double* __restrict__ temperature,
                                                      const double* __restrict__ u,
                                                      int32_t* __restrict__ out_idx,
                                                      double* __restrict__ out_p,
                                                      int32_t* __restrict__ out_drew) {
    constexpr int NSQ = Geo<BS>::NSQ, NPOL = Geo<BS>::NPOL;
    __shared__ double sp[WPB][NPOL + 7];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int r = blockIdx.x * WPB + wid;
    if (r >= n_rows) return;
    const int32_t* vrow = visits + (size_t)r * NPOL;
    double* prow = out_p + (size_t)r * NPOL;
    const int n = lane < NSQ ? vrow[lane] : 0;
    const int npass = vrow[NSQ];
    double p = 0.0, ppass = 0.0;
    int idx = -3, drew = 0;
    if (!__any(n < 0) && npass >= 0)
        idx = select_action<BS>(n, npass, lane, sp[wid], temperature[r],
                                [&]() -> double { return u[r]; }, p, ppass, drew);
    if (lane < NSQ) prow[lane] = p;
    if (lane == 0) {
        prow[NSQ] = ppass;
        out_idx[r] = idx;
        if (out_drew) out_drew[r] = drew;
    }
}

template <int BS>
__global__ __launch_bounds__(256) void k_reset(View v, const uint32_t* __restrict__ seeds,
                                               const uint8_t* __restrict__ mask) {
    __shared__ uint32_t key[WPB][624];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int g = blockIdx.x * WPB + wid;
    if (g >= v.G) return;
    if (mask && !mask[g]) return;
    reset_game<BS>(v, g, lane, seeds[g], key[wid]);
}

// The self-play driver's per-ply bookkeeping in one launch (SelfPlayRunner, self_play.py:80-101
// run back to back): plies[g] += (idx[g] >= 0) (a move was committed); when `reset`, a game that
// just ended counts in done[g], takes its slot's next seed (seeds[g] += stride) and restarts from
// the start position with it. Per-game counters: no contended atomics; the totals are summed
// when read.
template <int BS>
__global__ __launch_bounds__(256) void k_autoreset(View v, const int32_t* __restrict__ idx,
                                                   int64_t* __restrict__ seeds, int64_t stride,
                                                   int64_t* __restrict__ plies,
                                                   int64_t* __restrict__ done, int reset) {
    __shared__ uint32_t key[WPB][624];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int g = blockIdx.x * WPB + wid;
    if (g >= v.G) return;
    if (lane == 0 && idx[g] >= 0) plies[g] += 1;
    if (!reset || !v.status[4 * g + 1]) return;
    int64_t sd = 0;
    if (lane == 0) {
        done[g] += 1;
        sd = seeds[g] + stride;
        seeds[g] = sd;
    }
    sd = __shfl(sd, 0);
    reset_game<BS>(v, g, lane, (uint32_t)(sd & 0xFFFFFFFFll), key[wid]);
}

// rvz_dirichlet_noise's exhaustion flag: the call has no engine, so its ERR_NOISE goes to this
// word of the device, which rvz_check of any engine of the device reports and clears
__device__ int32_t g_noise_err;

// rvz_dirichlet_noise: one wave per row, WPB rows per workgroup
template <int BS>
__global__ __launch_bounds__(256) void k_dirichlet(int n, const uint64_t* __restrict__ legal,
                                                   const uint32_t* __restrict__ seed32,
                                                   const int32_t* __restrict__ tag, uint32_t salt,
                                                   float alpha, float* __restrict__ out,
                                                   uint32_t* __restrict__ out_bits) {
    constexpr int NSQ = Geo<BS>::NSQ, NPOL = Geo<BS>::NPOL;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (r >= n) return;
    const uint64_t V = legal[r] & Geo<BS>::FULL;
    const uint32_t sd = seed32[r], tg = (uint32_t)tag[r];
    const float eta = dirichlet_eta(sd, salt, tg, alpha, V, lane, &g_noise_err);
    if (lane < NSQ) out[(size_t)r * NPOL + lane] = eta;
    if (lane == 0) out[(size_t)r * NPOL + NSQ] = 0.0f;
    if (out_bits && lane < NSQ)
        reinterpret_cast<uint4*>(out_bits)[(size_t)r * NSQ + lane] =
            philox4x32_10(sd, salt, 0u, (uint32_t)lane, tg, 0u);
}

// ---- board kernels on caller arrays (one thread per board) --------------------------------------
template <int BS>
__global__ void k_board_legal(int n, const uint64_t* __restrict__ black,
                              const uint64_t* __restrict__ white, const int32_t* __restrict__ status,
                              uint64_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int side = status[4 * i];
    const uint64_t P = side == 1 ? black[i] : white[i], O = side == 1 ? white[i] : black[i];
    out[i] = legal<BS>(P, O);
}

// rvz_env_openings' row rules, a thread per pool row: *first_bad ends as the lowest row with
// overlapping discs, a bit at or above S*S, a side other than 1 | 2 or a mover without a legal
// square (the caller sets it to INT_MAX)
template <int BS>
__global__ void k_openings_validate(int n, const uint64_t* __restrict__ black,
                                    const uint64_t* __restrict__ white,
                                    const int32_t* __restrict__ side, int32_t* first_bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t b = black[i], w = white[i];
    const int sd = side[i];
    bool bad = (b & w) != 0 || ((b | w) & ~Geo<BS>::FULL) != 0 || (sd != 1 && sd != 2);
    if (!bad) bad = legal<BS>(sd == 1 ? b : w, sd == 1 ? w : b) == 0;
    if (bad) atomicMin(first_bad, i);
}

template <int BS>
__global__ void k_board_apply(int n, uint64_t* __restrict__ black, uint64_t* __restrict__ white,
                              int32_t* __restrict__ status, const int32_t* __restrict__ sq,
                              int32_t* __restrict__ ok) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    GameS s;
    s.black = black[i];
    s.white = white[i];
    const int4 st = reinterpret_cast<const int4*>(status)[i];
    s.side = st.x; s.over = st.y; s.winner = st.z; s.passed = st.w;
    const bool r = make_move<BS>(s, sq[i]);
    if (r) {
        black[i] = s.black;
        white[i] = s.white;
        reinterpret_cast<int4*>(status)[i] = make_int4(s.side, s.over, s.winner, s.passed);
    }
    if (ok) ok[i] = r ? 1 : 0;
}

template <int BS>
__global__ void k_board_canonical(int n, const uint64_t* __restrict__ black,
                                  const uint64_t* __restrict__ white,
                                  const int32_t* __restrict__ status, float* __restrict__ out) {
    constexpr int NSQ = Geo<BS>::NSQ;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = t / NSQ, s = t % NSQ;
    if (i >= n) return;
    const int side = status[4 * i];
    const uint64_t P = side == 1 ? black[i] : white[i], O = side == 1 ? white[i] : black[i];
    const uint64_t V = legal<BS>(P, O);
    float* row = out + (size_t)i * 3 * NSQ;
    row[s] = (float)((P >> s) & 1ull);
    row[NSQ + s] = (float)((O >> s) & 1ull);
    row[2 * NSQ + s] = (float)((V >> s) & 1ull);
}

}  // namespace

// =================================================================================================
// host side
// =================================================================================================
static thread_local std::string g_create_error;

// Stream-ordered 32-bit fill as a kernel of our own instead of hipMemsetAsync: inside a captured
// HIP graph a memset node's replays were seen to leave device words of the filled buffer
// holding a 64-bit address (tools/diag_stagger.py: rvz_play's queue words after the second replay
// of a 60-ply graph), after which the queue's task counter never reset. A kernel node has no
// such problem, and costs one ~2 us launch.
__global__ __launch_bounds__(256) void k_fill32(uint32_t* __restrict__ p, uint32_t v, size_t n) {
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        p[i] = v;
}

hipError_t fill32_async(void* p, uint32_t v, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    size_t blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_fill32, dim3((unsigned)blocks), dim3(256), 0, st,
                       static_cast<uint32_t*>(p), v, n);
    return hipGetLastError();
}

// Timing events: no system-scope fence (a fenced record writes back and invalidates the caches,
// which would both slow the timed kernel and inflate the interval).
static hipEvent_t timing_event(rvz_engine* e) {
    if (e->ev_used == e->ev_pool.size()) {
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, hipEventDisableSystemFence) != hipSuccess) return nullptr;
        e->ev_pool.push_back(ev);
    }
    return e->ev_pool[e->ev_used++];
}

static void timing_begin(rvz_engine* e, int kind) {
    if (!e->timing) return;
    hipEvent_t a = timing_event(e), b = timing_event(e);
    if (!a || !b) { e->timing = 0; return; }
    e->ev_marks.push_back({kind, e->ev_used - 2});
    (void)hipEventRecord(a, e->stream);
}

static void timing_end(rvz_engine* e) {
    if (!e->timing || e->ev_marks.empty()) return;
    (void)hipEventRecord(e->ev_pool[e->ev_marks.back().second + 1], e->stream);
}

template <typename T>
static T* dalloc(rvz_engine* e, size_t count) {
    void* p = nullptr;
    if (hipMalloc(&p, count * sizeof(T)) != hipSuccess) p = nullptr;
    e->allocs.push_back(p);
    return static_cast<T*>(p);
}

extern "C" {

int rvz_version(void) { return 1; }

const char* rvz_last_error(const rvz_engine* e) {
    return e ? e->err.c_str() : g_create_error.c_str();
}

int rvz_create(const rvz_config* cfg, rvz_engine** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return RVZ_EINVAL; }
    *out = nullptr;
    const int bs = cfg->board_size;
    if (!board_ok(bs)) { g_create_error = "board_size must be 8 or 6"; return RVZ_EINVAL; }
    if (cfg->n_games <= 0 || cfg->num_simulations <= 0 || cfg->batch_size <= 0) {
        g_create_error = "n_games, num_simulations and batch_size must be positive";
        return RVZ_EINVAL;
    }
    const int E = (cfg->num_simulations + cfg->batch_size - 1) / cfg->batch_size;
    if (E > PATH_CAP) {
        g_create_error = "ceil(num_simulations / batch_size) must be <= 64";
        return RVZ_EINVAL;
    }
    if (cfg->leaf_dtype != RVZ_LEAF_F32 && cfg->leaf_dtype != RVZ_LEAF_BF16) {
        g_create_error = "leaf_dtype must be RVZ_LEAF_F32 or RVZ_LEAF_BF16";
        return RVZ_EINVAL;
    }
    if (hipSetDevice(cfg->device) != hipSuccess) { g_create_error = "hipSetDevice failed"; return RVZ_EHIP; }
    rvz_engine* e = new rvz_engine();
    if (hipGetSymbolAddress(reinterpret_cast<void**>(&e->noise_err), HIP_SYMBOL(g_noise_err)) !=
        hipSuccess)
        e->noise_err = nullptr;
    e->cfg = *cfg;
    e->BS = bs;
    e->NSQ = bs * bs;
    e->NPOL = e->NSQ + 1;
    e->E = E;
    // root + E expansion blocks; rvz_search_memo(on) grows the pool to two halves of E blocks
    // (the memo's two trees) the first time it is enabled, so memo-off engines hold one tree
    e->M = 1 + E * e->NSQ;
    e->v.E = E;
    e->v.NS = (cfg->n_games + RVZ_LIVE_STRIPE - 1) / RVZ_LIVE_STRIPE;
    e->v.live = nullptr;
    e->v.row_of = nullptr;
    e->v.live_total = nullptr;
    const int G = cfg->n_games;
    View& v = e->v;
    v.G = G;
    v.M = e->M;
    v.cpuct = (float)cfg->c_puct;
    v.black = dalloc<uint64_t>(e, G);
    v.white = dalloc<uint64_t>(e, G);
    v.status = dalloc<int32_t>(e, (size_t)G * 4);
    v.nodes = dalloc<Node>(e, (size_t)G * e->M);
    v.meta = dalloc<uint32_t>(e, (size_t)G * e->M);
    v.path = dalloc<int32_t>(e, (size_t)G * PATH_CAP);
    v.pend = dalloc<int32_t>(e, G);
    v.plen = dalloc<int32_t>(e, G);
    v.leaf_legal = dalloc<uint64_t>(e, G);
    v.root_legal = dalloc<uint64_t>(e, G);
    v.leaf_meta = dalloc<uint32_t>(e, G);
    v.nexp = dalloc<int32_t>(e, G);
    v.rng_u = dalloc<double>(e, (size_t)G * RNG_DRAWS);
    v.rng_pos = dalloc<int32_t>(e, G);
    v.err = dalloc<int32_t>(e, 1);
    v.memo = 0;
    v.carry = dalloc<uint32_t>(e, G);
    v.bval = dalloc<float>(e, (size_t)G * 2 * E);
    v.noise_eps = 0.0f;
    v.noise_om = 1.0f;
    v.noise_alpha = 1.0f;
    v.noise_salt = 0u;
    v.sched_from = 0;
    v.sched_late = 0.0;
    v.open_n = 0;
    v.open_salt = 0u;
    v.open_black = nullptr;
    v.open_white = nullptr;
    v.open_side = nullptr;
    v.seed32 = dalloc<uint32_t>(e, G);
    v.eta = dalloc<float>(e, (size_t)G * WAVE);
    e->stats_buf = dalloc<unsigned long long>(e, 3 * (size_t)G);
    v.stats = nullptr;
    for (void* p : e->allocs)
        if (!p) { g_create_error = "hipMalloc failed (out of device memory?)"; rvz_destroy(e); return RVZ_ENOMEM; }
    hipError_t s = hipMemset(v.err, 0, sizeof(int32_t));
    s = s == hipSuccess ? hipMemset(v.pend, 0, sizeof(int32_t) * G) : s;
    s = s == hipSuccess ? hipMemset(v.rng_pos, 0, sizeof(int32_t) * G) : s;
    s = s == hipSuccess ? hipMemset(v.meta, 0, sizeof(uint32_t) * (size_t)G * e->M) : s;
    s = s == hipSuccess ? hipMemset(v.root_legal, 0, sizeof(uint64_t) * G) : s;
    s = s == hipSuccess ? hipMemset(v.leaf_meta, 0, sizeof(uint32_t) * G) : s;
    s = s == hipSuccess ? hipMemset(v.path, 0, sizeof(int32_t) * G * PATH_CAP) : s;
    s = s == hipSuccess ? hipMemsetD32(v.carry, LINK_NONE, G) : s;
    if (s == hipSuccess) s = hipDeviceSynchronize();
    if (s != hipSuccess) {
        g_create_error = std::string("device init: ") + hipGetErrorString(s);
        rvz_destroy(e);
        return RVZ_EHIP;
    }
    *out = e;
    // every game starts at the start position with seed = game index until rvz_env_reset
    std::vector<uint32_t> seeds(G);
    for (int g = 0; g < G; ++g) seeds[g] = (uint32_t)g;
    uint32_t* dseeds = nullptr;
    if (hipMalloc(&dseeds, sizeof(uint32_t) * G) != hipSuccess) { rvz_destroy(e); *out = nullptr; return RVZ_ENOMEM; }
    int r = hipMemcpy(dseeds, seeds.data(), sizeof(uint32_t) * G, hipMemcpyHostToDevice) == hipSuccess
                ? rvz_env_reset(e, dseeds, nullptr) : RVZ_EHIP;
    if (hipDeviceSynchronize() != hipSuccess) r = RVZ_EHIP;
    (void)hipFree(dseeds);
    if (r != RVZ_OK) { g_create_error = e->err; rvz_destroy(e); *out = nullptr; return r; }
    return RVZ_OK;
}

void rvz_destroy(rvz_engine* e) {
    if (!e) return;
    table_free(e);
    if (e->open_buf) (void)hipFree(e->open_buf);
    for (hipEvent_t ev : e->ev_pool) (void)hipEventDestroy(ev);
    for (void* p : e->allocs)
        if (p) (void)hipFree(p);
    delete e;
}

int rvz_set_stream(rvz_engine* e, void* stream) {
    if (!e) return RVZ_EINVAL;
    e->stream = (hipStream_t)stream;
    return RVZ_OK;
}

int rvz_sync(rvz_engine* e) {
    if (!e) return RVZ_EINVAL;
    RVZ_HIP(hipStreamSynchronize(e->stream), e);
    return RVZ_OK;
}

int rvz_check(rvz_engine* e, int32_t* host_err) {
    if (!e) return RVZ_EINVAL;
    int32_t h = 0, hn = 0;
    RVZ_HIP(hipMemcpyAsync(&h, e->v.err, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream), e);
    if (e->noise_err)   // rvz_dirichlet_noise's flag (it has no engine): the device's word
        RVZ_HIP(hipMemcpyAsync(&hn, e->noise_err, sizeof(int32_t), hipMemcpyDeviceToHost,
                               e->stream), e);
    RVZ_HIP(hipStreamSynchronize(e->stream), e);
    if (hn) RVZ_HIP(hipMemsetAsync(e->noise_err, 0, sizeof(int32_t), e->stream), e);
    const int32_t own = h;
    h |= hn;
    if (host_err) *host_err = h;
    if (h) {
        if (own) RVZ_HIP(hipMemsetAsync(e->v.err, 0, sizeof(int32_t), e->stream), e);
        e->err = "device error word " + std::to_string(h) +
                 " (1: rng stream exhausted, 2: node pool, 4: path depth, 8: non-finite NN "
                 "value or probability, 16: rvz_play queue wait timed out, 32: root-noise "
                 "Gamma sampler out of attempts)";
        return RVZ_EDEVICE;
    }
    return RVZ_OK;
}

int rvz_env_reset(rvz_engine* e, const uint32_t* seeds, const uint8_t* mask) {
    if (!e || !seeds) return RVZ_EINVAL;
    e->pending = 0;
    launch_games_unchecked(e, k_reset<8>, k_reset<6>, e->v, seeds, mask);
    e->searching = 0;
    return launch_check(e, "k_reset");
}

int rvz_env_autoreset(rvz_engine* e, const int32_t* idx, int64_t* seeds, int64_t stride,
                      int64_t* plies, int64_t* done, int32_t reset) {
    const Range trace_range("rvz.env.autoreset");
    if (!e || !idx || !plies || (reset && (!seeds || !done))) return RVZ_EINVAL;
    if (reset) e->pending = 0;
    return launch_games(e, "k_autoreset", k_autoreset<8>, k_autoreset<6>, e->v, idx, seeds, stride,
                        plies, done, reset);
}

// The pool is copied into one allocation of the engine's own (black, white, side, and the word
// the validation kernel writes) and checked there; a refused pool leaves the setting as it was.
// The old copy is freed behind a stream synchronisation, so no launch still reads it; pointers
// held by an already captured graph would dangle: set the pool before capturing.
int rvz_env_openings(rvz_engine* e, int32_t n, const uint64_t* black, const uint64_t* white,
                     const int32_t* side, uint32_t salt) {
    if (!e) return RVZ_EINVAL;
    if (n < 0 || (n > 0 && (!black || !white || !side))) {
        e->err = "rvz_env_openings: n >= 0, and with n > 0 black, white and side";
        return RVZ_EINVAL;
    }
    if (in_search(e, "rvz_env_openings")) return RVZ_EINVAL;
    void* buf = nullptr;
    if (n > 0) {
        const size_t N = (size_t)n;
        const size_t bytes = (size_t)up16((int64_t)(N * 20)) + 16;
        if (hipMalloc(&buf, bytes) != hipSuccess) {
            e->err = "hipMalloc failed (the opening pool)";
            return RVZ_ENOMEM;
        }
        uint64_t* pb = static_cast<uint64_t*>(buf);
        uint64_t* pw = pb + N;
        int32_t* ps = reinterpret_cast<int32_t*>(pw + N);
        int32_t* bad = reinterpret_cast<int32_t*>(static_cast<char*>(buf) + bytes - 16);
        int32_t first_bad = 0x7fffffff;
        hipError_t s = hipMemcpyAsync(pb, black, N * 8, hipMemcpyDeviceToDevice, e->stream);
        s = s == hipSuccess ? hipMemcpyAsync(pw, white, N * 8, hipMemcpyDeviceToDevice, e->stream) : s;
        s = s == hipSuccess ? hipMemcpyAsync(ps, side, N * 4, hipMemcpyDeviceToDevice, e->stream) : s;
        s = s == hipSuccess ? hipMemcpyAsync(bad, &first_bad, 4, hipMemcpyHostToDevice, e->stream) : s;
        if (s == hipSuccess) {
            const Geometry g = thread_per_row(n);
            launch_bs_unchecked(e->BS, k_openings_validate<8>, k_openings_validate<6>, g.grid,
                                g.block, e->stream, n, (const uint64_t*)pb, (const uint64_t*)pw,
                                (const int32_t*)ps, bad);
            s = hipGetLastError();
        }
        s = s == hipSuccess ? hipMemcpyAsync(&first_bad, bad, 4, hipMemcpyDeviceToHost, e->stream) : s;
        s = s == hipSuccess ? hipStreamSynchronize(e->stream) : s;
        if (s != hipSuccess || first_bad != 0x7fffffff) {
            (void)hipFree(buf);
            if (s != hipSuccess) {
                e->err = std::string("rvz_env_openings: ") + hipGetErrorString(s);
                return RVZ_EHIP;
            }
            e->err = "rvz_env_openings: row " + std::to_string(first_bad) +
                     " is no opening (overlapping discs, a bit at or above S*S, a side other "
                     "than 1 | 2, or the mover has no legal square)";
            return RVZ_EINVAL;
        }
        e->v.open_black = pb;
        e->v.open_white = pw;
        e->v.open_side = ps;
    } else {
        RVZ_HIP(hipStreamSynchronize(e->stream), e);
        e->v.open_black = nullptr;
        e->v.open_white = nullptr;
        e->v.open_side = nullptr;
    }
    if (e->open_buf) (void)hipFree(e->open_buf);   // synchronised above: no launch reads it
    e->open_buf = buf;
    e->v.open_n = n;
    e->v.open_salt = n > 0 ? salt : 0u;
    return RVZ_OK;
}

int rvz_env_get(rvz_engine* e, uint64_t* black, uint64_t* white, int32_t* status) {
    if (!e) return RVZ_EINVAL;
    const size_t G = e->v.G;
    if (black) RVZ_HIP(hipMemcpyAsync(black, e->v.black, G * 8, hipMemcpyDeviceToDevice, e->stream), e);
    if (white) RVZ_HIP(hipMemcpyAsync(white, e->v.white, G * 8, hipMemcpyDeviceToDevice, e->stream), e);
    if (status) RVZ_HIP(hipMemcpyAsync(status, e->v.status, G * 16, hipMemcpyDeviceToDevice, e->stream), e);
    return RVZ_OK;
}

// The memo's carried links hold only while each search follows the previous one's move
// (rvz_act with apply): a position set or moved from the host, or an abandoned search, drops them.
static int memo_drop(rvz_engine* e) {
    if (!e->v.memo) return RVZ_OK;
    RVZ_HIP(fill32_async(e->v.carry, LINK_NONE, (size_t)e->v.G, e->stream), e);
    return RVZ_OK;
}

int rvz_env_set(rvz_engine* e, const uint64_t* black, const uint64_t* white, const int32_t* status) {
    if (!e || !black || !white || !status) return RVZ_EINVAL;
    e->pending = 0;
    if (memo_drop(e) != RVZ_OK) return RVZ_EHIP;
    const size_t G = e->v.G;
    RVZ_HIP(hipMemcpyAsync(e->v.black, black, G * 8, hipMemcpyDeviceToDevice, e->stream), e);
    RVZ_HIP(hipMemcpyAsync(e->v.white, white, G * 8, hipMemcpyDeviceToDevice, e->stream), e);
    RVZ_HIP(hipMemcpyAsync(e->v.status, status, G * 16, hipMemcpyDeviceToDevice, e->stream), e);
    e->searching = 0;
    return RVZ_OK;
}

int rvz_env_set_draws(rvz_engine* e, const double* u) {
    static_assert(RNG_DRAWS == RVZ_DRAWS, "include/rvz.h's RVZ_DRAWS is the stream length");
    if (!e || !u) return RVZ_EINVAL;
    const size_t G = e->v.G;
    RVZ_HIP(hipMemcpyAsync(e->v.rng_u, u, G * RNG_DRAWS * sizeof(double), hipMemcpyDeviceToDevice,
                           e->stream), e);
    RVZ_HIP(hipMemsetAsync(e->v.rng_pos, 0, G * sizeof(int32_t), e->stream), e);
    return RVZ_OK;
}

int rvz_env_draws(rvz_engine* e, int32_t* out_pos) {
    if (!e || !out_pos) return RVZ_EINVAL;
    RVZ_HIP(hipMemcpyAsync(out_pos, e->v.rng_pos, (size_t)e->v.G * sizeof(int32_t),
                           hipMemcpyDeviceToDevice, e->stream), e);
    return RVZ_OK;
}

int rvz_board_legal(int32_t bs, int32_t n, const uint64_t* black, const uint64_t* white,
                    const int32_t* status, uint64_t* out, void* stream) {
    if (!board_ok(bs) || n < 0 || (n > 0 && (!black || !white || !status || !out)))
        return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    const Geometry g = thread_per_row(n);
    return launch_bs(bs, k_board_legal<8>, k_board_legal<6>, g.grid, g.block, (hipStream_t)stream,
                     n, black, white, status, out);
}

int rvz_board_apply(int32_t bs, int32_t n, uint64_t* black, uint64_t* white, int32_t* status,
                    const int32_t* sq, int32_t* ok, void* stream) {
    if (!board_ok(bs) || n < 0 || (n > 0 && (!black || !white || !status || !sq)))
        return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    const Geometry g = thread_per_row(n);
    return launch_bs(bs, k_board_apply<8>, k_board_apply<6>, g.grid, g.block, (hipStream_t)stream,
                     n, black, white, status, sq, ok);
}

int rvz_board_canonical(int32_t bs, int32_t n, const uint64_t* black, const uint64_t* white,
                        const int32_t* status, float* out, void* stream) {
    if (!board_ok(bs) || n < 0 || (n > 0 && (!black || !white || !status || !out)))
        return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    const Geometry g = thread_per_row(n * bs * bs);   // one thread per square
    return launch_bs(bs, k_board_canonical<8>, k_board_canonical<6>, g.grid, g.block,
                     (hipStream_t)stream, n, black, white, status, out);
}

int rvz_policy_softmax(int32_t bs, int32_t n, const float* logits, float* probs, void* stream) {
    if (!board_ok(bs) || n < 0 || (n > 0 && (!logits || !probs))) return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    const Geometry g = wave_per_row(n, WPB);
    return launch_bs(bs, k_policy_softmax<8>, k_policy_softmax<6>, g.grid, g.block,
                     (hipStream_t)stream, n, logits, probs);
}

int rvz_env_legal(rvz_engine* e, uint64_t* out) {
    if (!e) return RVZ_EINVAL;
    int r = rvz_board_legal(e->BS, e->v.G, e->v.black, e->v.white, e->v.status, out, e->stream);
    if (r != RVZ_OK) e->err = "rvz_env_legal launch failed";
    else e->counters[1] += 1;
    return r;
}

int rvz_env_apply(rvz_engine* e, const int32_t* sq, int32_t* ok) {
    const Range trace_range("rvz.env.apply");
    if (!e) return RVZ_EINVAL;
    if (memo_drop(e) != RVZ_OK) return RVZ_EHIP;
    int r = rvz_board_apply(e->BS, e->v.G, e->v.black, e->v.white, e->v.status, sq, ok, e->stream);
    if (r != RVZ_OK) e->err = "rvz_env_apply launch failed";
    else e->counters[1] += 1;
    e->searching = 0;
    return r;
}

int rvz_search_begin(rvz_engine* e) {
    const Range trace_range("rvz.search.begin");
    if (!e) return RVZ_EINVAL;
    if (e->searching && e->next_batch > 0 && memo_drop(e) != RVZ_OK) return RVZ_EHIP;
    e->next_batch = 0;
    e->searching = 1;
    if (e->v.live && e->live_dirty) {   // an abandoned search left counts behind
        RVZ_HIP(fill32_async(e->v.live, 0u, (size_t)e->E * e->v.NS * RVZ_LIVE_PITCH, e->stream),
                e);
        e->live_dirty = 0;
    }
    e->pending = 0;  // an unconsumed submit of an abandoned search is dropped
    return RVZ_OK;
}

int rvz_search_step(rvz_engine* e, void* leaf_x, int32_t* need) {
    const Range trace_range("rvz.search.step (expand/backup + select)");
    if (!e || !leaf_x || !need) return RVZ_EINVAL;
    if (!e->searching) { e->err = "rvz_search_step before rvz_search_begin"; return RVZ_EINVAL; }
    const int S = e->cfg.num_simulations, B = e->cfg.batch_size;
    const int start = e->next_batch * B;
    if (start >= S) return RVZ_DONE;
    const int bsz = S - start < B ? S - start : B;
    const int first = e->next_batch == 0;
    const int ex = e->pending;
    const float* pol = e->pend_policy;
    const float* val = e->pend_value;
    const int lg = e->pend_is_logits;
    const auto step = [&](auto* x) {   // k_step<BS, XT> for the leaf planes' type
        using XT = std::remove_pointer_t<decltype(x)>;
        launch_games_unchecked(e, k_step<8, XT>, k_step<6, XT>, e->v, ex, pol, lg, val, first, bsz,
                               e->next_batch, x, need);
    };
    timing_begin(e, 0);
    if (e->cfg.leaf_dtype == RVZ_LEAF_F32) step((float*)leaf_x);
    else step((__hip_bfloat16*)leaf_x);
    timing_end(e);
    e->pending = 0;
    e->next_batch += 1;
    if (e->v.live) e->live_dirty = 1;
    e->counters[0] += 1;
    return launch_check(e, "k_step");
}

int rvz_search_submit(rvz_engine* e, const float* policy, int32_t is_logits, const float* value) {
    const Range trace_range("rvz.search.submit");
    if (!e || !policy || !value) return RVZ_EINVAL;
    if (!e->searching || e->next_batch == 0) {
        e->err = "rvz_search_submit without a preceding rvz_search_step";
        return RVZ_EINVAL;
    }
    if (e->pending) { e->err = "rvz_search_submit twice for one batch"; return RVZ_EINVAL; }
    // deferred: the expand + backup runs at the head of the next k_step / k_act launch (or of
    // k_expand_backup for rvz_search_visits); policy/value must stay valid until then.
    e->pending = 1;
    e->pend_policy = policy;
    e->pend_value = value;
    e->pend_is_logits = is_logits;
    return RVZ_OK;
}

static int flush_pending(rvz_engine* e) {
    if (!e->pending) return RVZ_OK;
    launch_games_unchecked(e, k_expand_backup<8>, k_expand_backup<6>, e->v, e->pending,
                           e->pend_policy, e->pend_is_logits, e->pend_value);
    e->pending = 0;
    return launch_check(e, "k_expand_backup");
}

int rvz_search_visits(rvz_engine* e, int32_t* out) {
    if (!e || !out) return RVZ_EINVAL;
    int r = flush_pending(e);
    if (r != RVZ_OK) return r;
    return launch_games(e, "k_visits", k_visits<8>, k_visits<6>, e->v, out);
}

int rvz_search_compact(rvz_engine* e, int32_t on) {
    if (!e) return RVZ_EINVAL;
    if (in_search(e, "rvz_search_compact")) return RVZ_EINVAL;
    if (on && !e->live_buf) {
        // [E] live counts, [G] row map, then the 8-byte running total
        const size_t nlive = (size_t)e->E * e->v.NS * RVZ_LIVE_PITCH;
        const size_t words = (nlive + e->v.G + 1) / 2 * 2 + 2;
        e->live_buf = dalloc<int32_t>(e, words);
        if (!e->live_buf) { e->err = "hipMalloc failed (live counts)"; return RVZ_ENOMEM; }
        RVZ_HIP(hipMemsetAsync(e->live_buf, 0, sizeof(int32_t) * words, e->stream), e);
        e->live_total = reinterpret_cast<unsigned long long*>(e->live_buf + words - 2);
        e->live_dirty = 0;
    }
    e->v.live = on ? e->live_buf : nullptr;
    e->v.row_of = on ? e->live_buf + (size_t)e->E * e->v.NS * RVZ_LIVE_PITCH : nullptr;
    e->v.live_total = on ? e->live_total : nullptr;
    return RVZ_OK;
}

// The memo needs the node pool's second half (the previous search's tree stays readable while a
// search writes the other half): the first rvz_search_memo(on) reallocates nodes and meta with
// M = 1 + 2 E S^2. Outside a search no tree is live (the carried links are dropped here anyway),
// so nothing is copied. Pointers held by an already captured graph would dangle: enable the memo
// before capturing (rvz.Engine does it in its constructor).
static int memo_grow(rvz_engine* e) {
    const int M2 = 1 + 2 * e->E * e->NSQ;
    if (e->M == M2) return RVZ_OK;
    const size_t G = e->v.G;
    Node* nodes = nullptr;
    uint32_t* meta = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&nodes), G * M2 * sizeof(Node)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&meta), G * M2 * sizeof(uint32_t)) != hipSuccess) {
        if (nodes) (void)hipFree(nodes);
        e->err = "hipMalloc failed (the memo's second node-pool half)";
        return RVZ_ENOMEM;
    }
    RVZ_HIP(hipStreamSynchronize(e->stream), e);   // no launch may still read the old pool
    for (void*& p : e->allocs) {
        if (p == e->v.nodes) { (void)hipFree(p); p = nodes; }
        else if (p == e->v.meta) { (void)hipFree(p); p = meta; }
    }
    e->v.nodes = nodes;
    e->v.meta = meta;
    e->M = e->v.M = M2;
    RVZ_HIP(hipMemsetAsync(meta, 0, G * M2 * sizeof(uint32_t), e->stream), e);
    return RVZ_OK;
}

int rvz_search_memo(rvz_engine* e, int32_t on) {
    if (!e) return RVZ_EINVAL;
    if (in_search(e, "rvz_search_memo")) return RVZ_EINVAL;
    if (on) {
        const int r = memo_grow(e);
        if (r != RVZ_OK) return r;
    }
    e->v.memo = 1;             // so that memo_drop clears the links either way
    if (memo_drop(e) != RVZ_OK) return RVZ_EHIP;
    e->v.memo = on ? 1 : 0;
    return RVZ_OK;
}

int rvz_search_memo_reset(rvz_engine* e) {
    if (!e) return RVZ_EINVAL;
    const int r = memo_drop(e);
    return r != RVZ_OK ? r : table_bump(e);   // new weights: the table's rows are stale too
}

// alpha as the kernels take it: a positive, finite float32 (NaN fails the comparisons)
static bool noise_alpha_ok(double alpha) { return alpha >= 1.0e-37 && alpha <= 3.0e38; }

int rvz_search_root_noise(rvz_engine* e, double alpha, double epsilon, uint32_t salt) {
    if (!e) return RVZ_EINVAL;
    if (!noise_alpha_ok(alpha) || !(epsilon >= 0.0 && epsilon <= 1.0)) {
        e->err = "rvz_search_root_noise: alpha a positive finite float32 (1e-37 .. 3e38), "
                 "0 <= epsilon <= 1";
        return RVZ_EINVAL;
    }
    if (in_search(e, "rvz_search_root_noise")) return RVZ_EINVAL;
    // eps and 1 - eps as float32, once, here: the kernels (and a test's restatement) use these
    const float eps = (float)epsilon;
    e->v.noise_eps = eps;
    e->v.noise_om = 1.0f - eps;
    e->v.noise_alpha = (float)alpha;
    e->v.noise_salt = salt;
    return RVZ_OK;
}

int rvz_dirichlet_noise(int32_t bs, int32_t n, const uint64_t* legal, const uint32_t* seed32,
                        const int32_t* tag, uint32_t salt, double alpha, float* out,
                        uint32_t* out_bits, void* stream) {
    if (!board_ok(bs) || n < 0 || !noise_alpha_ok(alpha) ||
        (n > 0 && (!legal || !seed32 || !tag || !out)) || ((uintptr_t)out_bits & 15) != 0)
        return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    const Geometry g = wave_per_row(n, WPB);
    return launch_bs(bs, k_dirichlet<8>, k_dirichlet<6>, g.grid, g.block, (hipStream_t)stream, n,
                     legal, seed32, tag, salt, (float)alpha, out, out_bits);
}

int rvz_act_schedule(rvz_engine* e, int32_t from_discs, double late_temperature) {
    if (!e) return RVZ_EINVAL;
    if (from_discs > 0 && !(late_temperature >= 0.0 && late_temperature <= 1.7976931348623157e308)) {
        e->err = "rvz_act_schedule: late_temperature must be finite and >= 0";
        return RVZ_EINVAL;
    }
    if (in_search(e, "rvz_act_schedule")) return RVZ_EINVAL;
    e->v.sched_from = from_discs > 0 ? from_discs : 0;
    e->v.sched_late = from_discs > 0 ? late_temperature : 0.0;
    return RVZ_OK;
}

int rvz_action_probs(int32_t bs, int32_t n, const int32_t* visits, const double* temperature,
                     const double* u, int32_t* out_idx, double* out_p, int32_t* out_drew,
                     void* stream) {
    if (!board_ok(bs) || n < 0 ||
        (n > 0 && (!visits || !temperature || !u || !out_idx || !out_p)))
        return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    const Geometry g = wave_per_row(n, WPB);
    return launch_bs(bs, k_action_probs<8>, k_action_probs<6>, g.grid, g.block,
                     (hipStream_t)stream, n, visits, temperature, u, out_idx, out_p, out_drew);
}

int rvz_search_rows_total(rvz_engine* e, int64_t* out) {
    if (!e || !out) return RVZ_EINVAL;
    *out = 0;
    if (!e->live_total) return RVZ_OK;
    unsigned long long h = 0;
    RVZ_HIP(hipMemcpyAsync(&h, e->live_total, sizeof(h), hipMemcpyDeviceToHost, e->stream), e);
    RVZ_HIP(hipStreamSynchronize(e->stream), e);
    *out = (int64_t)h;
    return RVZ_OK;
}

const int32_t* rvz_search_live_count(const rvz_engine* e) {
    if (!e || !e->v.live || e->next_batch == 0) return nullptr;
    return e->v.live + (size_t)(e->next_batch - 1) * e->v.NS * RVZ_LIVE_PITCH;
}

#ifdef RVZ_WALK_STATS
// host int64[10]: sums over games of the 5 walk counters, then their maxima; zeroes them
int rvz_walk_stats(int32_t n_games, int64_t* out10) {
    std::vector<unsigned int> h;
    const int n = n_games < WALK_STATS_MAX ? n_games : WALK_STATS_MAX;
    if (take_rows(g_walk, n, h) != RVZ_OK) return RVZ_EHIP;
    for (int i = 0; i < 10; ++i) out10[i] = 0;
    for (int gi = 0; gi < n; ++gi)
        for (int i = 0; i < 5; ++i) {
            out10[i] += h[(size_t)gi * 5 + i];
            if ((int64_t)h[(size_t)gi * 5 + i] > out10[5 + i]) out10[5 + i] = h[(size_t)gi * 5 + i];
        }
    return RVZ_OK;
}

// host int64[11]: the 5 shader-clock categories of the game with the largest total, then the
// means over games, then that game's index; zeroes them
int rvz_walk_times(int32_t n_games, int64_t* out11) {
    std::vector<unsigned long long> h;
    const int n = n_games < WALK_STATS_MAX ? n_games : WALK_STATS_MAX;
    if (take_rows(g_wtime, n, h) != RVZ_OK) return RVZ_EHIP;
    int best = 0;
    unsigned long long bt = 0;
    double mean[5] = {0, 0, 0, 0, 0};
    for (int gi = 0; gi < n; ++gi) {
        unsigned long long t = 0;
        for (int i = 0; i < 5; ++i) {
            t += h[(size_t)gi * 5 + i];
            mean[i] += (double)h[(size_t)gi * 5 + i] / n;
        }
        if (t > bt) { bt = t; best = gi; }
    }
    for (int i = 0; i < 5; ++i) {
        out11[i] = (int64_t)h[(size_t)best * 5 + i];
        out11[5 + i] = (int64_t)mean[i];
    }
    out11[10] = best;
    return RVZ_OK;
}

#endif

int rvz_search_skip(rvz_engine* e) {
    if (!e) return RVZ_EINVAL;
    const int S = e->cfg.num_simulations, B = e->cfg.batch_size;
    if (!e->searching || e->next_batch == 0 || e->next_batch * B < S) {
        e->err = "rvz_search_skip is only valid after the last rvz_search_step of a search";
        return RVZ_EINVAL;
    }
    if (e->pending) { e->err = "rvz_search_skip after rvz_search_submit"; return RVZ_EINVAL; }
    if (S <= B) {     // one batch: its leaf is the root, whose expansion the act needs
        e->err = "rvz_search_skip needs a search of at least two batches (num_simulations > "
                 "batch_size): a single batch's leaf is the root";
        return RVZ_EINVAL;
    }
    e->pending = 2;   // rvz_act: visit counts only
    return RVZ_OK;
}

int rvz_act(rvz_engine* e, double temperature, const double* u, int32_t apply, int32_t* out_idx,
            double* out_p) {
    const Range trace_range("rvz.act (expand/backup + action + move)");
    if (!e || !out_idx || !out_p) return RVZ_EINVAL;
    const int ex = e->pending;
    timing_begin(e, 1);
    launch_games_unchecked(e, k_act<8>, k_act<6>, e->v, ex, e->pend_policy, e->pend_is_logits,
                           e->pend_value, temperature, u, apply, out_idx, out_p);
    timing_end(e);
    e->pending = 0;
    e->live_dirty = 0;
    if (apply) e->searching = 0;
    return launch_check(e, "k_act");
}

// ---- stream-ordered HIP event timer without system fence (bench.py: per-launch kernel
// durations in eager plies; torch's events carry a system-scope fence that adds tens of us)
struct rvz_timer {
    std::vector<hipEvent_t> ev;
};

int rvz_timer_create(int32_t n, rvz_timer** out) {
    if (n <= 0 || !out) return RVZ_EINVAL;
    rvz_timer* t = new rvz_timer;
    t->ev.resize(n, nullptr);
    for (auto& e : t->ev) {
        if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) {
            for (auto& f : t->ev)
                if (f) (void)hipEventDestroy(f);
            delete t;
            return RVZ_EHIP;
        }
    }
    *out = t;
    return RVZ_OK;
}

int rvz_timer_record(rvz_timer* t, int32_t i, void* stream) {
    if (!t || i < 0 || i >= (int32_t)t->ev.size()) return RVZ_EINVAL;
    return hipEventRecord(t->ev[i], (hipStream_t)stream) == hipSuccess ? RVZ_OK : RVZ_EHIP;
}

int rvz_timer_elapsed(rvz_timer* t, int32_t i, int32_t j, float* ms) {
    if (!t || !ms || i < 0 || j < 0 || i >= (int32_t)t->ev.size() || j >= (int32_t)t->ev.size())
        return RVZ_EINVAL;
    if (hipEventSynchronize(t->ev[j]) != hipSuccess) return RVZ_EHIP;
    return hipEventElapsedTime(ms, t->ev[i], t->ev[j]) == hipSuccess ? RVZ_OK : RVZ_EHIP;
}

void rvz_timer_destroy(rvz_timer* t) {
    if (!t) return;
    for (auto& e : t->ev)
        if (e) (void)hipEventDestroy(e);
    delete t;
}

int rvz_counters(const rvz_engine* e, int64_t* out2) {
    if (!e || !out2) return RVZ_EINVAL;
    out2[0] = e->counters[0];
    out2[1] = e->counters[1];
    return RVZ_OK;
}

int rvz_stats_enable(rvz_engine* e, int32_t on) {
    if (!e) return RVZ_EINVAL;
    e->v.stats = on ? e->stats_buf : nullptr;
    if (on) RVZ_HIP(hipMemsetAsync(e->stats_buf, 0, 3 * (size_t)e->v.G * sizeof(unsigned long long), e->stream), e);
    return RVZ_OK;
}

int rvz_stats_read(rvz_engine* e, int64_t* out3) {
    if (!e || !out3) return RVZ_EINVAL;
    const size_t G = e->v.G;
    std::vector<unsigned long long> h(3 * G);
    RVZ_HIP(hipMemcpyAsync(h.data(), e->stats_buf, h.size() * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, e->stream), e);
    RVZ_HIP(hipStreamSynchronize(e->stream), e);
    for (int k = 0; k < 3; ++k) {
        unsigned long long t = 0;
        for (size_t g = 0; g < G; ++g) t += h[k * G + g];
        out3[k] = (int64_t)t;
    }
    return RVZ_OK;
}

int rvz_timing_enable(rvz_engine* e, int32_t on) {
    if (!e) return RVZ_EINVAL;
    e->timing = on ? 1 : 0;
    e->ev_used = 0;
    e->ev_marks.clear();
    return RVZ_OK;
}

int rvz_timing_read(rvz_engine* e, double* out_ms, int32_t* out_n) {
    if (!e || !out_ms || !out_n) return RVZ_EINVAL;
    RVZ_HIP(hipStreamSynchronize(e->stream), e);
    double sum[2] = {0.0, 0.0};
    int32_t n[2] = {0, 0};
    for (const auto& mk : e->ev_marks) {
        float ms = 0.0f;
        RVZ_HIP(hipEventElapsedTime(&ms, e->ev_pool[mk.second], e->ev_pool[mk.second + 1]), e);
        sum[mk.first] += ms;
        n[mk.first] += 1;
    }
    for (int k = 0; k < 2; ++k) {
        out_ms[k] = n[k] ? sum[k] / n[k] : 0.0;
        out_n[k] = n[k];
    }
    return RVZ_OK;
}

int rvz_tree_nodes(const rvz_engine* e) { return e ? e->M : RVZ_EINVAL; }

int rvz_tree_export(rvz_engine* e, void* nodes_out, uint32_t* meta_out) {
    if (!e) return RVZ_EINVAL;
    int r = flush_pending(e);
    if (r != RVZ_OK) return r;
    const size_t n = (size_t)e->v.G * e->M;
    if (nodes_out) RVZ_HIP(hipMemcpyAsync(nodes_out, e->v.nodes, n * sizeof(Node), hipMemcpyDeviceToDevice, e->stream), e);
    if (meta_out) RVZ_HIP(hipMemcpyAsync(meta_out, e->v.meta, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, e->stream), e);
    return RVZ_OK;
}

int rvz_footprint(const rvz_engine* e, int64_t* bytes_tree, int64_t* bytes_env) {
    if (!e) return RVZ_EINVAL;
    const int64_t G = e->v.G;
    if (bytes_tree)
        *bytes_tree = G * e->M * (int64_t)(sizeof(Node) + sizeof(uint32_t)) +
                      G * (PATH_CAP * 4 + 4 * 4 + 8) + G * (4 + 2 * e->E * 4);   // + memo
    if (bytes_env) *bytes_env = G * (8 + 8 + 16) + G * (RNG_DRAWS * 8 + 4);
    return RVZ_OK;
}

}  // extern "C"
