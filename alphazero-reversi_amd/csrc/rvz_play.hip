// rvz_play.hip — the host side of fused self-play (rvz_play, include/rvz.h): the scratch layout, the
// launch of k_play (csrc/rvz_play.hip.h) at the (board, filters) pair's h2 tile, the pass gate's
// setting and the cross-game table. The engine's other entry points are in csrc/rvz_engine.hip; the
// two units share struct rvz_engine and the launch helpers (csrc/rvz_engine_host.h).
//
// The instrumented builds' device arrays exist once per translation unit, so the readers of the
// words k_play writes are here: rvz_play_walk_read (g_wtime, g_ftime: csrc/rvz_search.hip.h) and
// rvz_play_timing_read (g_play_t: csrc/rvz_play.hip.h; g_pass_t: csrc/rvz_resnet_common.hip.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../include/rvz.h"
#include "rvz_engine_host.h"
#include "rvz_h2.hip.h"
#include "rvz_host.hip.h"
#include "rvz_play.hip.h"
#include "rvz_search.hip.h"
#include "rvz_trace.h"

using namespace rvz;

// (The team-specialised fused kernel k_play12 of round 4 — measured 4% behind k_play, DESIGN
// §8.6 — is kept as tools/patches/play12_teams.patch, not in the product library.)

// a new table generation (new weights): every slot of an older generation reads as empty
__global__ void k_table_bump(unsigned* gen) {
    if (threadIdx.x == 0) atomicAdd(gen, 1u);
}

int table_bump(rvz_engine* e) {
    if (!e->tgen) return RVZ_OK;
    hipLaunchKernelGGL(k_table_bump, dim3(1), dim3(64), 0, e->stream, e->tgen);
    RVZ_HIP(hipGetLastError(), e);
    return RVZ_OK;
}

void table_free(rvz_engine* e) {
    for (void* p : {(void*)e->tab, (void*)e->tclaim, (void*)e->tgen})
        if (p) (void)hipFree(p);
    e->tab = nullptr;
    e->tclaim = nullptr;
    e->tgen = nullptr;
    e->tslots = 0;
    e->tab_blob = nullptr;
}

extern "C" {

int rvz_play_gate(rvz_engine* e, double fraction, double timeout_us, double late_us) {
    if (!e || !(fraction <= 1.0) || !(timeout_us >= 0.0) || !(late_us >= 0.0) ||
        timeout_us > 1e6 || late_us > 1e6) {
        if (e) e->err = "rvz_play_gate: fraction <= 1 (< 0: the default), 0 <= us <= 1e6";
        return RVZ_EINVAL;
    }
    e->gate_frac = fraction;
    e->gate_us = timeout_us;
    e->gate_late_us = late_us;
    return RVZ_OK;
}

int rvz_play_ahead(rvz_engine* e, int32_t mode) {
    if (!e || mode > 2) {
        if (e) e->err = "rvz_play_ahead: mode 0, 1 or 2 (< 0: the default)";
        return RVZ_EINVAL;
    }
    e->ahead = mode;
    return RVZ_OK;
}

int rvz_play_ahead_stats(rvz_engine* e, int64_t* stats) {
    if (!e) return RVZ_EINVAL;
    e->ahead_stats = stats;
    return RVZ_OK;
}

int rvz_play_table(rvz_engine* e, int64_t slots, int32_t max_discs) {
    if (!e) return RVZ_EINVAL;
    if (slots != 0 && (slots < 1024 || (slots & (slots - 1)) != 0 || slots > (1ll << 30) ||
                       max_discs < 4)) {
        e->err = "rvz_play_table: slots a power of two in [1024, 2^30] (or 0), max_discs >= 4";
        return RVZ_EINVAL;
    }
    RVZ_HIP(hipStreamSynchronize(e->stream), e);
    if (slots == e->tslots && slots != 0) {   // same size: new limit, a fresh generation
        e->tmaxd = max_discs;
        return table_bump(e);
    }
    table_free(e);
    if (slots == 0) return RVZ_OK;
    const size_t stride = e->BS == 8 ? TabGeo<8>::STRIDE : TabGeo<6>::STRIDE;
    if (hipMalloc(reinterpret_cast<void**>(&e->tab), (size_t)slots * stride * 8) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&e->tclaim), (size_t)slots * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&e->tgen), 4) != hipSuccess) {
        table_free(e);
        e->err = "hipMalloc failed (rvz_play_table)";
        return RVZ_ENOMEM;
    }
    hipError_t st = hipMemset(e->tab, 0, (size_t)slots * stride * 8);   // tags 0: no generation
    if (st == hipSuccess) st = hipMemset(e->tclaim, 0, (size_t)slots * 4);
    if (st == hipSuccess) st = hipMemsetD32(e->tgen, 1u, 1);
    if (st == hipSuccess) st = hipDeviceSynchronize();
    if (st != hipSuccess) {
        table_free(e);
        e->err = std::string("rvz_play_table init: ") + hipGetErrorString(st);
        return RVZ_EHIP;
    }
    e->tslots = slots;
    e->tmaxd = max_discs;
    return RVZ_OK;
}

#ifdef RVZ_WALK_STATS
// tools/exp_play_walks.py: host uint64 [n][9] = g_wtime's 5 columns, then g_ftime's 4; zeroes both
int rvz_play_walk_read(int32_t n_games, uint64_t* out) {
    const int n = n_games < WALK_STATS_MAX ? n_games : WALK_STATS_MAX;
    std::vector<unsigned long long> a, b;
    if (take_rows(g_wtime, n, a) != RVZ_OK || take_rows(g_ftime, n, b) != RVZ_OK) return RVZ_EHIP;
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 5; ++k) out[(size_t)i * 9 + k] = a[(size_t)i * 5 + k];
        for (int k = 0; k < 4; ++k) out[(size_t)i * 9 + 5 + k] = b[(size_t)i * 4 + k];
    }
    return RVZ_OK;
}
#endif

// rvz_play's scratch: the offset of every block and the total, in 4-byte words, each block
// 16-byte aligned. First the queue words, zeroed per launch as one run of `queue` words: q_next
// (the task counter, padded to 4), q_done (one 64-bit {published | claimed} word per group, at
// most G), the pass gate's words (PlayArgs::gate: 8 XCDs x 128 bytes); then the leaf planes, need,
// the head-conv rows, logits and value. The forms with ahead rows (play_ahead_shape: leaves as
// bitboards, head-conv rows in LDS) use neither x nor work; with ahead rows on they keep two rows
// per game there instead of one in logits / value: ah_logits [2 G][NPOL] and ah_value [2 G]
// inside x, the slots' keys ah_key [G][3] (64-bit) inside work.
struct PlayScratch {
    int64_t q_next, q_done, gate, queue, x, need, work, logits, value, total;
    int64_t ah_logits, ah_value, ah_key;
};
static PlayScratch play_scratch(int64_t G, int NSQ, int NPOL) {
    const auto al4 = [](int64_t n) { return (n + 3) / 4 * 4; };
    int64_t at = 0;
    const auto take = [&](int64_t words) { const int64_t o = at; at += al4(words); return o; };
    PlayScratch s;
    s.q_next = take(4);
    s.q_done = take(2 * al4(G));
    s.gate = take(8 * 32);
    s.queue = at;
    s.x = take(G * 3 * NSQ);
    s.need = take(G);
    s.work = take(G * 192);
    s.logits = take(G * NPOL);
    s.value = take(G);
    s.total = at;
    s.ah_logits = s.x;
    s.ah_value = s.x + al4(2 * G * NPOL);
    s.ah_key = s.work;
    return s;
}
int64_t rvz_play_scratch_size(const rvz_engine* e) {
    if (!e) return RVZ_EINVAL;
    return play_scratch(e->v.G, e->NSQ, e->NPOL).total;
}

#ifndef RVZ_PLAY_GROUP
#define RVZ_PLAY_GROUP 4      // games per task of the queue schedule
#endif
// the pass gate's default (rvz_play_gate; measured on C3, profiles/r06c_gate_ab_*): a round opens
// when 0.8 of the XCD's running workgroups arrived or 400 us after a waiter's arrival; a workgroup
// arriving within 200 us of a round's opening joins it at once
// ahead rows (rvz_play_ahead): the default of the forms that have them
#ifndef RVZ_PLAY_AHEAD_DEFAULT
#define RVZ_PLAY_AHEAD_DEFAULT 1
#endif
#ifndef RVZ_PLAY_GATE_FRAC
#define RVZ_PLAY_GATE_FRAC 0.8
#endif
#ifndef RVZ_PLAY_GATE_US
#define RVZ_PLAY_GATE_US 400.0
#endif
#ifndef RVZ_PLAY_GATE_LATE_US
#define RVZ_PLAY_GATE_LATE_US 200.0
#endif
extern "C++" {
// T: the (board, filters) pair's H2Tile (rvz_h2.hip.h): k_play runs the evaluator's tile, T::OCC
// workgroups resident per CU
template <class T>
static int play_launch(rvz_engine* e, const View& v, const PlayArgs& pa) {
    constexpr int F = T::F, BS = T::BS;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->cfg.device) !=
            hipSuccess || cus <= 0)
        cus = 256;
    PlayArgs a = pa;
    if constexpr (play_ahead_shape<F, T::NB, BS>()) {
        // two rows per game: the game's own and its ahead slot (row G + g), in the scratch's x
        // part, which this form does not use (3 NSQ >= 2 NPOL + 4 words per game)
        static_assert(3 * Geo<BS>::NSQ >= 2 * Geo<BS>::NPOL + 8, "ahead rows fit");
        if (a.ahead) {
            const PlayScratch sc = play_scratch(v.G, e->NSQ, e->NPOL);
            float* scratch = a.x - sc.x;
            a.logits = scratch + sc.ah_logits;
            a.value = scratch + sc.ah_value;
            a.ah_key = reinterpret_cast<uint64_t*>(scratch + sc.ah_key);
        }
    } else {
        a.ahead = 0;
    }
    const int slots = cus * T::OCC;
    dim3 grid;
    if (a.q_next) {     // queue: one persistent workgroup per resident slot, groups of gpw games
        if (a.gpw <= 0) a.gpw = RVZ_PLAY_GROUP;
        if (a.gpw > play_gpw_max<F, BS>()) a.gpw = play_gpw_max<F, BS>();
        a.n_groups = (v.G + a.gpw - 1) / a.gpw;
        grid = dim3(a.n_groups < slots ? a.n_groups : slots);
        RVZ_HIP(fill32_async(a.q_next, 0u, (size_t)play_scratch(v.G, e->NSQ, e->NPOL).queue,
                             e->stream), e);
    } else {            // static: workgroup w owns group w for every ply
        if (a.gpw <= 0) a.gpw = (v.G + slots - 1) / slots;
        if (a.gpw > play_gpw_max<F, BS>()) a.gpw = play_gpw_max<F, BS>();
        a.n_groups = (v.G + a.gpw - 1) / a.gpw;
        grid = dim3(a.n_groups);
    }
    PlayCtx ctx;
    ctx.v = v;
    ctx.a = a;
    hipLaunchKernelGGL((k_play<T::F, T::NB, T::CTW, T::PTW, T::BS, T::OCC>), grid, dim3(256), 0,
                       e->stream, ctx);
    return launch_check(e, "k_play");
}
}  // extern "C++"

#ifdef RVZ_PLAY_TIMING
// tools/exp_play_phases.py: host copy of g_play_t (n workgroups x PLAY_T_SLOTS = 16) and g_pass_t
// (n x 6), then zeroed
int rvz_play_timing_read(uint64_t* host, int n) {
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_play_t), (size_t)n * PLAY_T_SLOTS * 8) != hipSuccess)
        return RVZ_EHIP;
    if (hipMemcpyFromSymbol(host + (size_t)n * PLAY_T_SLOTS, HIP_SYMBOL(g_pass_t),
                            (size_t)n * 6 * 8) != hipSuccess)
        return RVZ_EHIP;
    std::vector<unsigned long long> z((size_t)16384 * PLAY_T_SLOTS, 0ull);
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_pass_t), z.data(), (size_t)16384 * 6 * 8) != hipSuccess)
        return RVZ_EHIP;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_play_t), z.data(), z.size() * 8) == hipSuccess
               ? RVZ_OK : RVZ_EHIP;
}
#endif

// The pass gate's three words for a launch: rvz_play_gate's setting (fraction < 0: the
// RVZ_PLAY_GATE_* defaults), the environment's RVZ_PLAY_GATE ("fraction,us[,late_us]" or "off")
// overriding it. frac: Q16, 0 = off (always off without the queue); t, late: 100 MHz ticks.
struct PlayGate {
    unsigned frac, t, late;
};
static PlayGate play_gate_setting(const rvz_engine* e, bool queue) {
    double frac = e->gate_frac, us = e->gate_us, late = e->gate_late_us;
    if (frac < 0.0) {
        frac = RVZ_PLAY_GATE_FRAC;
        us = RVZ_PLAY_GATE_US;
        late = RVZ_PLAY_GATE_LATE_US;
    }
    if (const char* gs = getenv("RVZ_PLAY_GATE")) {
        double f = 0.0, u = 0.0, l = 0.0;
        const int n = sscanf(gs, "%lf,%lf,%lf", &f, &u, &l);
        frac = n >= 2 ? f : 0.0;
        us = u;
        late = n >= 3 ? l : 0.0;
    }
    PlayGate g;
    g.frac = (queue && frac > 0.0 && us > 0.0) ? (unsigned)(fmin(frac, 1.0) * 65536.0 + 0.5) : 0u;
    g.t = (unsigned)(us * 100.0);
    g.late = late > 0.0 ? (unsigned)(late * 100.0) : 0u;
    return g;
}

int rvz_play(rvz_engine* e, const rvz_play_args* a) {
    const Range trace_range("rvz.play (fused search + h2 evaluator)");
    if (!e || !a) return RVZ_EINVAL;
    if (!a->params || !a->blob || !a->scratch || !a->seeds || !a->plies_done || !a->out_idx ||
        !a->out_p || (a->reset && !a->games_done) || a->plies < 1 || a->blocks < 0 ||
        !h2_tile_ok(e->BS, a->filters) || a->games_per_workgroup < -PLAY_GPW_MAX ||
        e->cfg.leaf_dtype != RVZ_LEAF_F32) {
        e->err = "rvz_play: invalid arguments";
        return RVZ_EINVAL;
    }
    if ((((uintptr_t)a->params | (uintptr_t)a->blob | (uintptr_t)a->scratch) & 15) != 0) {
        e->err = "rvz_play: params, blob and scratch must be 16-byte aligned";
        return RVZ_EINVAL;
    }
    if (in_search(e, "rvz_play")) return RVZ_EINVAL;
    View v = e->v;
    v.live = nullptr;       // the workgroups compact their own rows
    v.row_of = nullptr;
    v.live_total = nullptr;
    v.stats = nullptr;
    if ((a->rec_black || a->rec_white || a->rec_side || a->rec_p) &&
        !(a->rec_black && a->rec_white && a->rec_side && a->rec_p)) {
        e->err = "rvz_play: rec_black, rec_white, rec_side and rec_p go together";
        return RVZ_EINVAL;
    }
    PlayArgs pa;
    // the network
    pa.prm = a->params;
    pa.L = make_layout(a->filters, a->blocks, e->BS);
    pa.blob = a->blob;
    pa.n_blocks = a->blocks;
    pa.ovf = a->ovf;
    // the scratch. games_per_workgroup > 0: static groups of that size; <= 0: the task queue,
    // groups of -games_per_workgroup games (0: RVZ_PLAY_GROUP), with the per-XCD pass gate
    // (rvz_play.hip.h play_gate; 8x8 at 128 / 256 filters) whose words are zeroed with the queue's
    const PlayScratch sc = play_scratch(v.G, e->NSQ, e->NPOL);
    const bool queue = a->games_per_workgroup <= 0;
    pa.q_next = queue ? reinterpret_cast<unsigned*>(a->scratch + sc.q_next) : nullptr;
    pa.q_done = queue ? reinterpret_cast<unsigned long long*>(a->scratch + sc.q_done) : nullptr;
    pa.gate = queue ? reinterpret_cast<unsigned long long*>(a->scratch + sc.gate) : nullptr;
    pa.x = a->scratch + sc.x;
    pa.need = reinterpret_cast<int32_t*>(a->scratch + sc.need);
    pa.work = a->scratch + sc.work;
    pa.logits = a->scratch + sc.logits;
    pa.value = a->scratch + sc.value;
    // the schedule
    pa.n_groups = 0;
    pa.gpw = queue ? -a->games_per_workgroup : a->games_per_workgroup;
    const PlayGate gate = play_gate_setting(e, queue);
    pa.gate_frac = gate.frac;
    pa.gate_t = gate.t;
    pa.gate_late = gate.late;
    // the queue's bounded wait (device error 16 when exceeded); RVZ_PLAY_SPIN_LIMIT lowers it to
    // inject the timeout in tests (tests/test_gpu_play.py)
    pa.spin_limit = 1u << 26;
    if (const char* sl = getenv("RVZ_PLAY_SPIN_LIMIT")) pa.spin_limit = (unsigned)strtoul(sl, nullptr, 10);
    // the one-board shape for the C2 pair's passes with one live board (on; RVZ_PLAY_SINGLE_PASS=0
    // runs the pair shape everywhere: the tests' and same-library A/Bs' switch, the same games)
    pa.single_pass = 1;
    if (const char* sp = getenv("RVZ_PLAY_SINGLE_PASS")) pa.single_pass = atoi(sp) != 0;
    // the search and the plies. A search of one batch (S <= B) evaluates it: its leaf is the
    // root, which the act needs expanded (the deferred last batch is dead only from the second
    // batch on). Forced searches go with the deferred last batch (hence E >= 2): the act then
    // takes the visit counts alone
    pa.S = e->cfg.num_simulations;
    pa.B = e->cfg.batch_size;
    pa.skip_last = a->skip_last_eval && pa.S > pa.B ? 1 : 0;
    pa.skip_forced = a->skip_forced_roots && pa.skip_last ? 1 : 0;
    pa.plies = a->plies;
    pa.budget = a->ply_budget;
    pa.temperature = a->temperature;
    pa.reset = a->reset ? 1 : 0;
    pa.seeds = a->seeds;
    pa.stride = a->seed_stride;
    // outputs: per game, then the launch's counters
    pa.ply_ctr = a->plies_done;
    pa.done = a->games_done;
    pa.out_idx = a->out_idx;
    pa.out_p = a->out_p;
    pa.hist = a->hist;
    pa.rows = reinterpret_cast<unsigned long long*>(a->rows_evaluated);
    pa.unread = reinterpret_cast<unsigned long long*>(a->rows_unread);
    pa.roots_unread = reinterpret_cast<unsigned long long*>(a->roots_unread);
    pa.tstats = reinterpret_cast<unsigned long long*>(a->table_stats);
    // ahead rows (on for the 8x8 / 64-filter pair shape, the only form that has them;
    // rvz_play_ahead sets it, RVZ_PLAY_AHEAD overrides: 0 off, 1 fill the empty board slots,
    // 2 also in place of holding an odd row; the same games with any setting)
    pa.ahead = e->ahead < 0 ? RVZ_PLAY_AHEAD_DEFAULT : e->ahead;
    if (const char* ah = getenv("RVZ_PLAY_AHEAD")) pa.ahead = atoi(ah);
    if (pa.ahead < 0 || pa.ahead > 2 || !pa.single_pass) pa.ahead = 0;   // (the pair shape
                                       // everywhere is the launch as it was: no ahead rows either)
    pa.ah_key = nullptr;
    pa.ah_stats = reinterpret_cast<unsigned long long*>(e->ahead_stats);
    // self-play records
    pa.rec_black = a->rec_black;
    pa.rec_white = a->rec_white;
    pa.rec_side = a->rec_side;
    pa.rec_p = a->rec_p;
    // the cross-game table (rvz_play_table)
    pa.tab = nullptr;
    pa.tclaim = nullptr;
    pa.tgen = nullptr;
    pa.tmask = 0;
    pa.tmaxd = 0;
    if (e->tab) {
        if (e->tab_blob != a->blob) {   // other weights than the generation's rows came from
            if (e->tab_blob) {
                // the generation bump is a kernel on the stream: inside a capture it would be
                // recorded and replayed, invalidating the table on every replay
                hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
                if (hipStreamIsCapturing(e->stream, &cs) == hipSuccess &&
                    cs != hipStreamCaptureStatusNone) {
                    e->err = "rvz_play: another weight blob than the table's while the stream is "
                             "capturing (play once eagerly with this evaluator before capturing)";
                    return RVZ_EINVAL;
                }
                const int r = table_bump(e);
                if (r != RVZ_OK) return r;
            }
            e->tab_blob = a->blob;
        }
        pa.tab = e->tab;
        pa.tclaim = e->tclaim;
        pa.tgen = e->tgen;
        pa.tmask = (unsigned)(e->tslots - 1);
        pa.tmaxd = e->tmaxd;
    }
    e->searching = 0;
    int r = RVZ_EINVAL;
    h2_tile(e->BS, a->filters, [&](auto t) { r = play_launch<decltype(t)>(e, v, pa); });
    return r;
}

}  // extern "C"
