// rvz_engine_host.h — the engine's host state and launch helpers, shared by the two translation
// units behind the engine's C-ABI: csrc/rvz_engine.hip (the pull-style search, the env, the rest)
// and csrc/rvz_play.hip (rvz_play and its table and gate). Private to csrc/, host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/rvz.h"
#include "rvz_host.hip.h"
#include "rvz_search.hip.h"

using namespace rvz;

struct rvz_engine {
    rvz_config cfg;
    int BS, NSQ, NPOL, E, M;
    hipStream_t stream = nullptr;
    int next_batch = 0;  // batches issued in the current search
    int32_t* live_buf = nullptr;    // rvz_search_compact: [E] live counts + [G] row map + total
    unsigned long long* live_total = nullptr;
    int live_dirty = 0;             // a k_step counted since the last k_act zeroed the counts
    int searching = 0;
    // a submitted batch whose expand + backup runs at the start of the next launch (k_step/k_act)
    int pending = 0;
    const float* pend_policy = nullptr;
    const float* pend_value = nullptr;
    int pend_is_logits = 0;
    int64_t counters[2] = {0, 0};
    View v;
    unsigned long long* stats_buf = nullptr;
    // launch timing (rvz_timing_enable): HIP event pairs around k_step / k_act on the stream
    int timing = 0;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::vector<std::pair<int, size_t>> ev_marks;  // (kind 0 = k_step, 1 = k_act, first event)
    std::vector<void*> allocs;
    std::string err;
    // rvz_play_table: the cross-game NN-output table (tab null: off)
    unsigned long long* tab = nullptr;
    unsigned* tclaim = nullptr;
    unsigned* tgen = nullptr;
    int64_t tslots = 0;
    int tmaxd = 0;
    const void* tab_blob = nullptr;   // the weight blob the current generation's rows came from
    // rvz_play_gate: the per-XCD pass gate of the 10x128 k_play form (fraction < 0: the default)
    double gate_frac = -1.0, gate_us = 0.0, gate_late_us = 0.0;
    // rvz_play_ahead: ahead rows of the 8x8 / 64-filter k_play form (< 0: the default)
    int ahead = -1;
    int64_t* ahead_stats = nullptr;   // rvz_play_ahead_stats: device int64 [2], or null
    // the device's g_noise_err word (rvz_dirichlet_noise's exhaustion flag), read by rvz_check
    int32_t* noise_err = nullptr;
    // rvz_env_openings: the engine's copy of the pool (black, white, side, the validation's word)
    void* open_buf = nullptr;
};

#define RVZ_HIP(call, e)                                                                   \
    do {                                                                                   \
        hipError_t _s = (call);                                                            \
        if (_s != hipSuccess) {                                                            \
            (e)->err = std::string(#call) + ": " + hipGetErrorString(_s);                  \
            return RVZ_EHIP;                                                               \
        }                                                                                  \
    } while (0)

static int launch_check(rvz_engine* e, const char* what) {
    hipError_t s = hipGetLastError();
    if (s != hipSuccess) {
        e->err = std::string(what) + ": " + hipGetErrorString(s);
        return RVZ_EHIP;
    }
    e->counters[1] += 1;
    return RVZ_OK;
}

static int grid_games(int G) { return (G + WPB - 1) / WPB; }

// The launch of a per-game kernel (one wave per game) for the engine's board on its stream. The
// unchecked form is for the callers that have work between the launch and its launch_check.
template <class... P, class... A>
static void launch_games_unchecked(rvz_engine* e, void (*k8)(P...), void (*k6)(P...), A... args) {
    launch_bs_unchecked(e->BS, k8, k6, dim3(grid_games(e->v.G)), dim3(WPB * WAVE), e->stream,
                        args...);
}
template <class... P, class... A>
static int launch_games(rvz_engine* e, const char* what, void (*k8)(P...), void (*k6)(P...),
                        A... args) {
    launch_games_unchecked(e, k8, k6, args...);
    return launch_check(e, what);
}

// true, with the error text set: a setting that may not change while a search is under way
static bool in_search(rvz_engine* e, const char* name) {
    if (!e->pending && !(e->searching && e->next_batch > 0)) return false;
    e->err = std::string(name) + " inside a search";
    return true;
}

// Host helpers both units call, each defined once with its kernel; hidden, so that the library
// exports nothing but include/rvz.h. fill32_async (csrc/rvz_engine.hip, k_fill32): a stream-ordered
// 32-bit fill. table_bump (csrc/rvz_play.hip, k_table_bump): a new generation of the cross-game
// table (rvz_play_table); table_free (csrc/rvz_play.hip): the table gone.
#define RVZ_HIDDEN __attribute__((visibility("hidden")))
RVZ_HIDDEN hipError_t fill32_async(void* p, uint32_t v, size_t n, hipStream_t st);
RVZ_HIDDEN int table_bump(rvz_engine* e);
RVZ_HIDDEN void table_free(rvz_engine* e);

#ifdef RVZ_WALK_STATS
// the first n rows of a per-game device counter table copied to the host; the table is then zeroed
template <class T, int N>
static int take_rows(T (&table)[WALK_STATS_MAX][N], int n, std::vector<T>& out) {
    out.assign((size_t)n * N, T(0));
    if (hipMemcpyFromSymbol(out.data(), HIP_SYMBOL(table), out.size() * sizeof(T)) != hipSuccess)
        return RVZ_EHIP;
    const std::vector<T> z((size_t)WALK_STATS_MAX * N, T(0));
    return hipMemcpyToSymbol(HIP_SYMBOL(table), z.data(), z.size() * sizeof(T)) == hipSuccess
               ? RVZ_OK : RVZ_EHIP;
}
#endif
