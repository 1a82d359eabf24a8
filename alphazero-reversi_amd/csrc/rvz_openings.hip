// rvz_openings.hip — the distinct positions after d plies under the engine's own rules
// (rvz_openings), and the pool row a seed picks (rvz_opening_index); contracts in include/rvz.h.
//
// A level-by-level frontier expansion with de-duplication. The scratch holds the current level's
// rows, the next level's candidates, a word per parent, a word per candidate and an open-addressed
// table of candidate indices. k_op_init writes level 0; every further level is five consecutive
// launches on the caller's stream, each reading the level's size from the scratch's header, so the
// host never learns a count and no workgroup waits on another:
//   k_op_count   a lane per parent: its live and its finished children by the engine's make_move;
//                the same launch empties the table
//   k_op_offsets one workgroup: the exclusive scan of the live counts (the chunked workgroup scan
//                of rvz_wave.hip.h, as k_rec_scan), the sum of the finished ones; a level whose
//                candidates exceed max_rows sets the header's row count to -1, which turns every
//                later launch into a no-op
//   k_op_expand  a lane per parent: its live children at its offset, in square order
//   k_op_insert  a lane per candidate: open addressing as rvz_merge.hip's k_insert. A candidate
//                claims an empty slot with a CAS or meets the candidate that holds it and compares
//                keys, read from the candidate arrays (immutable in this launch); equal keys:
//                atomicMin of its own index into the slot. A slot's key never changes once
//                claimed, so after the launch the slot holds the lowest index of its position:
//                which slot a position took is timing, which candidate is its first is not
//   k_op_compact one workgroup: a candidate is kept iff its slot holds its own index; the scan
//                of the flags gives its row in the next level (for the last level: in the
//                caller's outputs, with the status rows, *out_m and out_stats)
// Integer atomics only. Every output element is written once.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/rvz.h"
#include "rvz_host.hip.h"
#include "rvz_openings.hip.h"
#include "rvz_rules.hip.h"
#include "rvz_wave.hip.h"

namespace {

using namespace rvz;

constexpr int OP_THREADS = 256;                  // the lane-per-row kernels
constexpr int SCAN_THREADS = 1024;               // the two one-workgroup kernels: 16 waves
constexpr int SCAN_WAVES = SCAN_THREADS / 64;
constexpr int EMPTY = INT_MAX;                   // a table slot no candidate has claimed

// the header's words
enum { H_ROWS = 0, H_CAND = 1, H_DROPPED = 2, H_DUPS = 3, H_MAXCAND = 4, H_WORDS = 8 };

struct Rows {                                    // a level's rows, or its candidates
    uint64_t *black, *white;
    int32_t* side;
};

struct Layout {                                  // the scratch's parts
    int64_t* hdr;
    Rows cur, cand;
    int32_t *cnt, *off, *slot_of, *table;
    int64_t bytes = -1;                          // -1: bad arguments
    int32_t slots = 0;
    Layout(int32_t bs, int32_t max_rows, void* scratch) {
        if (!board_ok(bs) || max_rows < 1 || (int64_t)max_rows * 4 > INT32_MAX) return;
        int lg = 1;
        while (((int64_t)1 << lg) < 2 * (int64_t)max_rows) ++lg;
        slots = (int32_t)1 << lg;                // < 2^31: max_rows < 2^29
        const int64_t R = max_rows;
        Carver c(scratch);
        hdr = c.take<int64_t>(H_WORDS);
        for (Rows* r : {&cur, &cand}) {
            r->black = c.take<uint64_t>(R);
            r->white = c.take<uint64_t>(R);
            r->side = c.take<int32_t>(R);
        }
        cnt = c.take<int32_t>(R);
        off = c.take<int32_t>(R);
        slot_of = c.take<int32_t>(R);
        table = c.take<int32_t>(slots);
        bytes = c.at;
    }
};

__device__ __forceinline__ uint32_t key_hash(uint64_t b, uint64_t w, int side) {
    uint64_t h = (b * 0x9E3779B97F4A7C15ull) ^ (w * 0xC2B2AE3D27D4EB4Full) ^ (uint64_t)side;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    return (uint32_t)h;
}

__device__ __forceinline__ void status_row(int32_t* __restrict__ out_status, int64_t j, int side) {
    int32_t* st = out_status + 4 * j;            // a fresh start: not over, no winner, no passes
    st[0] = side;
    st[1] = 0;
    st[2] = -1;
    st[3] = 0;
}

__device__ __forceinline__ void write_stats(const int64_t* hdr, int64_t rows, int64_t cand,
                                            int64_t dups, int64_t maxcand,
                                            int32_t* __restrict__ out_m,
                                            int64_t* __restrict__ out_stats) {
    *out_m = (int32_t)rows;
    out_stats[0] = rows;
    out_stats[1] = cand;
    out_stats[2] = hdr[H_DROPPED];
    out_stats[3] = dups;
    out_stats[4] = maxcand;
    out_stats[5] = out_stats[6] = out_stats[7] = 0;
}

// level 0: the start position, black to move; with last (plies == 0) it is the output
template <int BS>
__global__ __launch_bounds__(64) void k_op_init(int64_t* __restrict__ hdr, Rows cur, int last,
                                                uint64_t* __restrict__ out_black,
                                                uint64_t* __restrict__ out_white,
                                                int32_t* __restrict__ out_status,
                                                int32_t* __restrict__ out_m,
                                                int64_t* __restrict__ out_stats) {
    if (threadIdx.x != 0) return;
    hdr[H_ROWS] = 1;
    hdr[H_CAND] = 1;
    hdr[H_DROPPED] = 0;
    hdr[H_DUPS] = 0;
    hdr[H_MAXCAND] = 1;
    hdr[5] = hdr[6] = hdr[7] = 0;
    cur.black[0] = Geo<BS>::START_BLACK;
    cur.white[0] = Geo<BS>::START_WHITE;
    cur.side[0] = 1;
    if (last) {
        out_black[0] = Geo<BS>::START_BLACK;
        out_white[0] = Geo<BS>::START_WHITE;
        status_row(out_status, 0, 1);
        write_stats(hdr, 1, 1, 0, 1, out_m, out_stats);
    }
}

// parent i's children over its legal squares in increasing index: f(child) for every live one;
// returns the number of finished ones
template <int BS, class F>
__device__ __forceinline__ int for_children(const Rows& cur, int i, F f) {
    const GameS parent = {cur.black[i], cur.white[i], cur.side[i], 0, -1, 0};
    uint64_t m = legal<BS>(mine(parent), theirs(parent));
    int finished = 0;
    while (m) {
        const int sq = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        GameS child = parent;
        make_move<BS>(child, sq);
        if (child.over) ++finished;
        else f(child);
    }
    return finished;
}

template <int BS>
__global__ __launch_bounds__(OP_THREADS) void k_op_count(const int64_t* __restrict__ hdr,
                                                         Rows cur, int32_t* __restrict__ cnt,
                                                         int32_t* __restrict__ table, int slots) {
    const int64_t n = hdr[H_ROWS];                                      // <= max_rows; -1: overflow
    if (n < 0) return;
    const int64_t step = (int64_t)gridDim.x * OP_THREADS;
    const int64_t first = (int64_t)blockIdx.x * OP_THREADS + threadIdx.x;
    for (int64_t s = first; s < slots; s += step) table[s] = EMPTY;
    for (int64_t i = first; i < n; i += step) {
        int live = 0;
        const int finished = for_children<BS>(cur, (int)i, [&](const GameS&) { ++live; });
        cnt[i] = live | (finished << 8);                                // each at most S*S - 4
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void k_op_offsets(int64_t* hdr,
                                                             const int32_t* __restrict__ cnt,
                                                             int32_t* __restrict__ off,
                                                             int max_rows) {
    __shared__ int64_t part[2][SCAN_WAVES];
    __shared__ int64_t sums[SCAN_WAVES];
    const int64_t n = hdr[H_ROWS];
    if (n < 0) return;                                                  // block-uniform
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int64_t carry = 0, finished = 0;
    int c = 0;
    for (int64_t base = 0; base < n; base += SCAN_THREADS, c ^= 1) {    // block-uniform trip count
        const int64_t i = base + threadIdx.x;
        int64_t live = 0;
        if (i < n) {
            const int32_t w = cnt[i];
            live = w & 0xff;
            finished += w >> 8;
        }
        const int64_t upto = block_scan(live, lane, wave, SCAN_WAVES, part[c], carry);
        // a total above max_rows stops the level before any offset is used
        if (i < n) off[i] = (int32_t)(upto - live < INT_MAX ? upto - live : INT_MAX);
    }
    const int64_t all = block_reduce<1>(&finished, lane, wave, SCAN_WAVES, sums, Sum());
    if (threadIdx.x == 0) {
        hdr[H_CAND] = carry;
        hdr[H_DROPPED] += all;
        if (carry > hdr[H_MAXCAND]) hdr[H_MAXCAND] = carry;
        if (carry > max_rows) hdr[H_ROWS] = -1;
    }
}

template <int BS>
__global__ __launch_bounds__(OP_THREADS) void k_op_expand(const int64_t* __restrict__ hdr,
                                                          Rows cur,
                                                          const int32_t* __restrict__ off,
                                                          Rows cand) {
    const int64_t n = hdr[H_ROWS];
    if (n < 0) return;
    const int64_t step = (int64_t)gridDim.x * OP_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * OP_THREADS + threadIdx.x; i < n; i += step) {
        int at = off[i];                         // at + the parent's live children <= H_CAND <= max_rows
        for_children<BS>(cur, (int)i, [&](const GameS& child) {
            cand.black[at] = child.black;
            cand.white[at] = child.white;
            cand.side[at] = child.side;
            ++at;
        });
    }
}

__global__ __launch_bounds__(OP_THREADS) void k_op_insert(const int64_t* __restrict__ hdr,
                                                          Rows cand, int32_t* table, int slots,
                                                          int32_t* __restrict__ slot_of) {
    if (hdr[H_ROWS] < 0) return;
    const int64_t n = hdr[H_CAND];                                      // <= max_rows
    const uint32_t mask = (uint32_t)slots - 1u;
    const int64_t step = (int64_t)gridDim.x * OP_THREADS;
    for (int64_t ii = (int64_t)blockIdx.x * OP_THREADS + threadIdx.x; ii < n; ii += step) {
        const int i = (int)ii;
        const uint64_t b = cand.black[i], w = cand.white[i];
        const int side = cand.side[i];
        uint32_t slot = key_hash(b, w, side) & mask;
        // at most max_rows <= slots / 2 slots are ever claimed, so an empty one always ends the
        // walk; the bound only keeps the loop finite whatever happens
        for (int probes = 0; probes < slots; ++probes) {
            // a slot only ever goes from EMPTY to an index of one position, then down among that
            // position's indices: a stale read can only show EMPTY (the CAS decides) or another
            // index with the same key
            int s = __hip_atomic_load(&table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (s == EMPTY) {
                s = atomicCAS(&table[slot], EMPTY, i);
                if (s == EMPTY) break;                                  // claimed
            }
            if (cand.black[s] == b && cand.white[s] == w && cand.side[s] == side) {
                atomicMin(&table[slot], i);
                break;
            }
            slot = (slot + 1u) & mask;
        }
        slot_of[i] = (int32_t)slot;
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void k_op_compact(
    int64_t* hdr, Rows cand, const int32_t* __restrict__ table,
    const int32_t* __restrict__ slot_of, Rows next, int last, int32_t* __restrict__ out_status,
    int32_t* __restrict__ out_m, int64_t* __restrict__ out_stats) {
    __shared__ int64_t part[2][SCAN_WAVES];
    if (hdr[H_ROWS] < 0) {                                              // block-uniform
        if (last && threadIdx.x == 0)
            write_stats(hdr, -1, hdr[H_CAND], hdr[H_DUPS], hdr[H_MAXCAND], out_m, out_stats);
        return;
    }
    const int64_t n = hdr[H_CAND];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int64_t carry = 0;
    int c = 0;
    for (int64_t base = 0; base < n; base += SCAN_THREADS, c ^= 1) {    // block-uniform trip count
        const int64_t i = base + threadIdx.x;
        const int64_t keep = i < n && table[slot_of[i]] == (int32_t)i ? 1 : 0;
        const int64_t j = block_scan(keep, lane, wave, SCAN_WAVES, part[c], carry) - keep;
        if (keep) {                                                     // j < kept <= n <= max_rows
            const int side = cand.side[i];
            next.black[j] = cand.black[i];
            next.white[j] = cand.white[i];
            if (last) status_row(out_status, j, side);
            else next.side[j] = side;
        }
    }
    if (threadIdx.x == 0) {
        const int64_t dups = hdr[H_DUPS] + (n - carry);
        hdr[H_ROWS] = carry;
        hdr[H_DUPS] = dups;
        if (last) write_stats(hdr, carry, n, dups, hdr[H_MAXCAND], out_m, out_stats);
    }
}

__global__ __launch_bounds__(OP_THREADS) void k_opening_index(int n_pool, int n,
                                                              const uint32_t* __restrict__ seed32,
                                                              uint32_t salt,
                                                              int32_t* __restrict__ out_index) {
    const int i = blockIdx.x * OP_THREADS + threadIdx.x;
    if (i < n) out_index[i] = opening_index(seed32[i], salt, n_pool);
}

}  // namespace

extern "C" int64_t rvz_openings_scratch_size(int32_t bs, int32_t max_rows) {
    return Layout(bs, max_rows, nullptr).bytes;
}

extern "C" int rvz_openings(int32_t bs, int32_t plies, int32_t max_rows, void* scratch,
                            int32_t* out_m, uint64_t* out_black, uint64_t* out_white,
                            int32_t* out_status, int64_t* out_stats, void* stream) {
    const Layout L(bs, max_rows, scratch);
    if (L.bytes < 0 || plies < 0 || plies > bs * bs - 4) return RVZ_EINVAL;
    if (!scratch_ok(scratch) || !out_m || !out_black || !out_white || !out_status || !out_stats)
        return RVZ_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const Rows out = {out_black, out_white, nullptr};
    launch_bs_unchecked(bs, k_op_init<8>, k_op_init<6>, dim3(1), dim3(64), s, L.hdr, L.cur,
                        (int)(plies == 0), out_black, out_white, out_status, out_m, out_stats);
    const Geometry rows = strided(max_rows, OP_THREADS, OP_THREADS);
    const Geometry clear = strided(L.slots, OP_THREADS, OP_THREADS);   // k_op_count also empties the table
    for (int level = 1; level <= plies; ++level) {
        const int last = level == plies;
        launch_bs_unchecked(bs, k_op_count<8>, k_op_count<6>, clear.grid, clear.block, s,
                            (const int64_t*)L.hdr, L.cur, L.cnt, L.table, L.slots);
        hipLaunchKernelGGL(k_op_offsets, dim3(1), dim3(SCAN_THREADS), 0, s, L.hdr,
                           (const int32_t*)L.cnt, L.off, max_rows);
        launch_bs_unchecked(bs, k_op_expand<8>, k_op_expand<6>, rows.grid, rows.block, s,
                            (const int64_t*)L.hdr, L.cur, (const int32_t*)L.off, L.cand);
        hipLaunchKernelGGL(k_op_insert, rows.grid, rows.block, 0, s, (const int64_t*)L.hdr, L.cand,
                           L.table, L.slots, L.slot_of);
        hipLaunchKernelGGL(k_op_compact, dim3(1), dim3(SCAN_THREADS), 0, s, L.hdr, L.cand,
                           (const int32_t*)L.table, (const int32_t*)L.slot_of, last ? out : L.cur,
                           last, out_status, out_m, out_stats);
    }
    return last_launch();
}

extern "C" int rvz_opening_index(int32_t n_pool, int32_t n, const uint32_t* seed32, uint32_t salt,
                                 int32_t* out_index, void* stream) {
    if (n_pool < 1 || n < 0 || (n > 0 && (!seed32 || !out_index))) return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    const Geometry g = thread_per_row(n);
    hipLaunchKernelGGL(k_opening_index, g.grid, g.block, 0, (hipStream_t)stream, n_pool, n, seed32,
                       salt, out_index);
    return last_launch();
}
