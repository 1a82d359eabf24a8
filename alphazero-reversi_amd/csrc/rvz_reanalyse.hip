// rvz_reanalyse.hip — the record side of replay reanalysis (rvz_replay_stale, rvz_replay_roots,
// rvz_replay_refresh; contract in include/rvz.h): the stalest rows of the ring chosen on the
// device, ring rows turned into the arrays rvz_env_set takes, and the fresh policy rows of the
// re-search written back over the old targets. The search between the last two is the engine's.
//
// Nothing floating-point is reduced across rows and every atomic is an integer one, so equal
// inputs give equal bytes. No workgroup waits on another: a call is a few consecutive launches.
//
// rvz_replay_stale, six launches: k_stale_clear zeroes the class histogram and the header;
// k_stale_hist, a grid-stride pass over the live rows, adds each eligible row to its age class
// (the lanes of a wavefront that share a class add once, into a histogram the workgroup keeps in
// LDS where the classes fit and flushes once); k_stale_pick, one workgroup, scans the
// classes to the threshold class T and the rows `take` still wanted from it; then a tiled stable
// compaction: k_stale_count leaves per tile the rows below T and the rows in T, k_stale_tiles, one
// workgroup, turns the pairs into exclusive prefixes (both in one 64-bit scan), and k_stale_write
// scans each tile again and stores a selected row's slot at (rows below T before it) + min(rows of
// T before it, take), the -1 tail behind them.
//
// rvz_replay_roots, two launches: a one-thread clear of the counter, then a lane per row.
//
// rvz_replay_refresh, three launches: k_ref_clear empties the slot table (rvz_slot_table.hip.h)
// and the counters; k_ref_rows, a wavefront per row, checks the row and enters (slot -> max r);
// k_ref_write, a wavefront per row, stores the row if it is its slot's winner. Both count through
// LDS and add once per workgroup.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rvz.h"
#include "rvz_host.hip.h"
#include "rvz_slot_table.hip.h"
#include "rvz_wave.hip.h"

namespace {

using namespace rvz;

constexpr int ST_THREADS = 1024;                 // one compaction tile: a row per thread
constexpr int ST_WAVES = ST_THREADS / 64;
constexpr int ST_MAX_CLASSES = 65536;
constexpr int ST_LDS_CLASSES = 2048;             // up to here a workgroup keeps its own histogram
constexpr int ST_HIST_ROWS = 2048;               // k_stale_hist: rows per workgroup and step
constexpr int REF_WPB = 16;                      // rvz_replay_refresh: rows (waves) per workgroup
constexpr int32_t REF_MAX_N = 1 << 30;

// ---------------------------------------------------------------- the stalest rows
// the scratch: head {T, take, count, stamps out of range}, hist [classes], tile [tiles][2]
struct StaleLayout {
    int64_t tiles, bytes;
    uint32_t *head, *hist, *tile;
    StaleLayout(int32_t capacity, int32_t classes, void* scratch)
        : tiles(((int64_t)capacity + ST_THREADS - 1) / ST_THREADS) {
        Carver c(scratch);
        head = c.take<uint32_t>(4);
        hist = c.take<uint32_t>(classes);
        tile = c.take<uint32_t>(2 * tiles);
        bytes = c.at;
    }
};

// logical row i's slot; start, i < capacity < 2^31, so the sum fits 32 unsigned bits
__device__ __forceinline__ int ring_slot(int start, int i, int capacity) {
    uint32_t s = (uint32_t)start + (uint32_t)i;
    if (s >= (uint32_t)capacity) s -= (uint32_t)capacity;
    return (int)s;
}

// a live row's age class, -1 if it is not eligible (stamp >= below), -2 if its stamp is negative
__device__ __forceinline__ int age_class(int stamp, int lo, int below) {
    if (stamp < 0) return -2;
    if (stamp >= below) return -1;
    return stamp > lo ? stamp - lo : 0;
}

__global__ __launch_bounds__(256) void k_stale_clear(uint32_t* __restrict__ head,
                                                     uint32_t* __restrict__ hist, int classes) {
    const int stride = gridDim.x * 256;
    for (int c = blockIdx.x * 256 + threadIdx.x; c < classes; c += stride) hist[c] = 0u;
    if (blockIdx.x == 0 && threadIdx.x < 4) head[threadIdx.x] = 0u;
}

// LOCAL: the workgroup adds into a histogram of its own in LDS (classes <= ST_LDS_CLASSES) and
// flushes the bins it touched once, so a ring whose rows share a few stamps does not send every
// add to the same few words of memory; else the adds go to memory directly.
template <bool LOCAL>
__global__ __launch_bounds__(256) void k_stale_hist(int capacity, const int32_t* __restrict__ stamp,
                                                    int start, int live, int lo, int below,
                                                    uint32_t* __restrict__ head,
                                                    uint32_t* __restrict__ hist) {
    __shared__ uint32_t local[LOCAL ? ST_LDS_CLASSES : 1];
    __shared__ uint32_t local_bad;
    const int classes = below - lo;
    if (LOCAL) {
        for (int c = threadIdx.x; c < classes; c += 256) local[c] = 0u;
        if (threadIdx.x == 0) local_bad = 0u;
        __syncthreads();
    }
    uint32_t* bins = LOCAL ? local : hist;
    uint32_t* bad_word = LOCAL ? &local_bad : &head[3];
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * 256;
    // whole wavefronts stay in the loop: the ballots below are the wave's
    for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63); base < live;
         base += stride) {
        const int64_t i = base + lane;
        int c = -1;
        if (i < live) c = age_class(stamp[ring_slot(start, (int)i, capacity)], lo, below);
        const uint64_t bad = __ballot(c == -2);
        if (bad && lane == 0) atomicAdd(bad_word, (uint32_t)__popcll(bad));
        uint64_t todo = __ballot(c >= 0);
        while (todo) {                           // one add per distinct class of the wavefront
            const int leader = __ffsll((long long)todo) - 1;
            const int lc = __shfl(c, leader, 64);
            const uint64_t same = __ballot(c == lc);
            if (lane == leader) atomicAdd(&bins[lc], (uint32_t)__popcll(same));
            todo &= ~same;
        }
    }
    if (LOCAL) {
        __syncthreads();
        for (int c = threadIdx.x; c < classes; c += 256) {
            const uint32_t v = local[c];
            if (v) atomicAdd(&hist[c], v);
        }
        if (threadIdx.x == 0 && local_bad) atomicAdd(&head[3], local_bad);
    }
}

// T: the smallest class whose inclusive prefix reaches n, take = n - its exclusive prefix; with
// fewer than n eligible rows T = classes (every class is below it) and take = 0
__global__ __launch_bounds__(ST_THREADS) void k_stale_pick(int classes, int n,
                                                           uint32_t* __restrict__ head,
                                                           const uint32_t* __restrict__ hist,
                                                           int32_t* __restrict__ out_count) {
    __shared__ int64_t part[2][ST_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t carry = 0;
    int flip = 0;
    for (int base = 0; base < classes; base += ST_THREADS, flip ^= 1) {
        const int c = base + threadIdx.x;
        const int64_t v = c < classes ? (int64_t)hist[c] : 0;
        const int64_t incl = block_scan(v, lane, wave, ST_WAVES, part[flip], carry);
        if (c < classes && incl - v < n && incl >= n) {        // one thread at most, and n > 0
            head[0] = (uint32_t)c;
            head[1] = (uint32_t)(n - (incl - v));
        }
    }
    if (threadIdx.x == 0) {                      // carry: the eligible rows
        if (carry < n) {
            head[0] = (uint32_t)classes;
            head[1] = 0u;
        }
        const int32_t count = (int32_t)(carry < n ? carry : n);
        head[2] = (uint32_t)count;
        out_count[0] = count;
        out_count[1] = (int32_t)head[3];
    }
}

// what a thread's row adds to its tile's pair: 1 if below T, 1 << 32 if in T
__device__ __forceinline__ uint64_t stale_item(int capacity, const int32_t* __restrict__ stamp,
                                               int start, int live, int lo, int below, uint32_t T,
                                               int64_t i, int* slot) {
    if (i >= live) return 0;
    *slot = ring_slot(start, (int)i, capacity);
    const int c = age_class(stamp[*slot], lo, below);
    if (c < 0) return 0;
    return (uint32_t)c < T ? 1ull : (uint32_t)c == T ? 1ull << 32 : 0ull;
}

__global__ __launch_bounds__(ST_THREADS) void k_stale_count(int capacity,
                                                            const int32_t* __restrict__ stamp,
                                                            int start, int live, int lo, int below,
                                                            const uint32_t* __restrict__ head,
                                                            uint32_t* __restrict__ tile) {
    __shared__ uint64_t part[ST_WAVES];
    int slot = 0;
    const uint64_t v = stale_item(capacity, stamp, start, live, lo, below, head[0],
                                  (int64_t)blockIdx.x * ST_THREADS + threadIdx.x, &slot);
    const uint64_t all = block_reduce<1>(&v, threadIdx.x & 63, threadIdx.x >> 6, ST_WAVES, part,
                                         Sum());
    if (threadIdx.x == 0) {
        tile[2 * (int64_t)blockIdx.x] = (uint32_t)all;
        tile[2 * (int64_t)blockIdx.x + 1] = (uint32_t)(all >> 32);
    }
}

// the pairs become exclusive prefixes in place; each half stays below 2^31, so one 64-bit scan
// carries both
__global__ __launch_bounds__(ST_THREADS) void k_stale_tiles(int64_t tiles,
                                                            uint32_t* __restrict__ tile) {
    __shared__ uint64_t part[2][ST_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    int flip = 0;
    for (int64_t base = 0; base < tiles; base += ST_THREADS, flip ^= 1) {
        const int64_t t = base + threadIdx.x;
        const uint64_t v = t < tiles ? (uint64_t)tile[2 * t] | (uint64_t)tile[2 * t + 1] << 32 : 0;
        const uint64_t excl = block_scan(v, lane, wave, ST_WAVES, part[flip], carry) - v;
        if (t < tiles) {
            tile[2 * t] = (uint32_t)excl;
            tile[2 * t + 1] = (uint32_t)(excl >> 32);
        }
    }
}

// workgroups [0, tiles) place their tile's selected rows; every thread of the grid then takes its
// share of the -1 tail [count, n)
__global__ __launch_bounds__(ST_THREADS) void k_stale_write(int capacity,
                                                            const int32_t* __restrict__ stamp,
                                                            int start, int live, int lo, int below,
                                                            int n, int64_t tiles,
                                                            const uint32_t* __restrict__ head,
                                                            const uint32_t* __restrict__ tile,
                                                            int32_t* __restrict__ out_slot) {
    __shared__ uint64_t part[ST_WAVES];
    const uint32_t T = head[0], take = head[1];
    if (blockIdx.x < tiles) {                    // uniform in the workgroup
        int slot = 0;
        const uint64_t v = stale_item(capacity, stamp, start, live, lo, below, T,
                                      (int64_t)blockIdx.x * ST_THREADS + threadIdx.x, &slot);
        uint64_t carry = (uint64_t)tile[2 * (int64_t)blockIdx.x] |
                         (uint64_t)tile[2 * (int64_t)blockIdx.x + 1] << 32;
        const uint64_t excl =
            block_scan(v, threadIdx.x & 63, threadIdx.x >> 6, ST_WAVES, part, carry) - v;
        const uint32_t below_T = (uint32_t)excl, in_T = (uint32_t)(excl >> 32);
        // a selected row's place is below count <= n: the rows below T number less than n, and
        // of T's rows the first `take` are placed
        if (v == 1ull || (v && in_T < take))
            out_slot[below_T + (in_T < take ? in_T : take)] = slot;
    }
    const int64_t stride = (int64_t)gridDim.x * ST_THREADS;
    for (int64_t j = (int64_t)head[2] + (int64_t)blockIdx.x * ST_THREADS + threadIdx.x; j < n;
         j += stride)
        out_slot[j] = -1;
}

// ---------------------------------------------------------------- ring rows as engine roots
__global__ void k_roots_clear(int32_t* __restrict__ out_bad) { *out_bad = 0; }

__global__ __launch_bounds__(256) void k_roots(int capacity, uint64_t board,
                                               const uint64_t* __restrict__ mover,
                                               const uint64_t* __restrict__ opponent, int n,
                                               const int32_t* __restrict__ slot,
                                               uint64_t* __restrict__ out_black,
                                               uint64_t* __restrict__ out_white,
                                               int32_t* __restrict__ out_status,
                                               int32_t* __restrict__ out_bad) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (r < n) {
        const int s = slot[r];
        uint64_t b = 0, w = 0;
        bool live = false;
        if (s >= 0 && s < capacity) {
            b = mover[s];
            w = opponent[s];
            live = !(b & w) && !((b | w) & ~board);
            bad = !live;
        } else {
            bad = s != -1;
        }
        out_black[r] = live ? b : 0;
        out_white[r] = live ? w : 0;
        // {side, over, winner, passed}: a live game with black to move, or a game that is over
        reinterpret_cast<int4*>(out_status)[r] = live ? make_int4(1, 0, -1, 0) : make_int4(1, 1, 0, 0);
    }
    const uint64_t bads = __ballot(bad);
    if (bads && (threadIdx.x & 63) == 0) atomicAdd(out_bad, (int32_t)__popcll(bads));
}

// ---------------------------------------------------------------- fresh targets into the ring
// the scratch: ok [n] (1: the row passed its checks), the table's key [T] and, behind it, val [T]
struct RefreshLayout {
    int64_t T, bytes;
    uint32_t *ok, *key, *val;
    RefreshLayout(int32_t n, void* scratch) : T(slot_table_entries(n)) {
        Carver c(scratch);
        ok = c.take<uint32_t>(n);
        key = c.take<uint32_t>(T);
        val = c.take<uint32_t>(T);
        bytes = c.at;
    }
};

__global__ __launch_bounds__(256) void k_ref_clear(uint32_t* __restrict__ table, int64_t words,
                                                   int32_t* __restrict__ out_counts) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += stride)
        table[i] = 0u;
    if (blockIdx.x == 0 && threadIdx.x < 2) out_counts[threadIdx.x] = 0;
}

// NPOL 65 | 37. The row's sum: lane l holds p[l] (0 from NPOL on), lane 0 adds p[64] to its own
// where there is one, then the xor butterfly of rvz_wave.hip.h.
template <int NPOL>
__global__ __launch_bounds__(REF_WPB * 64) void k_ref_rows(int capacity, int n,
                                                           const int32_t* __restrict__ slot,
                                                           const double* __restrict__ p,
                                                           const int32_t* __restrict__ idx,
                                                           uint32_t* __restrict__ ok,
                                                           uint32_t* __restrict__ key,
                                                           uint32_t* __restrict__ val,
                                                           uint32_t mask,
                                                           int32_t* __restrict__ out_counts) {
    __shared__ uint32_t skips;
    if (threadIdx.x == 0) skips = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * REF_WPB + (threadIdx.x >> 6);
    const bool row = r < n;                      // the whole wavefront
    const int s = row ? slot[r] : -1;
    bool good = row && s >= 0 && s < capacity && idx[r] != -2;
    if (good) {                                  // uniform in the wavefront
        const double* row = p + r * NPOL;
        double x = lane < NPOL ? row[lane] : 0.0;
        bool fine = x >= 0.0 && x < INFINITY;    // NaN fails
        if (NPOL > 64 && lane == 0) {
            const double last = row[64];
            fine = fine && last >= 0.0 && last < INFINITY;
            x += last;
        }
        const double sum = wave_sum(x);
        good = __ballot(!fine) == 0 && fabs(sum - 1.0) <= 1e-9;
    }
    if (row && lane == 0) {
        ok[r] = good ? 1u : 0u;
        if (good)
            slot_table_enter(key, val, mask, s, (int)r);
        else
            atomicAdd(&skips, 1u);
    }
    __syncthreads();                             // one add per workgroup
    if (threadIdx.x == 0 && skips) atomicAdd(&out_counts[1], (int32_t)skips);
}

template <int NPOL>
__global__ __launch_bounds__(REF_WPB * 64) void k_ref_write(int n, const int32_t* __restrict__ slot,
                                                            const double* __restrict__ p,
                                                            int32_t new_stamp,
                                                            const uint32_t* __restrict__ ok,
                                                            const uint32_t* __restrict__ key,
                                                            const uint32_t* __restrict__ val,
                                                            uint32_t mask,
                                                            float* __restrict__ policy,
                                                            int32_t* __restrict__ stamp,
                                                            int32_t* __restrict__ out_counts) {
    __shared__ uint32_t wins;
    if (threadIdx.x == 0) wins = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * REF_WPB + (threadIdx.x >> 6);
    if (r < n && ok[r]) {                        // the whole wavefront
        const int s = slot[r];
        if (slot_table_wins(key, val, mask, s, (int)r)) {
            const double* row = p + r * NPOL;
            float* out = policy + (int64_t)s * NPOL;
            if (lane < NPOL) out[lane] = (float)row[lane];
            if (lane == 0) {
                if (NPOL > 64) out[64] = (float)row[64];
                stamp[s] = new_stamp;
                atomicAdd(&wins, 1u);
            }
        }
    }
    __syncthreads();                             // one add per workgroup
    if (threadIdx.x == 0 && wins) atomicAdd(&out_counts[0], (int32_t)wins);
}

bool ring_ok(int32_t capacity, int32_t start, int32_t live) {
    return capacity >= 1 && live >= 1 && live <= capacity && start >= 0 && start < capacity;
}

}  // namespace

extern "C" int64_t rvz_replay_stale_scratch_size(int32_t capacity, int32_t classes) {
    if (capacity < 1 || classes < 1 || classes > ST_MAX_CLASSES) return -1;
    return StaleLayout(capacity, classes, nullptr).bytes;
}

extern "C" int rvz_replay_stale(int32_t capacity, const int32_t* stamp, int32_t start,
                                int32_t live, int32_t n, int32_t lo, int32_t below, void* scratch,
                                int64_t scratch_bytes, int32_t* out_slot, int32_t* out_count,
                                void* stream) {
    if (!ring_ok(capacity, start, live) || n < 0) return RVZ_EINVAL;
    if (lo < 0 || below <= lo || (int64_t)below - lo > ST_MAX_CLASSES) return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    const int classes = below - lo;
    if (!stamp || !out_slot || !out_count || !scratch_ok(scratch) ||
        scratch_bytes < rvz_replay_stale_scratch_size(capacity, classes))
        return RVZ_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const StaleLayout l(capacity, classes, scratch);
    const int64_t tiles = ((int64_t)live + ST_THREADS - 1) / ST_THREADS;    // <= l.tiles
    const Geometry c = strided(classes, 256, 256);
    hipLaunchKernelGGL(k_stale_clear, c.grid, c.block, 0, s, l.head, l.hist, classes);
    const Geometry h = strided(live, ST_HIST_ROWS, 256);
    hipLaunchKernelGGL(classes <= ST_LDS_CLASSES ? k_stale_hist<true> : k_stale_hist<false>, h.grid,
                       h.block, 0, s, capacity, stamp, start, live, lo, below, l.head, l.hist);
    hipLaunchKernelGGL(k_stale_pick, dim3(1), dim3(ST_THREADS), 0, s, classes, n, l.head,
                       (const uint32_t*)l.hist, out_count);
    hipLaunchKernelGGL(k_stale_count, dim3((unsigned)tiles), dim3(ST_THREADS), 0, s, capacity, stamp,
                       start, live, lo, below, (const uint32_t*)l.head, l.tile);
    hipLaunchKernelGGL(k_stale_tiles, dim3(1), dim3(ST_THREADS), 0, s, tiles, l.tile);
    const Geometry w = strided(n, ST_THREADS, ST_THREADS);     // the -1 tail strides
    const int64_t grid = tiles > (int64_t)w.grid.x ? tiles : (int64_t)w.grid.x;
    hipLaunchKernelGGL(k_stale_write, dim3((unsigned)grid), dim3(ST_THREADS), 0, s, capacity, stamp,
                       start, live, lo, below, n, tiles, (const uint32_t*)l.head,
                       (const uint32_t*)l.tile, out_slot);
    return last_launch();
}

extern "C" int rvz_replay_roots(int32_t board_size, int32_t capacity, const uint64_t* mover,
                                const uint64_t* opponent, int32_t n, const int32_t* slot,
                                uint64_t* out_black, uint64_t* out_white, int32_t* out_status,
                                int32_t* out_bad, void* stream) {
    if (!board_ok(board_size) || capacity < 1 || n < 0 || n > REF_MAX_N) return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    if (!mover || !opponent || !slot || !out_black || !out_white || !scratch_ok(out_status) ||
        !out_bad)
        return RVZ_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t board = board_size == 8 ? ~0ull : (1ull << 36) - 1;
    hipLaunchKernelGGL(k_roots_clear, dim3(1), dim3(1), 0, s, out_bad);
    const Geometry g = thread_per_row(n);
    hipLaunchKernelGGL(k_roots, g.grid, g.block, 0, s, capacity, board, mover, opponent, n, slot,
                       out_black, out_white, out_status, out_bad);
    return last_launch();
}

extern "C" int64_t rvz_replay_refresh_scratch_size(int32_t n) {
    if (n < 0 || n > REF_MAX_N) return -1;
    return RefreshLayout(n, nullptr).bytes;
}

extern "C" int rvz_replay_refresh(int32_t board_size, int32_t capacity, float* policy,
                                  int32_t* stamp, int32_t n, const int32_t* slot, const double* p,
                                  const int32_t* idx, int32_t new_stamp, void* scratch,
                                  int64_t scratch_bytes, int32_t* out_counts, void* stream) {
    if (!board_ok(board_size) || capacity < 1 || n < 0 || n > REF_MAX_N || new_stamp < 0)
        return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    if (!policy || !stamp || !slot || !p || !idx || !out_counts || !scratch_ok(scratch) ||
        scratch_bytes < rvz_replay_refresh_scratch_size(n))
        return RVZ_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const RefreshLayout l(n, scratch);
    const uint32_t mask = (uint32_t)(l.T - 1);
    const Geometry c = strided(2 * l.T, 256, 256);
    hipLaunchKernelGGL(k_ref_clear, c.grid, c.block, 0, s, l.key, 2 * l.T, out_counts);
    const Geometry g = wave_per_row(n, REF_WPB);
    launch_bs_unchecked(board_size, k_ref_rows<65>, k_ref_rows<37>, g.grid, g.block, s, capacity, n,
                        slot, p, idx, l.ok, l.key, l.val, mask, out_counts);
    launch_bs_unchecked(board_size, k_ref_write<65>, k_ref_write<37>, g.grid, g.block, s, n, slot,
                        p, new_stamp, (const uint32_t*)l.ok, (const uint32_t*)l.key,
                        (const uint32_t*)l.val, mask, policy, stamp, out_counts);
    return last_launch();
}
