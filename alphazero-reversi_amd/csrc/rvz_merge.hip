// rvz_merge.hip — one training row per distinct position (rvz_merge_positions; contract in
// include/rvz.h): rows with equal (mover, opponent) bitboards become one row, in order of first
// occurrence, whose policy and value are the means of the members'.
//
// Every sum is an integer sum of q(x) = rint(x * 2^36) in int64, so no result depends on the order
// in which the hardware performs the adds; the mean is one float64 division per entry. A group of
// one member copies its row, bits untouched.
//
// Nine small launches on the caller's stream, no host step between them:
//   k_init       table = -1, first = INT_MAX, count = 0
//   k_validate   one wavefront per row, lane = policy entry: the malformed-row rules
//   k_insert     one lane per row: open addressing on an int32 table of row indices. A row
//                claims an empty slot with a CAS or meets the row s that holds it and compares
//                keys, read from the immutable inputs. The slot's holder is the group's
//                provisional representative (which member wins the slot is timing); the group's
//                identity is made timing-free by atomicMin(first[rep], row): its lowest row.
//   k_count / k_scan_blocks / k_assign   a three-kernel exclusive scan over two flags per row
//                (the row is its group's first; and the group has two or more members), giving
//                each group its dense output row and each multi-member group a slot of sums
//   k_zero       the sums of the slots in use
//   k_accumulate one wavefront per row: a singleton copies; any other row adds its q's, lane =
//                entry, 8-byte integer atomics on contiguous addresses. A workgroup owns
//                ACC_ROWS consecutive rows and first sums the rows of large groups (HOT_MIN
//                members or more) in LDS, HOT_SLOTS groups at a time, so such a group takes one
//                global add per workgroup and entry instead of one per member
//   k_divide     one wavefront per multi-member group: the means
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/rvz.h"
#include "rvz_host.hip.h"
#include "rvz_wave.hip.h"

namespace {

using namespace rvz;

constexpr int MG_THREADS = 256;
constexpr int MG_WAVES = MG_THREADS / 64;
constexpr int MG_MAX_BLOCKS = 4096;              // grid-stride beyond that
constexpr int SCAN_ITEMS = 4;                    // consecutive rows per lane in the scan kernels
constexpr int SCAN_ROWS = MG_THREADS * SCAN_ITEMS;
constexpr int SCAN_TOP = 1024;                   // threads of the one block that scans the block sums
constexpr int ACC_ROWS = 2048;                   // consecutive rows per workgroup in k_accumulate
constexpr int HOT_SLOTS = 8;                     // groups a workgroup pre-reduces in LDS at a time
constexpr int HOT_MIN = 64;                      // members from which a group is pre-reduced
constexpr double Q_SCALE = 68719476736.0;        // 2^36
constexpr int PENDING = -2;                      // prov[]: a well-formed row not yet inserted

typedef unsigned long long u64;

struct Layout {                                  // the scratch's parts
    int32_t *hdr, *table, *prov, *first, *cnt, *gidx, *sslot, *mlist;
    u64 *bsum, *sums;
    int64_t total = -1;                          // -1: bad arguments
    int32_t slots, nblk;
    Layout(int32_t bs, int32_t n, int32_t table_log2, void* scratch) {
        const int64_t np = (int64_t)bs * bs + 1;
        if (!board_ok(bs) || n < 0 || (int64_t)n * np > INT32_MAX) return;
        int lg = table_log2;
        if (lg == 0) {
            while (((int64_t)1 << lg) < 2 * (int64_t)n) ++lg;
        } else if (lg < 0 || lg > 30 || ((int64_t)1 << lg) <= n) {
            return;
        }
        slots = (int32_t)1 << lg;
        nblk = (n + SCAN_ROWS - 1) / SCAN_ROWS;
        Carver c(scratch);
        hdr = c.take<int32_t>(16);
        table = c.take<int32_t>(slots);
        prov = c.take<int32_t>(n);
        first = c.take<int32_t>(n);
        cnt = c.take<int32_t>(n);
        gidx = c.take<int32_t>(n);
        sslot = c.take<int32_t>(n);
        mlist = c.take<int32_t>(n / 2 + 1);
        bsum = c.take<u64>(nblk + 1);
        sums = c.packed<u64>((np + 1) * (int64_t)(n / 2));   // groups of two or more: at most n/2
        total = c.at;
    }
};

template <int BS>
struct MG {
    static constexpr int NSQ = BS * BS, NPOL = NSQ + 1, NE = NPOL + 1;   // NE: policy, then value
};

__device__ __forceinline__ void row_key(const uint64_t* __restrict__ black,
                                        const uint64_t* __restrict__ white,
                                        const int32_t* __restrict__ status, int i, uint64_t& P,
                                        uint64_t& O) {
    const uint64_t b = black[i], w = white[i];
    const bool first = status[4 * (size_t)i] == 1;
    P = first ? b : w;
    O = first ? w : b;
}

__device__ __forceinline__ uint32_t key_hash(uint64_t P, uint64_t O) {
    uint64_t h = (P * 0x9E3779B97F4A7C15ull) ^ (O * 0xC2B2AE3D27D4EB4Full);
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    return (uint32_t)h;
}

__global__ __launch_bounds__(MG_THREADS) void k_init(int n, int slots, int32_t* __restrict__ table,
                                                     int32_t* __restrict__ first,
                                                     int32_t* __restrict__ cnt,
                                                     int32_t* __restrict__ hdr) {
    const long long step = (long long)gridDim.x * MG_THREADS;
    const long long top = slots > n ? slots : n;
    for (long long i = (long long)blockIdx.x * MG_THREADS + threadIdx.x; i < top; i += step) {
        if (i < slots) table[i] = -1;
        if (i < n) {
            first[i] = INT_MAX;
            cnt[i] = 0;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 16) hdr[threadIdx.x] = 0;
}

template <int BS>
__global__ __launch_bounds__(MG_THREADS) void k_validate(
    int n, const uint64_t* __restrict__ black, const uint64_t* __restrict__ white,
    const int32_t* __restrict__ status, const float* __restrict__ policy,
    const float* __restrict__ value, int32_t* __restrict__ prov) {
    constexpr int NSQ = MG<BS>::NSQ, NPOL = MG<BS>::NPOL;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int step = gridDim.x * MG_WAVES;
    for (int i = blockIdx.x * MG_WAVES + wave; i < n; i += step) {      // wave-uniform trip count
        const float* prow = policy + (size_t)i * NPOL;
        bool bad = false;
        for (int e = lane; e < NPOL; e += 64) {
            const float x = prow[e];
            bad |= !(x >= 0.0f && x <= 1.0f);                           // NaN fails both
        }
        if (lane == 63) {                                               // the lane with one entry
            const float v = value[i];
            const uint64_t b = black[i], w = white[i];
            const int side = status[4 * (size_t)i];
            bad |= !(v >= -1.0f && v <= 1.0f) || (b & w) != 0 || (side != 1 && side != 2);
            if (NSQ < 64) bad |= ((b | w) >> (NSQ & 63)) != 0;
        }
        const bool any = __ballot(bad) != 0;
        if (lane == 0) prov[i] = any ? -1 : PENDING;
    }
}

__global__ __launch_bounds__(MG_THREADS) void k_insert(
    int n, int slots, const uint64_t* __restrict__ black, const uint64_t* __restrict__ white,
    const int32_t* __restrict__ status, int32_t* table, int32_t* prov, int32_t* first,
    int32_t* cnt) {
    const uint32_t mask = (uint32_t)slots - 1u;
    const long long step = (long long)gridDim.x * MG_THREADS;
    for (long long ii = (long long)blockIdx.x * MG_THREADS + threadIdx.x; ii < n; ii += step) {
        const int i = (int)ii;
        if (prov[i] != PENDING) continue;
        uint64_t P, O;
        row_key(black, white, status, i, P, O);
        uint32_t slot = key_hash(P, O) & mask;
        int rep = -1;
        // at most n < slots slots are ever claimed, so an empty one always ends the walk; the
        // bound only keeps the loop finite whatever happens
        for (int probes = 0; probes < slots; ++probes) {
            // a slot is written once: a stale read can only show -1, and then the CAS decides
            int s = __hip_atomic_load(&table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (s == -1) {
                s = atomicCAS(&table[slot], -1, i);
                if (s == -1) s = i;
            }
            if (s == i) {
                rep = i;
                break;
            }
            uint64_t SP, SO;
            row_key(black, white, status, s, SP, SO);
            if (SP == P && SO == O) {
                rep = s;
                break;
            }
            slot = (slot + 1u) & mask;
        }
        prov[i] = rep;
        if (rep >= 0) {
            atomicMin(&first[rep], i);
            atomicAdd(&cnt[rep], 1);
        }
    }
}

// bit 0: row i is the first of its group; bit 32: and the group has two or more members
__device__ __forceinline__ u64 row_flags(int i, const int32_t* __restrict__ prov,
                                         const int32_t* __restrict__ first,
                                         const int32_t* __restrict__ cnt) {
    const int r = prov[i];
    if (r < 0 || first[r] != i) return 0ull;
    return cnt[r] >= 2 ? (1ull << 32) | 1ull : 1ull;
}

// the exclusive scan of v over the block's NW waves and its total (both 32-bit halves at once:
// neither carries, every total is at most 2^25): one step of the workgroup scan; lds: NW words
template <int NW>
__device__ __forceinline__ u64 block_exclusive_scan(u64 v, u64* lds, u64& total) {
    total = 0ull;
    return block_scan(v, threadIdx.x & 63, threadIdx.x >> 6, NW, lds, total) - v;
}

__global__ __launch_bounds__(MG_THREADS) void k_count(int n, const int32_t* __restrict__ prov,
                                                      const int32_t* __restrict__ first,
                                                      const int32_t* __restrict__ cnt,
                                                      u64* __restrict__ bsum) {
    __shared__ u64 lds[MG_WAVES];
    const long long base = (long long)blockIdx.x * SCAN_ROWS + (long long)threadIdx.x * SCAN_ITEMS;
    u64 v = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (base + k < n) v += row_flags((int)(base + k), prov, first, cnt);
    u64 total;
    block_exclusive_scan<MG_WAVES>(v, lds, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one block: bsum[0 .. nblk) becomes its own exclusive scan; the totals are m and the number of
// multi-member groups
__global__ __launch_bounds__(SCAN_TOP) void k_scan_blocks(int nblk, u64* bsum,
                                                          int32_t* __restrict__ hdr,
                                                          int32_t* __restrict__ out_m) {
    __shared__ u64 lds[SCAN_TOP / 64];
    const int per = (nblk + SCAN_TOP - 1) / SCAN_TOP;
    const int lo = threadIdx.x * per;
    const int hi = lo + per < nblk ? lo + per : nblk;
    u64 v = 0;
    for (int b = lo; b < hi; ++b) v += bsum[b];
    u64 total;
    u64 run = block_exclusive_scan<SCAN_TOP / 64>(v, lds, total);
    for (int b = lo; b < hi; ++b) {
        const u64 x = bsum[b];
        bsum[b] = run;
        run += x;
    }
    if (threadIdx.x == 0) {
        hdr[0] = (int32_t)(total & 0xFFFFFFFFull);
        hdr[1] = (int32_t)(total >> 32);
        out_m[0] = (int32_t)(total & 0xFFFFFFFFull);
    }
}

__global__ __launch_bounds__(MG_THREADS) void k_assign(
    int n, const int32_t* __restrict__ prov, const int32_t* __restrict__ first,
    const int32_t* __restrict__ cnt, const u64* __restrict__ bsum, int32_t* __restrict__ gidx,
    int32_t* __restrict__ sslot, int32_t* __restrict__ mlist, int32_t* __restrict__ out_first,
    int32_t* __restrict__ out_count) {
    __shared__ u64 lds[MG_WAVES];
    const long long base = (long long)blockIdx.x * SCAN_ROWS + (long long)threadIdx.x * SCAN_ITEMS;
    u64 f[SCAN_ITEMS];
    u64 v = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        f[k] = base + k < n ? row_flags((int)(base + k), prov, first, cnt) : 0ull;
        v += f[k];
    }
    u64 total;
    u64 run = bsum[blockIdx.x] + block_exclusive_scan<MG_WAVES>(v, lds, total);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (f[k]) {
            const int i = (int)(base + k);
            const int r = prov[i];
            const int j = (int)(run & 0xFFFFFFFFull);       // < m <= n
            const int c = cnt[r];
            out_first[j] = i;
            out_count[j] = c;
            gidx[r] = j;
            if (f[k] >> 32) {
                const int s = (int)(run >> 32);             // < groups of two or more <= n / 2
                sslot[r] = s;
                mlist[s] = j;
            }
            run += f[k];
        }
    }
}

__global__ __launch_bounds__(MG_THREADS) void k_zero(const int32_t* __restrict__ hdr, int ne,
                                                     u64* __restrict__ sums) {
    const long long top = (long long)hdr[1] * ne;
    const long long step = (long long)gridDim.x * MG_THREADS;
    for (long long i = (long long)blockIdx.x * MG_THREADS + threadIdx.x; i < top; i += step)
        sums[i] = 0ull;
}

__device__ __forceinline__ u64 quantum(float x) {
    return (u64)__double2ll_rn((double)x * Q_SCALE);        // the product is exact
}

template <int BS>
__global__ __launch_bounds__(MG_THREADS) void k_accumulate(
    int n, int hot, const float* __restrict__ policy, const float* __restrict__ value,
    const int32_t* __restrict__ prov, const int32_t* __restrict__ gidx,
    const int32_t* __restrict__ sslot, const int32_t* __restrict__ cnt, u64* sums,
    float* __restrict__ out_policy, float* __restrict__ out_value,
    int32_t* __restrict__ out_group) {
    constexpr int NPOL = MG<BS>::NPOL, NE = MG<BS>::NE;
    __shared__ int hot_rep[HOT_SLOTS];
    __shared__ u64 acc[HOT_SLOTS][NE];
    for (int t = threadIdx.x; t < HOT_SLOTS * NE; t += MG_THREADS) (&acc[0][0])[t] = 0ull;
    if (threadIdx.x < HOT_SLOTS) hot_rep[threadIdx.x] = -1;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long row0 = (long long)blockIdx.x * ACC_ROWS;
    const int row1 = (int)(row0 + ACC_ROWS < n ? row0 + ACC_ROWS : n);
    for (int i = (int)row0 + wave; i < row1; i += MG_WAVES) {           // wave-uniform
        const int r = prov[i];
        if (r < 0) {
            if (lane == 0) out_group[i] = -1;
            continue;
        }
        const int j = gidx[r], c = cnt[r];
        const float* prow = policy + (size_t)i * NPOL;
        if (lane == 0) out_group[i] = j;
        if (c == 1) {                                                   // moved, never recomputed
            float* orow = out_policy + (size_t)j * NPOL;
            for (int e = lane; e < NPOL; e += 64) orow[e] = prow[e];
            if (lane == 0) out_value[j] = value[i];
            continue;
        }
        int h = -1;
        if (hot && c >= HOT_MIN) {
            if (lane == 0) {
                const int at = (int)(((uint32_t)r * 2654435761u) >> 16);
                for (int t = 0; t < HOT_SLOTS; ++t) {
                    const int s = (at + t) & (HOT_SLOTS - 1);
                    const int old = atomicCAS(&hot_rep[s], -1, r);
                    if (old == -1 || old == r) {
                        h = s;
                        break;
                    }
                }
            }
            h = __shfl(h, 0, 64);
        }
        u64* dst = sums + (size_t)sslot[r] * NE;
        for (int e = lane; e < NE; e += 64) {
            const u64 q = quantum(e < NPOL ? prow[e] : value[i]);
            if (h >= 0) atomicAdd(&acc[h][e], q);
            else atomicAdd(&dst[e], q);
        }
    }
    __syncthreads();
    for (int h = 0; h < HOT_SLOTS; ++h) {
        const int r = hot_rep[h];
        if (r < 0) continue;                                            // block-uniform
        u64* dst = sums + (size_t)sslot[r] * NE;
        for (int e = threadIdx.x; e < NE; e += MG_THREADS) atomicAdd(&dst[e], acc[h][e]);
    }
}

template <int BS>
__global__ __launch_bounds__(MG_THREADS) void k_divide(
    const int32_t* __restrict__ hdr, const int32_t* __restrict__ mlist,
    const int32_t* __restrict__ out_count, const u64* __restrict__ sums,
    float* __restrict__ out_policy, float* __restrict__ out_value) {
    constexpr int NPOL = MG<BS>::NPOL, NE = MG<BS>::NE;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int groups = hdr[1];
    const int step = gridDim.x * MG_WAVES;
    for (int k = blockIdx.x * MG_WAVES + wave; k < groups; k += step) {
        const int j = mlist[k];
        const double den = (double)out_count[j] * Q_SCALE;
        const u64* src = sums + (size_t)k * NE;
        for (int e = lane; e < NE; e += 64) {
            const float mean = (float)((double)(long long)src[e] / den);
            if (e < NPOL) out_policy[(size_t)j * NPOL + e] = mean;
            else out_value[j] = mean;
        }
    }
}

int blocks_for(int64_t units, int per_block) {
    const int64_t need = (units + per_block - 1) / per_block;
    return (int)(need < MG_MAX_BLOCKS ? (need > 0 ? need : 1) : MG_MAX_BLOCKS);
}

}  // namespace

extern "C" int64_t rvz_merge_scratch_size(int32_t bs, int32_t n, int32_t table_log2) {
    return Layout(bs, n, table_log2, nullptr).total;
}

extern "C" int rvz_merge_positions(int32_t bs, int32_t n, const uint64_t* black,
                                   const uint64_t* white, const int32_t* status,
                                   const float* policy, const float* value, int32_t table_log2,
                                   void* scratch, int32_t* out_m, int32_t* out_first,
                                   int32_t* out_count, float* out_policy, float* out_value,
                                   int32_t* out_group, void* stream) {
    const Layout L(bs, n, table_log2, scratch);
    if (L.total < 0) return RVZ_EINVAL;
    if (n > 0 && (!black || !white || !status || !policy || !value || !scratch_ok(scratch) ||
                  !out_m || !out_first || !out_count || !out_policy || !out_value || !out_group))
        return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    const char* env = getenv("RVZ_MERGE_HOT");                  // "0": no LDS pre-reduction
    const int hot = !(env && env[0] == '0' && env[1] == 0);
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(MG_THREADS);
    const dim3 per_lane(blocks_for(n, MG_THREADS)), per_wave(blocks_for(n, MG_WAVES));
    const int ne = bs * bs + 2;

    hipLaunchKernelGGL(k_init, dim3(blocks_for(L.slots > n ? L.slots : n, MG_THREADS)), block, 0,
                       s, n, L.slots, L.table, L.first, L.cnt, L.hdr);
    launch_bs_unchecked(bs, k_validate<8>, k_validate<6>, per_wave, block, s, n, black, white,
                        status, policy, value, L.prov);
    hipLaunchKernelGGL(k_insert, per_lane, block, 0, s, n, L.slots, black, white, status, L.table,
                       L.prov, L.first, L.cnt);
    hipLaunchKernelGGL(k_count, dim3(L.nblk), block, 0, s, n, L.prov, L.first, L.cnt, L.bsum);
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(SCAN_TOP), 0, s, L.nblk, L.bsum, L.hdr, out_m);
    hipLaunchKernelGGL(k_assign, dim3(L.nblk), block, 0, s, n, L.prov, L.first, L.cnt, L.bsum,
                       L.gidx, L.sslot, L.mlist, out_first, out_count);
    hipLaunchKernelGGL(k_zero, dim3(blocks_for((int64_t)(n / 2) * ne, 4 * MG_THREADS)), block, 0,
                       s, L.hdr, ne, L.sums);
    const dim3 chunks((n + ACC_ROWS - 1) / ACC_ROWS);
    launch_bs_unchecked(bs, k_accumulate<8>, k_accumulate<6>, chunks, block, s, n, hot, policy,
                        value, L.prov, L.gidx, L.sslot, L.cnt, L.sums, out_policy, out_value,
                        out_group);
    // the last of the nine launches: its error return answers for all of them
    return launch_bs(bs, k_divide<8>, k_divide<6>, dim3(blocks_for(n / 2, MG_WAVES)), block, s,
                     L.hdr, L.mlist, out_count, L.sums, out_policy, out_value);
}
