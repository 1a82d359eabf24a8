// rvz_replay.hip — a training minibatch drawn from a compact ring of records (rvz_replay_batch;
// contract in include/rvz.h).
//
// The ring holds a record as (mover bitboard, opponent bitboard, policy row, value): 280 B on 8x8
// against the 1028 B of its expanded planes and policy. k_replay_batch: one wavefront per output
// row, lane = output square. The wave draws its record and symmetry from one Philox4x32-10 block
// keyed by (seed, step, row), so the draw is wave-uniform and a pure function of those three;
// then it is k_training_rows' wave (rvz_symmetry.hip.h): three ballots give the image bitboards,
// one cross-lane read moves the policy, the planes go out as float4 and the policy as dwords,
// every output byte once. Nothing is recomputed and no table lives in memory.
//
// The draw of the logical row: i = mulhi(x.0, live), the multiply-high of a uniform 32-bit word.
// Of the 2^32 words, floor(2^32 / live) or one more map to each i, so a row's probability is
// within 2^-32 of 1 / live: a relative bias of at most live / 2^32 (0.05% at 2^21 rows).
//
// The weighted draw (rvz_replay_cdf, rvz_replay_batch_weighted): a per-slot float32 weight becomes
// the fixed-point integer q = rint(w * 2^16), and a table holds the inclusive prefix sums C of q
// over the live rows in logical order. k_cdf_scan / k_cdf_add build it as a tiled scan in
// consecutive launches on one stream (a tile's local scan and its total, the totals scanned the
// same way, the offsets added back), so no workgroup ever waits on another; every sum is an
// integer, so the table's bytes depend on neither the tile nor the order of the adds.
// rvz_replay_batch_weighted is k_replay_batch with another draw: t = mulhi64(u, total) of a
// uniform 64-bit word u, and the row is the first i with C[i] > t, found 64 pivots at a time (a
// load per lane and one ballot per round, 4 rounds at 2^21 rows).
//
// rvz_replay_ownership: a drawn batch's final-ownership targets from two more bitboards a slot, a
// second small kernel on the draw's own out_slot / out_sym (k_replay_ownership).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rvz.h"
#include "rvz_host.hip.h"
#include "rvz_philox.hip.h"
#include "rvz_rules.hip.h"
#include "rvz_symmetry.hip.h"
#include "rvz_wave.hip.h"

namespace {

using namespace rvz;

// ---------------------------------------------------------------- the weighted draw's table
constexpr int CDF_THREADS = 256;                 // 4 waves a tile
constexpr int CDF_WAVES = CDF_THREADS / 64;
constexpr int CDF_HEAD = 4;                      // total, invalid weights, start, live
constexpr int CDF_TILE_LOG2 = 11;                // the default tile: 2,048 rows a workgroup
constexpr int CDF_MAX_LEVELS = 8;                // 2^31 rows at the 64-row tile need 6
constexpr int CDF_ADD_MAX_BLOCKS = 1 << 16;      // grid-stride beyond that

inline bool tile_ok(int t) { return t == 0 || (t >= 6 && t <= 12); }

// The table of n rows at tile 2^tile_log2 (0: the default): the four header words, then the scan's
// levels, cnt[0] = n, cnt[k + 1] = ceil(cnt[k] / tile), down to cnt[L] == 1 (L >= 1). Level 0 is C
// (tot[0]; it has no counts); level k >= 1 is the totals tot[k] and the invalid counts inv[k] of
// level k - 1's tiles, cnt[k] words each.
struct CdfLayout {
    int L = 0, tl;
    int64_t cnt[CDF_MAX_LEVELS + 1], bytes;
    uint64_t *head, *tot[CDF_MAX_LEVELS + 1], *inv[CDF_MAX_LEVELS + 1];
    CdfLayout(int64_t n, int tile_log2, void* cdf) : tl(tile_log2 ? tile_log2 : CDF_TILE_LOG2) {
        Carver c(cdf);
        head = c.packed<uint64_t>(CDF_HEAD);
        cnt[0] = n;
        tot[0] = c.packed<uint64_t>(n);
        do {
            cnt[L + 1] = (cnt[L] + ((int64_t)1 << tl) - 1) >> tl;
            ++L;
            tot[L] = c.packed<uint64_t>(cnt[L]);
            inv[L] = c.packed<uint64_t>(cnt[L]);
        } while (cnt[L] > 1);
        bytes = up16(c.at);
    }
};

// One tile of one level: the local inclusive scan of the tile's items into vals, the tile's total
// into tot_out[tile] and its invalid weights into inv_out[tile]. LEAF: item i is q of the weight
// of logical row i (slot (start + i) % capacity) and vals is C; else item i is vals[i] (the totals
// of the level below, scanned in place) and its invalid count is inv_in[i]. A chunk of blockDim.x
// items per step of the workgroup scan (rvz_wave.hip.h; two LDS buffers, so one barrier a chunk).
template <bool LEAF>
__global__ __launch_bounds__(CDF_THREADS) void k_cdf_scan(
    const float* __restrict__ weight, int capacity, int start, uint64_t* vals,
    const uint64_t* __restrict__ inv_in, int64_t n, int tile, uint64_t* __restrict__ tot_out,
    uint64_t* __restrict__ inv_out) {
    __shared__ uint64_t part[2][CDF_WAVES];
    __shared__ uint64_t bad[CDF_WAVES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int waves = blockDim.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * tile;
    const int64_t end = base + tile < n ? base + tile : n;
    uint64_t carry = 0ull, nbad = 0ull;
    int c = 0;
    for (int64_t at = base; at < end; at += blockDim.x, c ^= 1) {      // block-uniform trip count
        const int64_t i = at + threadIdx.x;
        uint64_t v = 0ull;
        if (i < end) {
            if (LEAF) {
                const int64_t s = (int64_t)start + i;                   // below 2 * capacity
                const float w = weight[s >= capacity ? s - capacity : s];
                const bool valid = w >= 0.0f && w <= 65536.0f;          // NaN fails both
                v = valid ? (uint64_t)rint((double)w * 65536.0) : 0ull;
                nbad += valid ? 0ull : 1ull;
            } else {
                v = vals[i];
                nbad += inv_in[i];
            }
        }
        v = block_scan(v, lane, wave, waves, part[c], carry);
        if (i < end) vals[i] = v;
    }
    nbad = block_reduce<1>(&nbad, lane, wave, waves, bad, Sum());
    if (threadIdx.x == 0) {
        tot_out[blockIdx.x] = carry;
        inv_out[blockIdx.x] = nbad;
    }
}

// The offsets added back: vals[i] += prefix[i / tile - 1] for every item past the first tile
// (prefix: the scanned totals of the level above). head (the level of C only): the table's four
// header words, from the top level's one total and one count.
__global__ __launch_bounds__(CDF_THREADS) void k_cdf_add(
    uint64_t* __restrict__ vals, int64_t n, int tile_log2, const uint64_t* __restrict__ prefix,
    uint64_t* __restrict__ head, const uint64_t* __restrict__ top_tot,
    const uint64_t* __restrict__ top_inv, int start, int live) {
    const int64_t stride = (int64_t)gridDim.x * CDF_THREADS;
    for (int64_t i = ((int64_t)1 << tile_log2) + (int64_t)blockIdx.x * CDF_THREADS + threadIdx.x;
         i < n; i += stride)
        vals[i] += prefix[(i >> tile_log2) - 1];
    if (head && blockIdx.x == 0 && threadIdx.x == 0) {
        head[0] = *top_tot;
        head[1] = *top_inv;
        head[2] = (uint64_t)start;
        head[3] = (uint64_t)live;
    }
}

// ---------------------------------------------------------------- the draws and the batch kernel
// A draw is k_replay_batch's compile-time parameter, built once per wave from its Args (the host's
// part). `fresh`: it was built for this ring state (else every row is a zero row); row(): output
// row r's logical row from r's Philox block, by the whole wave (-1: none); prob(): lane 0's store.

// i = mulhi(x.0, live)
struct UniformDraw {
    struct Args {};
    static constexpr bool fresh = true;
    __device__ UniformDraw(Args, int, int) {}
    __device__ int row(int, int, const uint4& x, int live) const {
        return (int)__umulhi(x.x, (uint32_t)live);
    }
    __device__ void prob(int, int, bool) const {}
};

// The first i with C[i] > t, t = mulhi64(u, total). The search keeps [lo, hi] with C[hi] > t and
// C[lo - 1] <= t: each round lane j reads pivot lo + (j + 1) * step - 1 (step = ceil(size / 64),
// clamped to hi, which is known to be above t), and the first lane whose pivot is above t names
// the next range. Its trip count depends on live alone.
struct WeightedDraw {
    struct Args { const uint64_t *cdf, *word; float* out_prob; };      // word, out_prob: or null
    const uint64_t *__restrict__ C, *__restrict__ word;
    float* __restrict__ out_prob;
    uint64_t total;
    bool fresh;
    __device__ WeightedDraw(Args a, int start, int live)
        : C(a.cdf + CDF_HEAD), word(a.word), out_prob(a.out_prob), total(a.cdf[0]),
          fresh(a.cdf[2] == (uint64_t)start && a.cdf[3] == (uint64_t)live) {}
    __device__ int row(int lane, int r, const uint4& x, int live) const {
        if (!(fresh && total)) return -1;                               // wave-uniform
        const uint64_t u = word ? word[r] : (((uint64_t)x.z << 32) | x.w);
        const uint64_t t = __umul64hi(u, total);                        // < total = C[live - 1]
        int64_t lo = 0, hi = live - 1;
        while (hi - lo >= 64) {
            const int64_t step = (hi - lo + 64) >> 6;                   // ceil((hi - lo + 1) / 64)
            const int64_t mine = lo + (int64_t)(lane + 1) * step - 1;
            const bool above = mine >= hi || C[mine] > t;
            const int f = __ffsll((unsigned long long)__ballot(above)) - 1;     // lane 63 is
            const int64_t top = lo + (int64_t)(f + 1) * step - 1;
            lo += (int64_t)f * step;
            hi = top < hi ? top : hi;
        }
        const bool above = lo + lane >= hi || C[lo + lane] > t;
        return (int)(lo + __ffsll((unsigned long long)__ballot(above)) - 1);
    }
    __device__ void prob(int r, int i, bool in) const {
        if (!out_prob) return;
        float p = 0.0f;
        if (in && total) {
            const uint64_t q = C[i] - (i ? C[i - 1] : 0ull);
            p = (float)((double)q / (double)total);
        }
        out_prob[r] = p;
    }
};

// One wavefront per output row: the logical row (given or drawn), its slot, the record, its image
// (write_record) and lane 0's per-row words. A row that is not `ok` is written too, as zeros.
template <int BS, class Draw>
__global__ __launch_bounds__(SYM_THREADS) void k_replay_batch(
    int capacity, const uint64_t* __restrict__ mover, const uint64_t* __restrict__ opponent,
    const float* __restrict__ policy, const float* __restrict__ value, int start, int live, int nb,
    const int32_t* __restrict__ idx, const int32_t* __restrict__ sym,
    const typename Draw::Args draw_args, int random_sym, uint32_t key0, uint32_t key1,
    uint32_t step0, uint32_t step1, float* __restrict__ out_states,
    float* __restrict__ out_policy, float* __restrict__ out_value, int32_t* __restrict__ out_slot,
    int32_t* __restrict__ out_sym) {
    constexpr int NPOL = Geo<BS>::NPOL;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int stride = gridDim.x * SYM_WAVES;       // nb * NPOL fits int32, so r + stride does too
    const Draw draw(draw_args, start, live);
    for (int r = blockIdx.x * SYM_WAVES + wave; r < nb; r += stride) {  // wave-uniform trip count
        const uint4 x = philox4x32_10(key0, key1, (uint32_t)r, step0, step1, 0u);
        const int k = sym ? sym[r] : (random_sym ? (int)(x.y & 7u) : 0);
        const int i = idx ? idx[r] : draw.row(lane, r, x, live);        // idx: wave-uniform
        const bool in = draw.fresh && i >= 0 && i < live;
        const int64_t at = (int64_t)start + (in ? i : 0);              // below 2 * capacity
        const int slot = (int)(at >= capacity ? at - capacity : at);
        const bool ok = in && k >= 0 && k < 8;
        uint64_t P = 0ull, O = 0ull;
        float v = 0.0f;
        if (ok) {                                                       // wave-uniform
            P = mover[slot];
            O = opponent[slot];
            v = value[slot];
        }
        write_record<BS, 1>(lane, P, O, policy + (size_t)slot * NPOL, ok, ok ? k : -1, (size_t)r,
                            out_states, out_policy, nullptr);           // capacity * NPOL: 64-bit
        if (lane == 0) {
            out_value[r] = v;
            out_slot[r] = in ? slot : -1;
            out_sym[r] = ok ? k : -1;
            draw.prob(r, i, in);
        }
    }
}

// What the two entry points share. RVZ_EINVAL: a bad ring or nb (at nb == 0 too), or at nb > 0 a
// missing pointer (draw_ok: the draw's own) or out_states off 16 bytes; RVZ_OK at nb == 0; else
// the one launch.
template <class Draw>
int batch(int bs, int capacity, const uint64_t* mover, const uint64_t* opponent,
          const float* policy, const float* value, int start, int live, int nb, const int32_t* idx,
          const int32_t* sym, typename Draw::Args draw, bool draw_ok, int random_sym, uint64_t seed,
          uint64_t step, float* out_states, float* out_policy, float* out_value, int32_t* out_slot,
          int32_t* out_sym, void* stream) {
    if (!board_ok(bs) || capacity < 1 || live < 1 || live > capacity || start < 0 ||
        start >= capacity || nb < 0)
        return RVZ_EINVAL;
    if ((int64_t)nb * (bs * bs + 1) > INT32_MAX) return RVZ_EINVAL;
    if (nb > 0 && (!mover || !opponent || !policy || !value || !out_states || !out_policy ||
                   !out_value || !out_slot || !out_sym || !draw_ok ||
                   ((uintptr_t)out_states & 15u) != 0))                 // float4 stores
        return RVZ_EINVAL;
    if (nb == 0) return RVZ_OK;
    const Geometry g = strided(nb, SYM_WAVES, SYM_THREADS);
    return launch_bs(bs, k_replay_batch<8, Draw>, k_replay_batch<6, Draw>, g.grid, g.block,
                     (hipStream_t)stream, capacity, mover, opponent, policy, value, start, live, nb,
                     idx, sym, draw, random_sym, (uint32_t)seed, (uint32_t)(seed >> 32),
                     (uint32_t)step, (uint32_t)(step >> 32), out_states, out_policy, out_value,
                     out_slot, out_sym);
}

// The ownership target of a drawn row (rvz_replay_ownership): one wavefront per output row, lane =
// output square. The slot and the symmetry are those k_replay_batch reported for the row, so the
// source square is the one its state planes were read from (sym_src).
template <int BS>
__global__ __launch_bounds__(SYM_THREADS) void k_replay_ownership(
    int capacity, const uint64_t* __restrict__ final_mover,
    const uint64_t* __restrict__ final_opponent, int nb, const int32_t* __restrict__ slot,
    const int32_t* __restrict__ sym, float* __restrict__ out_own, float* __restrict__ out_margin) {
    constexpr int NSQ = Geo<BS>::NSQ;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int stride = gridDim.x * SYM_WAVES;       // nb * NPOL fits int32, so r + stride does too
    for (int r = blockIdx.x * SYM_WAVES + wave; r < nb; r += stride) {  // wave-uniform trip count
        const int s = slot[r], k = sym[r];
        uint64_t P = 0ull, O = 0ull;
        if (s >= 0 && s < capacity && k >= 0 && k < 8) {                // wave-uniform
            P = final_mover[s];
            O = final_opponent[s];
            if ((P & O) || ((P | O) & ~Geo<BS>::FULL)) P = O = 0ull;
        }
        if (lane < NSQ) {
            const int from = sym_src<BS>(lane, k & 7);
            out_own[(size_t)r * NSQ + lane] =
                (float)((int)((P >> from) & 1ull) - (int)((O >> from) & 1ull));
        }
        if (lane == 0) out_margin[r] = (float)((int)__popcll(P) - (int)__popcll(O));
    }
}

}  // namespace

extern "C" int rvz_replay_ownership(int32_t bs, int32_t capacity, const uint64_t* final_mover,
                                    const uint64_t* final_opponent, int32_t nb,
                                    const int32_t* slot, const int32_t* sym, float* out_own,
                                    float* out_margin, void* stream) {
    if (!board_ok(bs) || capacity < 1 || nb < 0) return RVZ_EINVAL;
    if ((int64_t)nb * (bs * bs + 1) > INT32_MAX) return RVZ_EINVAL;
    if (nb > 0 && (!final_mover || !final_opponent || !slot || !sym || !out_own || !out_margin))
        return RVZ_EINVAL;
    if (nb == 0) return RVZ_OK;
    const Geometry g = strided(nb, SYM_WAVES, SYM_THREADS);
    return launch_bs(bs, k_replay_ownership<8>, k_replay_ownership<6>, g.grid, g.block,
                     (hipStream_t)stream, capacity, final_mover, final_opponent, nb, slot, sym,
                     out_own, out_margin);
}

extern "C" int rvz_replay_batch(int32_t bs, int32_t capacity, const uint64_t* mover,
                                const uint64_t* opponent, const float* policy, const float* value,
                                int32_t start, int32_t live, int32_t nb, const int32_t* idx,
                                const int32_t* sym, int32_t random_sym, uint64_t seed,
                                uint64_t step, float* out_states, float* out_policy,
                                float* out_value, int32_t* out_slot, int32_t* out_sym,
                                void* stream) {
    return batch<UniformDraw>(bs, capacity, mover, opponent, policy, value, start, live, nb, idx,
                              sym, {}, true, random_sym, seed, step, out_states, out_policy,
                              out_value, out_slot, out_sym, stream);
}

extern "C" int64_t rvz_replay_cdf_size(int32_t capacity, int32_t tile_log2) {
    if (capacity < 1 || !tile_ok(tile_log2)) return -1;
    return CdfLayout(capacity, tile_log2, nullptr).bytes;
}

extern "C" int rvz_replay_cdf(int32_t capacity, const float* weight, int32_t start, int32_t live,
                              int32_t tile_log2, void* cdf, void* stream) {
    if (capacity < 1 || live < 0 || live > capacity || start < 0 || start >= capacity ||
        !tile_ok(tile_log2))
        return RVZ_EINVAL;
    if (live == 0) return RVZ_OK;
    if (!weight || !scratch_ok(cdf)) return RVZ_EINVAL;
    const CdfLayout l(live, tile_log2, cdf);                            // of the live rows alone
    const int tl = l.tl, L = l.L;
    const int tile = 1 << tl;
    const int threads = tile < CDF_THREADS ? tile : CDF_THREADS;
    hipStream_t s = (hipStream_t)stream;
    const int64_t* cnt = l.cnt;
    uint64_t *head = l.head, *const *tot = l.tot, *const *inv = l.inv;
    hipLaunchKernelGGL(k_cdf_scan<true>, dim3((unsigned)cnt[1]), dim3(threads), 0, s, weight,
                       capacity, start, tot[0], (const uint64_t*)nullptr, cnt[0], tile, tot[1],
                       inv[1]);
    for (int k = 1; k < L; ++k)
        hipLaunchKernelGGL(k_cdf_scan<false>, dim3((unsigned)cnt[k + 1]), dim3(threads), 0, s,
                           (const float*)nullptr, 0, 0, tot[k], (const uint64_t*)inv[k], cnt[k],
                           tile, tot[k + 1], inv[k + 1]);
    for (int k = L - 2; k >= 0; --k) {                                  // tot[L - 1] is complete
        const int64_t rest = cnt[k] - tile;                             // the items past tile 0
        int64_t blocks = rest > 0 ? (rest + CDF_THREADS - 1) / CDF_THREADS : 1;
        if (blocks > CDF_ADD_MAX_BLOCKS) blocks = CDF_ADD_MAX_BLOCKS;
        hipLaunchKernelGGL(k_cdf_add, dim3((unsigned)blocks), dim3(CDF_THREADS), 0, s, tot[k],
                           cnt[k], tl, (const uint64_t*)tot[k + 1], k ? nullptr : head,
                           (const uint64_t*)tot[L], (const uint64_t*)inv[L], start, live);
    }
    if (L == 1)                                                         // one tile: the header
        hipLaunchKernelGGL(k_cdf_add, dim3(1), dim3(CDF_THREADS), 0, s, tot[0], cnt[0], tl,
                           (const uint64_t*)tot[1], head, (const uint64_t*)tot[1],
                           (const uint64_t*)inv[1], start, live);
    return last_launch();
}

extern "C" int rvz_replay_batch_weighted(int32_t bs, int32_t capacity, const uint64_t* mover,
                                         const uint64_t* opponent, const float* policy,
                                         const float* value, const void* cdf, int32_t start,
                                         int32_t live, int32_t nb, const int32_t* idx,
                                         const int32_t* sym, const uint64_t* word,
                                         int32_t random_sym, uint64_t seed, uint64_t step,
                                         float* out_states, float* out_policy, float* out_value,
                                         int32_t* out_slot, int32_t* out_sym, float* out_prob,
                                         void* stream) {
    return batch<WeightedDraw>(bs, capacity, mover, opponent, policy, value, start, live, nb, idx,
                               sym, {(const uint64_t*)cdf, word, out_prob}, scratch_ok(cdf),
                               random_sym, seed, step, out_states, out_policy, out_value, out_slot,
                               out_sym, stream);
}
