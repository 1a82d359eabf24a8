// rvz_records.hip — a window of autoreset self-play records cut into finished games
// (rvz_records_games; contract in include/rvz.h), and the final position of the game a record
// belongs to (rvz_records_final, the ownership target; its kernels stand before the entry points).
//
// rvz_play with reset = 1 writes one record per ply and slot, a slot's games one after another.
// Three consecutive launches on one stream turn a window [plies][n_games] of such records into the
// compact rows a replay ring holds; no workgroup waits on another, nothing is an atomic, and every
// output element is written once.
//
// k_rec_walk, a lane per slot: the walk of the contract down the slot's column (the [ply][slot]
// layout makes each ply's loads coalesced across the lanes) with the engine's own make_move
// (rvz_rules.hip.h). A record enters the scratch as "open" with its side; when its segment ends or
// is abandoned, the lane goes back over the segment's plies and writes each record's final state,
// its value target and, for an emitted record, its rank among the slot's rows. A record is
// revisited once at most (segments are disjoint), and a lane reads back only words it wrote
// itself. The slot's seven counts go to the scratch, slot-minor.
//
// k_rec_scan, one workgroup: the exclusive scan of the slots' row counts (the chunked workgroup
// scan of rvz_wave.hip.h, as k_cdf_scan) and the seven sums in 64 bits; it writes out_m and
// out_stats.
//
// k_rec_rows, a wavefront per record, lane = policy entry (on 8x8 lane 0 also carries the pass
// entry, as in rvz_policy_value_loss): out_state of every record, and for an emitted one the row
// at offset[slot] + rank: the policy converted to float32, the two bitboards from the mover's
// side, the value, the source index.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rvz.h"
#include "rvz_host.hip.h"
#include "rvz_rules.hip.h"
#include "rvz_wave.hip.h"

namespace {

using namespace rvz;

constexpr int WALK_THREADS = 64;                 // k_rec_walk: one wave a workgroup, a lane a slot
constexpr int SCAN_THREADS = 1024;               // k_rec_scan's one workgroup: 16 waves
constexpr int SCAN_WAVES = SCAN_THREADS / 64;
constexpr int ROWS_WAVES = 4;                    // k_rec_rows: records per workgroup and step
constexpr int ROWS_THREADS = ROWS_WAVES * 64;
constexpr int N_COUNTS = 7;                      // out_stats [0, 7) per slot

// a record's states (out_state)
constexpr int ST_MALFORMED = -5, ST_NONE = -1, ST_OPEN = 0, ST_EMITTED = 1, ST_EARLIER = 2,
              ST_ABANDONED = 3;

// the scratch's word per record: bits 0-7 state + 8, bits 8-9 the side, bits 16-17 value + 1
__device__ __forceinline__ int32_t pack(int state, int side, int value) {
    return (state + 8) | (side << 8) | ((value + 1) << 16);
}
__device__ __forceinline__ int word_state(int32_t w) { return (w & 0xff) - 8; }
__device__ __forceinline__ int word_side(int32_t w) { return (w >> 8) & 3; }
__device__ __forceinline__ int word_value(int32_t w) { return ((w >> 16) & 3) - 1; }

// the scratch: offset [n_games], counts [7][n_games], info [records], rank [records]; each part
// 16-byte aligned
struct Layout {
    int64_t* offset;
    int32_t *counts, *info, *rank;
    int64_t bytes;
    Layout(int64_t plies, int64_t n_games, void* scratch) {
        Carver c(scratch);
        offset = c.take<int64_t>(n_games);
        counts = c.take<int32_t>(N_COUNTS * n_games);
        info = c.take<int32_t>(plies * n_games);
        rank = c.take<int32_t>(plies * n_games);
        bytes = c.at;
    }
};

template <int BS>
__global__ __launch_bounds__(WALK_THREADS) void k_rec_walk(
    int plies, int n_games, const uint64_t* __restrict__ rec_black,
    const uint64_t* __restrict__ rec_white, const int32_t* __restrict__ rec_side,
    const int32_t* __restrict__ rec_idx, int emit_from, int32_t* info, int32_t* __restrict__ rank,
    int32_t* __restrict__ counts) {
    constexpr int NSQ = Geo<BS>::NSQ;
    const int g = blockIdx.x * WALK_THREADS + threadIdx.x;
    if (g >= n_games) return;
    const size_t G = (size_t)n_games;
    int rows = 0, games = 0, abandoned = 0, malformed = 0, headless_games = 0, earlier = 0;
    bool open = false, headless = false;
    int seg_start = 0, seg_len = 0;
    GameS cur = {0ull, 0ull, 1, 0, -1, 0};

    // the segment's records in plies [from, to): every word still open becomes `state`; an
    // emitted record gets its value against `winner` and the slot's next rank
    auto close = [&](int from, int to, int state, int winner) {
        for (int q = from; q < to; ++q) {
            const size_t at = (size_t)q * G + g;
            const int32_t w = info[at];
            if (word_state(w) != ST_OPEN) continue;                     // a ply without a record
            const int side = word_side(w);
            const int value = state != ST_EMITTED || winner == 0 ? 0 : (winner == side ? 1 : -1);
            info[at] = pack(state, side, value);
            if (state == ST_EMITTED) rank[at] = rows++;
        }
    };

    for (int p = 0; p < plies; ++p) {
        const size_t at = (size_t)p * G + g;
        const int idx = rec_idx[at];
        if (idx < 0) {
            info[at] = pack(ST_NONE, 0, 0);
            continue;
        }
        const uint64_t b = rec_black[at], w = rec_white[at];
        const int side = rec_side[at];
        bool ok = !(b & w) && !((b | w) & ~Geo<BS>::FULL) && (side == 1 || side == 2) &&
                  idx <= NSQ;
        const bool chained = open && b == cur.black && w == cur.white && side == cur.side;
        if (ok && open && !chained) {                                   // the chain is broken
            close(seg_start, p, ST_ABANDONED, 0);
            abandoned += seg_len;
            open = false;
        }
        GameS t = cur;
        if (ok) {
            if (!chained) t = GameS{b, w, side, 0, -1, 0};
            ok = make_move<BS>(t, idx == NSQ ? -1 : idx);
        }
        if (!ok) {
            info[at] = pack(ST_MALFORMED, 0, 0);
            ++malformed;
            if (open) {
                close(seg_start, p, ST_ABANDONED, 0);
                abandoned += seg_len;
                open = false;
            }
            continue;
        }
        if (!open) {
            open = true;
            seg_start = p;
            seg_len = 0;
            headless = !(b == Geo<BS>::START_BLACK && w == Geo<BS>::START_WHITE && side == 1);
        }
        info[at] = pack(ST_OPEN, side, 0);
        ++seg_len;
        cur = t;
        if (cur.over) {
            if (p >= emit_from) {
                close(seg_start, p + 1, ST_EMITTED, cur.winner);
                ++games;
                headless_games += headless ? 1 : 0;
            } else {
                close(seg_start, p + 1, ST_EARLIER, 0);
                earlier += seg_len;
            }
            open = false;
        }
    }
    counts[0 * G + g] = rows;
    counts[1 * G + g] = games;
    counts[2 * G + g] = open ? seg_len : 0;
    counts[3 * G + g] = abandoned;
    counts[4 * G + g] = malformed;
    counts[5 * G + g] = headless_games;
    counts[6 * G + g] = earlier;
}

__global__ __launch_bounds__(SCAN_THREADS) void k_rec_scan(int n_games,
                                                           const int32_t* __restrict__ counts,
                                                           int64_t* __restrict__ offset,
                                                           int32_t* __restrict__ out_m,
                                                           int64_t* __restrict__ out_stats) {
    __shared__ int64_t part[2][SCAN_WAVES];
    __shared__ int64_t sums[SCAN_WAVES * N_COUNTS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t G = (size_t)n_games;
    int64_t carry = 0, s[N_COUNTS];
#pragma unroll
    for (int k = 0; k < N_COUNTS; ++k) s[k] = 0;
    int c = 0;
    for (int base = 0; base < n_games; base += SCAN_THREADS, c ^= 1) {  // block-uniform trip count
        const int i = base + (int)threadIdx.x;
        int64_t mine = 0;
        if (i < n_games) {
            mine = counts[i];
#pragma unroll
            for (int k = 0; k < N_COUNTS; ++k) s[k] += counts[k * G + i];
        }
        const int64_t upto = block_scan(mine, lane, wave, SCAN_WAVES, part[c], carry);
        if (i < n_games) offset[i] = upto - mine;
    }
    const int64_t all = block_reduce<N_COUNTS>(s, lane, wave, SCAN_WAVES, sums, Sum());
    if (threadIdx.x < 8) {
        out_stats[threadIdx.x] = all;                                   // thread k: count k; [7] is 0
        if (threadIdx.x == 0) *out_m = (int32_t)all;                    // rows <= records < 2^31
    }
}

template <int BS>
__global__ __launch_bounds__(ROWS_THREADS) void k_rec_rows(
    int records, int n_games, const uint64_t* __restrict__ rec_black,
    const uint64_t* __restrict__ rec_white, const double* __restrict__ rec_p,
    const int32_t* __restrict__ info, const int32_t* __restrict__ rank,
    const int64_t* __restrict__ offset, uint64_t* __restrict__ out_mover,
    uint64_t* __restrict__ out_opponent, float* __restrict__ out_policy,
    float* __restrict__ out_value, int32_t* __restrict__ out_src, int32_t* __restrict__ out_state) {
    constexpr int NPOL = Geo<BS>::NPOL;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int stride = gridDim.x * ROWS_WAVES;      // records * NPOL fits int32, so r + stride does
    for (int r = blockIdx.x * ROWS_WAVES + wave; r < records; r += stride) {    // wave-uniform
        const int32_t w = info[r];
        const int state = word_state(w);
        if (lane == 0 && out_state) out_state[r] = state;
        if (state != ST_EMITTED) continue;
        const size_t j = (size_t)(offset[r % n_games] + rank[r]);       // < *out_m <= records
        const double* __restrict__ src = rec_p + (size_t)r * NPOL;
        float* __restrict__ dst = out_policy + j * NPOL;
        if (lane < NPOL) dst[lane] = (float)src[lane];
        if (NPOL > 64 && lane == 0) dst[64] = (float)src[64];
        if (lane == 0) {
            const uint64_t b = rec_black[r], wh = rec_white[r];
            const bool black_moves = word_side(w) == 1;
            out_mover[j] = black_moves ? b : wh;
            out_opponent[j] = black_moves ? wh : b;
            out_value[j] = (float)word_value(w);
            out_src[j] = r;
        }
    }
}

// rvz_records_final, a lane per row: the walk of the contract from the row's own record down its
// slot's column to the end of its game. The wave's four counts go to out_stats as 64-bit integer
// adds (k_final_clear zeroed them in the launch before), so their sums depend on no order.
constexpr int FINAL_THREADS = 64;                // one wave a workgroup: the ballots below are its own
constexpr int FIN_OK = 1, FIN_OPEN = 2, FIN_OTHER = 3;

__global__ void k_final_clear(int64_t* __restrict__ out_stats) {
    if (threadIdx.x < 4) out_stats[threadIdx.x] = 0;
}

template <int BS>
__global__ __launch_bounds__(FINAL_THREADS) void k_rec_final(
    int plies, int n_games, const uint64_t* __restrict__ rec_black,
    const uint64_t* __restrict__ rec_white, const int32_t* __restrict__ rec_side,
    const int32_t* __restrict__ rec_idx, int n, const int32_t* __restrict__ src,
    const int32_t* __restrict__ count, uint64_t* __restrict__ out_final_mover,
    uint64_t* __restrict__ out_final_opponent, int32_t* __restrict__ out_ok,
    int64_t* __restrict__ out_stats) {
    constexpr int NSQ = Geo<BS>::NSQ;
    const int64_t j = (int64_t)blockIdx.x * FINAL_THREADS + threadIdx.x;
    int bound = n;
    if (count) {
        const int c = *count;
        bound = c < n ? (c < 0 ? 0 : c) : n;
    }
    const bool handled = j < bound;
    int code = 0;
    if (handled) {
        code = FIN_OTHER;
        const int s = src[j];
        const int records = plies * n_games;                            // fits: shape_ok
        uint64_t fm = 0ull, fo = 0ull;
        if (s >= 0 && s < records && rec_idx[s] >= 0) {
            const size_t G = (size_t)n_games;
            const int g = s % n_games;
            GameS cur = {0ull, 0ull, 1, 0, -1, 0};
            int mover = 0;                                              // the row's own side
            code = FIN_OPEN;
            for (int p = s / n_games; p < plies; ++p) {
                const size_t at = (size_t)p * G + g;
                const int idx = rec_idx[at];
                if (idx < 0) continue;                                  // a ply without a record
                const uint64_t b = rec_black[at], w = rec_white[at];
                const int side = rec_side[at];
                bool ok = !(b & w) && !((b | w) & ~Geo<BS>::FULL) && (side == 1 || side == 2) &&
                          idx <= NSQ;
                if (ok && mover) ok = b == cur.black && w == cur.white && side == cur.side;
                if (ok) {
                    if (!mover) {
                        cur = GameS{b, w, side, 0, -1, 0};
                        mover = side;
                    }
                    ok = make_move<BS>(cur, idx == NSQ ? -1 : idx);
                }
                if (!ok) {                                              // malformed, refused, broken
                    code = FIN_OTHER;
                    break;
                }
                if (cur.over) {
                    code = FIN_OK;
                    break;
                }
            }
            if (code == FIN_OK) {
                fm = mover == 1 ? cur.black : cur.white;
                fo = mover == 1 ? cur.white : cur.black;
            }
        }
        out_final_mover[j] = fm;
        out_final_opponent[j] = fo;
        out_ok[j] = code == FIN_OK ? 1 : 0;
    }
    const int c0 = __popcll(__ballot(handled)), c1 = __popcll(__ballot(code == FIN_OK)),
              c2 = __popcll(__ballot(code == FIN_OPEN)), c3 = __popcll(__ballot(code == FIN_OTHER));
    if (threadIdx.x < 4) {
        const int c = threadIdx.x == 0 ? c0 : (threadIdx.x == 1 ? c1 : (threadIdx.x == 2 ? c2 : c3));
        if (c) atomicAdd((unsigned long long*)out_stats + threadIdx.x, (unsigned long long)c);
    }
}

inline bool shape_ok(int64_t plies, int64_t n_games, int npol) {
    return plies >= 1 && n_games >= 1 && plies <= INT32_MAX / n_games &&
           plies * n_games <= INT32_MAX / npol;     // plies * n_games * npol < 2^31
}

}  // namespace

extern "C" int64_t rvz_records_scratch_size(int32_t plies, int32_t n_games) {
    if (!shape_ok(plies, n_games, 37)) return -1;   // too many records for either board
    return Layout(plies, n_games, nullptr).bytes;
}

extern "C" int rvz_records_games(int32_t bs, int32_t plies, int32_t n_games,
                                 const uint64_t* rec_black, const uint64_t* rec_white,
                                 const int32_t* rec_side, const int32_t* rec_idx,
                                 const double* rec_p, int32_t emit_from, void* scratch,
                                 int32_t* out_m, uint64_t* out_mover, uint64_t* out_opponent,
                                 float* out_policy, float* out_value, int32_t* out_src,
                                 int32_t* out_state, int64_t* out_stats, void* stream) {
    if (!board_ok(bs) || !shape_ok(plies, n_games, bs * bs + 1) || emit_from < 0 ||
        emit_from > plies)
        return RVZ_EINVAL;
    if (!rec_black || !rec_white || !rec_side || !rec_idx || !rec_p || !scratch_ok(scratch) ||
        !out_m || !out_mover || !out_opponent || !out_policy || !out_value || !out_src ||
        !out_stats)
        return RVZ_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const Layout l(plies, n_games, scratch);
    const int records = plies * n_games;
    launch_bs_unchecked(bs, k_rec_walk<8>, k_rec_walk<6>,
                        dim3((n_games + WALK_THREADS - 1) / WALK_THREADS), dim3(WALK_THREADS), s,
                        plies, n_games, rec_black, rec_white, rec_side, rec_idx, emit_from, l.info,
                        l.rank, l.counts);
    hipLaunchKernelGGL(k_rec_scan, dim3(1), dim3(SCAN_THREADS), 0, s, n_games,
                       (const int32_t*)l.counts, l.offset, out_m, out_stats);
    const Geometry g = strided(records, ROWS_WAVES, ROWS_THREADS);
    return launch_bs(bs, k_rec_rows<8>, k_rec_rows<6>, g.grid, g.block, s, records, n_games,
                     rec_black, rec_white, rec_p, (const int32_t*)l.info, (const int32_t*)l.rank,
                     (const int64_t*)l.offset, out_mover, out_opponent, out_policy, out_value,
                     out_src, out_state);
}

extern "C" int rvz_records_final(int32_t bs, int32_t plies, int32_t n_games,
                                 const uint64_t* rec_black, const uint64_t* rec_white,
                                 const int32_t* rec_side, const int32_t* rec_idx, int32_t n,
                                 const int32_t* src, const int32_t* count,
                                 uint64_t* out_final_mover, uint64_t* out_final_opponent,
                                 int32_t* out_ok, int64_t* out_stats, void* stream) {
    if (!board_ok(bs) || !shape_ok(plies, n_games, bs * bs + 1) || n < 0) return RVZ_EINVAL;
    if (!rec_black || !rec_white || !rec_side || !rec_idx || !out_stats) return RVZ_EINVAL;
    if (n > 0 && (!src || !out_final_mover || !out_final_opponent || !out_ok)) return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_final_clear, dim3(1), dim3(64), 0, s, out_stats);
    return launch_bs(bs, k_rec_final<8>, k_rec_final<6>,
                     dim3((unsigned)(((int64_t)n + FINAL_THREADS - 1) / FINAL_THREADS)),
                     dim3(FINAL_THREADS), s, plies, n_games, rec_black, rec_white, rec_side,
                     rec_idx, n, src, count, out_final_mover, out_final_opponent, out_ok,
                     out_stats);
}
