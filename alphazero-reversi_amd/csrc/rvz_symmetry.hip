// rvz_symmetry.hip — the eight symmetries of the square board on bitboards and training rows
// (rvz_board_symmetry, rvz_training_rows; contracts in include/rvz.h).
//
// Numbering: k = 4 * f + r, T_k(x) = fliplr(rot90(x, r)) if f else rot90(x, r) on an [S][S] array
// indexed (row, col) (NumPy's rot90: counter-clockwise). In coordinates, T_k(x)[i][j] =
// x[src_k(i, j)] with
//   k = 0 (i, j)          k = 1 (j, S-1-i)      k = 2 (S-1-i, S-1-j)   k = 3 (S-1-j, i)
//   k = 4 (i, S-1-j)      k = 5 (S-1-j, S-1-i)  k = 6 (S-1-i, j)       k = 7 (j, i)
//
// k_board_symmetry: one lane per board, the transform in registers. 8x8: with t = the transpose
// (three delta swaps) for odd k, else x, every image is t, its 64-bit reversal, its byte swap, or
// both (the mirror of the columns). 6x6: a 36-step bit gather through src_k.
//
// k_training_rows: one wavefront per input row, lane = output square. The row's bitboards and
// side are wave-uniform; each lane looks up its source square, the three image bitboards are
// three ballots, and the policy row moves through one cross-lane read, so nothing is recomputed
// and no table lives in memory. Per image the wave stores the 3*S*S plane floats as float4 (48
// lanes on 8x8, 27 on 6x6), the S*S+1 policy floats as dwords and one quirk word: 1028 B on 8x8
// (1032 B with the quirk), 580 B (584 B) on 6x6, each byte written once. The wave's part
// (write_record, write_image) is in rvz_symmetry.hip.h, shared with the replay's k_replay_batch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rvz.h"
#include "rvz_host.hip.h"
#include "rvz_rules.hip.h"
#include "rvz_symmetry.hip.h"

namespace {

using namespace rvz;

__device__ __forceinline__ uint64_t delta_swap(uint64_t x, uint64_t mask, int shift) {
    const uint64_t t = mask & (x ^ (x << shift));
    return x ^ t ^ (t >> shift);
}

// T_k of an 8x8 bitboard (k in [0, 8)): transpose for odd k, then the reversal of all 64 bits
// (rotation by 180 degrees) for k in {2, 3, 4, 5} and the byte swap (rows mirrored) for k in
// {1, 3, 4, 6}; reversal and byte swap together mirror the columns.
__device__ __forceinline__ uint64_t sym_image8(uint64_t x, int k) {
    uint64_t t = delta_swap(x, 0x0F0F0F0F00000000ull, 28);
    t = delta_swap(t, 0x3333000033330000ull, 14);
    t = delta_swap(t, 0x5500550055005500ull, 7);
    t = (k & 1) ? t : x;
    const uint64_t rv = __brevll(t);
    t = ((0x3Cu >> k) & 1u) ? rv : t;
    const uint64_t sw = __builtin_bswap64(t);
    return ((0x5Au >> k) & 1u) ? sw : t;
}

template <int BS>
__device__ __forceinline__ uint64_t sym_image(uint64_t x, int k) {
    if constexpr (BS == 8) {
        return sym_image8(x, k);
    } else {
        uint64_t y = 0;
#pragma unroll 4
        for (int s = 0; s < Geo<BS>::NSQ; ++s) y |= ((x >> sym_src<BS>(s, k)) & 1ull) << s;
        return y;
    }
}

// out_* may be the input pointers themselves: every lane reads its row before it writes it
template <int BS>
__global__ __launch_bounds__(SYM_THREADS) void k_board_symmetry(
    int n, const uint64_t* black, const uint64_t* white, const int32_t* __restrict__ sym,
    uint64_t* out_black, uint64_t* out_white) {
    const long long step = (long long)gridDim.x * SYM_THREADS;      // n + step can pass 2^31
    for (long long i = (long long)blockIdx.x * SYM_THREADS + threadIdx.x; i < n; i += step) {
        const int k = sym[i];
        const uint64_t b = black[i], w = white[i];
        const bool ok = k >= 0 && k < 8;
        out_black[i] = ok ? sym_image<BS>(b, k & 7) : 0ull;
        out_white[i] = ok ? sym_image<BS>(w, k & 7) : 0ull;
    }
}

template <int BS, int FAN>
__global__ __launch_bounds__(SYM_THREADS) void k_training_rows(
    int n, const uint64_t* __restrict__ black, const uint64_t* __restrict__ white,
    const int32_t* __restrict__ status, const float* __restrict__ policy,
    const int32_t* __restrict__ sym, float* __restrict__ out_states,
    float* __restrict__ out_policy, int32_t* __restrict__ out_quirk) {
    constexpr int NPOL = Geo<BS>::NPOL;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int step = gridDim.x * SYM_WAVES;
    for (int i = blockIdx.x * SYM_WAVES + wave; i < n; i += step) {     // wave-uniform trip count
        const int side = status[4 * i];
        const uint64_t b = black[i], w = white[i];
        const uint64_t P = side == 1 ? b : w, O = side == 1 ? w : b;    // as k_board_canonical
        write_record<BS, FAN>(lane, P, O, policy + (size_t)i * NPOL, true, FAN == 1 ? sym[i] : 0,
                              (size_t)i, out_states, out_policy, out_quirk);
    }
}

}  // namespace

extern "C" int rvz_board_symmetry(int32_t bs, int32_t n, const uint64_t* black,
                                  const uint64_t* white, const int32_t* sym, uint64_t* out_black,
                                  uint64_t* out_white, void* stream) {
    if (!board_ok(bs) || n < 0 ||
        (n > 0 && (!black || !white || !sym || !out_black || !out_white)))
        return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    const Geometry g = strided(n, SYM_THREADS, SYM_THREADS);          // one thread per board
    return launch_bs(bs, k_board_symmetry<8>, k_board_symmetry<6>, g.grid, g.block,
                     (hipStream_t)stream, n, black, white, sym, out_black, out_white);
}

extern "C" int rvz_training_rows(int32_t bs, int32_t n, const uint64_t* black,
                                 const uint64_t* white, const int32_t* status, const float* policy,
                                 const int32_t* sym, int32_t fan, float* out_states,
                                 float* out_policy, int32_t* out_quirk, void* stream) {
    if (!board_ok(bs) || n < 0 || (fan != 1 && fan != 8)) return RVZ_EINVAL;
    if ((int64_t)n * fan * (bs * bs + 1) > INT32_MAX) return RVZ_EINVAL;
    if (n > 0 && (!black || !white || !status || !policy || !out_states || !out_policy ||
                  (fan == 1 && !sym) || ((uintptr_t)out_states & 15u) != 0))   // float4 stores
        return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    const Geometry g = strided(n, SYM_WAVES, SYM_THREADS);            // one wavefront per row
    const auto launch = [&](auto k8, auto k6) {
        return launch_bs(bs, k8, k6, g.grid, g.block, (hipStream_t)stream, n, black, white,
                         status, policy, sym, out_states, out_policy, out_quirk);
    };
    return fan == 1 ? launch(k_training_rows<8, 1>, k_training_rows<6, 1>)
                    : launch(k_training_rows<8, 8>, k_training_rows<6, 8>);
}
