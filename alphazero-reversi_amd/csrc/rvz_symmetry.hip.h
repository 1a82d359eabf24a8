// rvz_symmetry.hip.h — what the two kernels that write training rows from bitboards share
// (k_training_rows in rvz_symmetry.hip, k_replay_batch in rvz_replay.hip): the source square of an
// output square under T_k, the wave that writes one image of one row and the one that writes a
// record's rows. Device code only.
// Numbering (include/rvz.h): k = 4 * f + r, T_k(x)[i][j] = x[src_k(i, j)].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rvz_rules.hip.h"

namespace rvz {

constexpr int SYM_THREADS = 256;                 // 4 waves, one row each per step
constexpr int SYM_WAVES = SYM_THREADS / 64;

// the source square of output square s under T_k (k in [0, 8))
template <int BS>
__device__ __forceinline__ int sym_src(int s, int k) {
    const int i = s / BS, j0 = s % BS;
    const int j = (k & 4) ? BS - 1 - j0 : j0;
    const int r = k & 3;
    const int si = r == 0 ? i : (r == 1 ? j : (r == 2 ? BS - 1 - i : BS - 1 - j));
    const int sj = r == 0 ? j : (r == 1 ? BS - 1 - i : (r == 2 ? BS - 1 - j : i));
    return si * BS + sj;
}

// One image of one row, by the whole wave. P, O, V (mover, opponent, legal mask of the original),
// pass and k are wave-uniform; pv is the lane's own policy entry (lane = square). k outside
// [0, 8): an all-zero row and quirk -1.
template <int BS>
__device__ __forceinline__ void write_image(int lane, uint64_t P, uint64_t O, uint64_t V, float pv,
                                            float pass, int k, size_t row,
                                            float* __restrict__ out_states,
                                            float* __restrict__ out_policy,
                                            int32_t* __restrict__ out_quirk) {
    constexpr int NSQ = Geo<BS>::NSQ, NPOL = Geo<BS>::NPOL;
    const bool ok = k >= 0 && k < 8;
    const bool sq = lane < NSQ;
    const int src = sq ? sym_src<BS>(lane, k & 7) : lane;
    const bool take = ok && sq;
    const uint64_t TP = __ballot(take && ((P >> src) & 1ull));
    const uint64_t TO = __ballot(take && ((O >> src) & 1ull));
    const uint64_t TV = __ballot(take && ((V >> src) & 1ull));
    const float moved = __shfl(pv, src, 64);

    if (lane < 3 * NSQ / 4) {                    // NSQ % 4 == 0: a float4 stays within one plane
        const int e = 4 * lane, plane = e / NSQ, s = e % NSQ;
        const uint64_t B = plane == 0 ? TP : (plane == 1 ? TO : TV);
        const uint32_t nib = (uint32_t)(B >> s) & 0xFu;
        reinterpret_cast<float4*>(out_states + row * (3 * NSQ))[lane] =
            make_float4((float)(nib & 1u), (float)((nib >> 1) & 1u), (float)((nib >> 2) & 1u),
                        (float)(nib >> 3));
    }
    float* prow = out_policy + row * NPOL;
    if (lane < NPOL) prow[lane] = ok ? (sq ? moved : pass) : 0.0f;
    if (NPOL > 64 && lane == 0) prow[NSQ] = ok ? pass : 0.0f;
    if (out_quirk) {             // wave-uniform; the image position's own mask, a direction per lane
        const uint64_t own = legal_wave<BS>(TP, TO, lane);
        if (lane == 0) out_quirk[row] = ok ? (int32_t)(own != TV) : -1;
    }
}

// The rows of one record (P, O, its policy row prow), by the whole wave; all wave-uniform. prow
// is read only if has_policy (else: zeros): the caller's own condition, not a null test, so no
// caller branches twice. FAN == 1: output row `row` is the image under T_k (k outside [0, 8):
// write_image's zero row). FAN == 8: k is not read, rows 8 * row + j are the images under T_j.
template <int BS, int FAN>
__device__ __forceinline__ void write_record(int lane, uint64_t P, uint64_t O,
                                             const float* __restrict__ prow, bool has_policy,
                                             int k, size_t row, float* __restrict__ out_states,
                                             float* __restrict__ out_policy,
                                             int32_t* __restrict__ out_quirk) {
    constexpr int NSQ = Geo<BS>::NSQ;
    const uint64_t V = legal<BS>(P, O);
    float pv = 0.0f, pass = 0.0f;
    if (has_policy) {                            // wave-uniform
        pv = lane < NSQ ? prow[lane] : 0.0f;
        pass = prow[NSQ];
    }
    if constexpr (FAN == 1) {
        write_image<BS>(lane, P, O, V, pv, pass, k, row, out_states, out_policy, out_quirk);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            write_image<BS>(lane, P, O, V, pv, pass, j, row * 8 + j, out_states, out_policy,
                            out_quirk);
    }
}

}  // namespace rvz
