// rvz_wave_dpp.hip.h — the wavefront primitives of the search kernels (k_step, k_act, k_play) and of
// the root noise: sums on the xor butterfly, maxima and the first-maximum index on the DPP network,
// a lane's value to every lane. Device code only, no storage; one wave of 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rvz {
namespace {

// ---- wave primitives --------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum_i(int x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
__device__ __forceinline__ float wave_sum_f(float x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
// Order key of a non-NaN score for an unsigned max (-0.0 ties +0.0).
__device__ __forceinline__ uint32_t score_key(float s) {
    const uint32_t b = __float_as_uint(s == 0.0f ? 0.0f : s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// Unsigned max over the wave on the DPP network (row shifts, then row broadcasts; lane 63 ends
// with the total): no LDS crossbar traffic, unlike __shfl_xor (ds_bpermute).
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x) {
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false));  // row_shr:1
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false));  // row_shr:2
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false));  // row_shr:4
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false));  // row_shr:8
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false));  // row_bcast:15
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false));  // row_bcast:31
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}
// fmaxf over the wave on the DPP network (order-independent: max is exact)
__device__ __forceinline__ float wave_max_f(float x) {
    const int ninf = (int)0xff800000u;   // -inf: the identity of the lanes a shift leaves empty
    x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(x), 0x111, 0xf, 0xf, false)));
    x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(x), 0x112, 0xf, 0xf, false)));
    x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(x), 0x114, 0xf, 0xf, false)));
    x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(x), 0x118, 0xf, 0xf, false)));
    x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(x), 0x142, 0xa, 0xf, false)));
    x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(x), 0x143, 0xc, 0xf, false)));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}
// First index holding the maximum: Python's `if score > best_score` scan over the children dict
// (mcts.py:423-428). NaN never wins (NaN > x is False); -0.0 ties +0.0. The max key on the DPP
// network, then the lowest lane holding it (all lanes invalid: lane 0).
__device__ __forceinline__ int wave_argmax_first(float s, bool valid, int lane) {
    const uint32_t key = (valid && !isnan(s)) ? score_key(s) : 0u;
    const uint32_t m = wave_max_u32(key);
    return __ffsll((unsigned long long)__ballot(key == m)) - 1;
}
// value of lane `src` (wave-uniform) to every lane
__device__ __forceinline__ int lane_bcast(int x, int src) { return __builtin_amdgcn_readlane(x, src); }
__device__ __forceinline__ float lane_bcast(float x, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), src));
}

}  // namespace
}  // namespace rvz
