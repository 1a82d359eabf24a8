// rvz_wave.hip.h — the wavefront and workgroup idioms of the record kernels (rvz_merge, the cdf
// table of rvz_replay, rvz_records, rvz_priority, rvz_loss), written once. Device code only, no
// storage: the caller owns the LDS words it passes, and lane / wave are its threadIdx.x & 63 and
// >> 6. (The fused self-play kernel keeps its own DPP-based primitives under its own flags.)
#pragma once
#include <hip/hip_runtime.h>

namespace rvz {

// lane l's sum of lanes 0 .. l of one 64-bit integer a lane (uint64_t or int64_t)
template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

// The float64 scans of rvz_score_loss's cumulative distribution. The order is part of the
// contract, as wave_reduce's is: the steps d = 1, 2, 4, ... 32 in that order, and in each step
// every lane l >= d (prefix) or l + d < 64 (suffix) computes v = v + (the value lane l - d, or
// l + d, held before the step); the other lanes keep theirs. wave_prefix_sum: lane l ends with the
// sum of lanes 0 .. l; wave_suffix_sum: with the sum of lanes l .. 63. The same inputs give the
// same bits on every call.
__device__ __forceinline__ double wave_prefix_sum(double v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double up = __shfl_up(v, d, 64);
        if (lane >= d) v = v + up;
    }
    return v;
}
__device__ __forceinline__ double wave_suffix_sum(double v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double down = __shfl_down(v, d, 64);
        if (lane + d < 64) v = v + down;
    }
    return v;
}

// The xor butterfly: every lane ends with op over the wave's 64 values. The order is part of the
// contract: d = 32, 16, ... 1, each step x = op(x, lane ^ d's x). rvz_loss.hip's float64 outputs
// are defined by it and tests/loss_ref.py restates it; op being commutative, the two lanes of a
// pair compute one result, so every lane ends with the same bits.
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T x, Op op) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = op(x, __shfl_xor(x, d, 64));
    return x;
}
struct Sum {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
template <class T>
__device__ __forceinline__ T wave_sum(T x) { return wave_reduce(x, Sum()); }

// One chunk of a workgroup's running scan of 64-bit integers: a thread's item in, its inclusive
// prefix over the chunk plus `carry` out (less the item: the exclusive one), and carry grows by
// the chunk's total in every thread alike. part: `waves` LDS words. One barrier; every thread of
// the workgroup calls it. A loop over chunks passes two buffers in turn (chunk k + 2 writes chunk
// k's words only behind chunk k + 1's barrier); a single call needs one.
template <class T>
__device__ __forceinline__ T block_scan(T v, int lane, int wave, int waves, T* part, T& carry) {
    v = wave_inclusive_scan(v, lane);
    if (lane == 63) part[wave] = v;
    __syncthreads();
    T before = carry;
    for (int w = 0; w < waves; ++w) {
        const T p = part[w];
        if (w < wave) before += p;
        carry += p;
    }
    return before + v;
}

// x[0 .. N) of every thread reduced over the workgroup: each wave's butterfly, lane 0 parks the N
// results in LDS (part: waves * N words), and thread k < N returns item k's partials combined in
// wave order, wave 0 first; every other thread returns T(). One barrier; every thread calls it.
// k_loss_reduce keeps its own tail: its thread 0 needs all six sums, not one thread a sum.
template <int N, class T, class Op>
__device__ __forceinline__ T block_reduce(const T* x, int lane, int wave, int waves, T* part,
                                          Op op) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const T r = wave_reduce(x[k], op);
        if (lane == 0) part[wave * N + k] = r;
    }
    __syncthreads();
    T all = T();
    if (threadIdx.x < N) {
        all = part[threadIdx.x];
        for (int w = 1; w < waves; ++w) all = op(all, part[w * N + threadIdx.x]);
    }
    return all;
}

}  // namespace rvz
