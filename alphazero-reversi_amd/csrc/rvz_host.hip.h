// rvz_host.hip.h — the host side of a launch that every translation unit writes the same way:
// the board-size rule, the 8 / 6 dispatch as a pair of kernel pointers with the arguments written
// once, the error return, and the launch geometries of the row kernels (a row per wavefront or
// thread; the capped grid of those that stride). Host code only, no storage: all inline.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rvz.h"

namespace rvz {

inline bool board_ok(int bs) { return bs == 8 || bs == 6; }

// the launch of k8 (bs == 8) or k6 alone: the caller reads hipGetLastError() itself
template <class... P, class... A>
inline void launch_bs_unchecked(int bs, void (*k8)(P...), void (*k6)(P...), dim3 grid, dim3 block,
                                hipStream_t s, A... args) {
    hipLaunchKernelGGL(bs == 8 ? k8 : k6, grid, block, 0, s, args...);
}

// launches k8 (bs == 8) or k6; RVZ_OK or RVZ_EHIP
template <class... P, class... A>
inline int launch_bs(int bs, void (*k8)(P...), void (*k6)(P...), dim3 grid, dim3 block,
                     hipStream_t s, A... args) {
    launch_bs_unchecked(bs, k8, k6, grid, block, s, args...);
    return hipGetLastError() == hipSuccess ? RVZ_OK : RVZ_EHIP;
}

struct Geometry {
    dim3 grid, block;
};
// one wavefront per row, wpb rows per workgroup
inline Geometry wave_per_row(int n, int wpb) { return {dim3((n + wpb - 1) / wpb), dim3(wpb * 64)}; }
// one thread per row, 256 per workgroup
inline Geometry thread_per_row(int n) { return {dim3((n + 255) / 256), dim3(256)}; }
// a grid-stride kernel: per_block units per workgroup and step, at most 2,048 workgroups
constexpr int STRIDED_MAX_BLOCKS = 2048;
inline Geometry strided(int64_t units, int per_block, int threads) {
    const int64_t need = (units + per_block - 1) / per_block;
    return {dim3((unsigned)(need < STRIDED_MAX_BLOCKS ? need : STRIDED_MAX_BLOCKS)), dim3(threads)};
}

}  // namespace rvz
