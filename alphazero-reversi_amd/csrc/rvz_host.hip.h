// rvz_host.hip.h — the host side of a launch that every translation unit writes the same way:
// the board-size rule, the 8 / 6 dispatch as a pair of kernel pointers with the arguments written
// once, the error return, the launch geometries of the row kernels (a row per wavefront or thread;
// the capped grid of those that stride), and a scratch buffer's parts carved from one description.
// Host code only, no storage: all inline.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rvz.h"

namespace rvz {

inline bool board_ok(int bs) { return bs == 8 || bs == 6; }

// after the last of a call's launches: its error return answers for all of them
inline int last_launch() { return hipGetLastError() == hipSuccess ? RVZ_OK : RVZ_EHIP; }

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
    return last_launch();
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

inline int64_t up16(int64_t bytes) { return (bytes + 15) & ~(int64_t)15; }
// a caller's scratch: there, and aligned for the parts below
inline bool scratch_ok(const void* p) { return p && ((uintptr_t)p & 15u) == 0; }

// A scratch buffer's parts in order. A translation unit describes its scratch in one function
// built on this; its entry point calls that function on the caller's scratch and its size function
// on a null one, where the parts' addresses mean nothing and `at` is the size.
struct Carver {
    uintptr_t base;                              // the scratch's address, or 0
    int64_t at = 0;                              // the bytes taken so far
    explicit Carver(void* scratch) : base((uintptr_t)scratch) {}
    // the next part, `count` T's: padded to a multiple of 16 bytes, or packed (what follows it is
    // only as aligned as the part leaves it)
    template <class T>
    T* take(int64_t count) { return bytes<T>(up16((int64_t)sizeof(T) * count)); }
    template <class T>
    T* packed(int64_t count) { return bytes<T>((int64_t)sizeof(T) * count); }
    template <class T>
    T* bytes(int64_t n) { return (T*)(base + (uintptr_t)((at += n) - n)); }
};

}  // namespace rvz
