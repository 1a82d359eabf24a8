// rvz_philox.hip.h — Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy
// as 1, 2, 3", SC'11), the counter-based generator of the root noise (rvz_dirichlet.hip.h) and of
// the replay buffer's draws (rvz_replay.hip): a block of four words as a pure function of a
// 64-bit key and a 128-bit counter, so no state is carried and a value does not depend on the
// launch geometry, the schedule or which kernel asks. Device code only, no storage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rvz {

__device__ __forceinline__ uint4 philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1,
                                               uint32_t c2, uint32_t c3) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

}  // namespace rvz
