// rvz_openings.hip.h — which row of an opening pool a game seeded with `seed` starts from
// (rvz_env_openings, rvz_opening_index; contract in include/rvz.h). One device function, used by
// the engine's reset_game and by the stateless k_opening_index alike, so the two cannot differ.
// Device code only, no storage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rvz_philox.hip.h"

namespace rvz {

// i = floor(x.0 * n / 2^32), x = Philox4x32-10(key (seed, salt), counter (0, 0, 0, 1)); n >= 1.
// Counter word 3 = 1 keeps the block apart from the root noise's (rvz_dirichlet.hip.h: word 3 = 0).
__device__ __forceinline__ int32_t opening_index(uint32_t seed, uint32_t salt, int32_t n) {
    const uint4 x = philox4x32_10(seed, salt, 0u, 0u, 0u, 1u);
    return (int32_t)(((uint64_t)x.x * (uint64_t)(uint32_t)n) >> 32);
}

}  // namespace rvz
