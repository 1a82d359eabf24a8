// rvz_dirichlet.hip.h — Dirichlet noise for the priors of a search root (rvz_search_root_noise,
// rvz_dirichlet_noise): dirichlet_eta, the device function of the search's root noise (k_step,
// k_play) and of k_dirichlet (csrc/rvz_engine.hip). Needs the wave reductions wave_max_f and
// wave_sum_f (rvz_wave_dpp.hip.h) and the generator (rvz_philox.hip.h).
//
// eta ~ Dirichlet(alpha, ..., alpha) over the k legal squares of a root, one lane per square and
// one wave per game, as a pure function of (seed32, salt, tag, alpha, legal mask): a counter-based
// generator, so no state is carried and the values do not depend on the launch geometry, the
// schedule or which kernel asks.
//  * Philox4x32-10 (Salmon et al., SC'11; rvz_philox.hip.h), key (seed32, salt), counter
//    (attempt, square, tag, 0).
//  * Gamma(alpha) per legal square by Marsaglia-Tsang rejection (ACM TOMS 26(3), 2000): the normal
//    by Box-Muller from words 0 and 1 of the attempt's block, the acceptance uniform from word 2;
//    every attempt is a new block (the attempt index is a counter word). alpha < 1 samples
//    Gamma(alpha + 1) and applies the boost G(alpha) = G(alpha + 1) * u^(1/alpha), u from word 3
//    of attempt 0.
//  * Everything stays in the log domain (u^(1/alpha) underflows float32 at the reference's
//    alpha = 0.03): lg = log g per square, eta = exp(lg - max lg) / sum, the maximum and the sum
//    by the fixed-order wave reductions.
//  * Uniforms are 23-bit, (m + 0.5) * 2^-23: the open interval (0, 1), every value exact in
//    float32, so no log(0).
//  * The rejection loop is bounded (NOISE_ATTEMPTS; the expected count is about 1.05): on
//    exhaustion the lane takes its last positive proposal (or v = 1) and ERR_NOISE is raised.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rvz_philox.hip.h"
#include "rvz_wave_dpp.hip.h"

namespace rvz {
namespace {

constexpr int32_t ERR_NOISE = 32;   // a Gamma rejection loop ran out of attempts (device error word)
constexpr int NOISE_ATTEMPTS = 64;

// the top 23 bits of a word as a uniform of the open interval (0, 1)
__device__ __forceinline__ float noise_u01(uint32_t w) {
    return ((float)(w >> 9) + 0.5f) * 0x1p-23f;
}

// eta of square `lane` (0 at a square that is not in V). Called by a whole wave (the reductions
// use every lane) from a wave-uniform branch; kept out of line so that the callers' register
// allocation is that of the code without it. All arguments by value: no frame, no scratch.
__device__ __forceinline__ float dirichlet_eta(uint32_t seed32, uint32_t salt, uint32_t tag,
                                            float alpha, uint64_t V, int lane, int32_t* err) {
    if (V == 0ull) return 0.0f;
    const bool legal = (V >> lane) & 1ull;
    const bool boost = alpha < 1.0f;
    const float a1 = boost ? alpha + 1.0f : alpha;
    const float d = a1 - (1.0f / 3.0f);
    const float c = 1.0f / sqrtf(9.0f * d);
    float lg = -INFINITY;
    if (legal) {
        float logv = 0.0f;       // log of the last positive proposal's v (v = 1 if none)
        uint32_t w3 = 0;         // word 3 of attempt 0: the boost's uniform
        bool accepted = false;
        for (int t = 0; t < NOISE_ATTEMPTS; ++t) {
            const uint4 b = philox4x32_10(seed32, salt, (uint32_t)t, (uint32_t)lane, tag, 0u);
            if (t == 0) w3 = b.w;
            const float x = sqrtf(-2.0f * logf(noise_u01(b.x))) * cospif(2.0f * noise_u01(b.y));
            const float t1 = 1.0f + c * x;
            if (t1 <= 0.0f) continue;
            const float v = t1 * t1 * t1;
            if (!(v > 0.0f)) continue;
            logv = logf(v);
            if (logf(noise_u01(b.z)) < 0.5f * x * x + d - d * v + d * logv) {
                accepted = true;
                break;
            }
        }
        if (!accepted) atomicOr(err, ERR_NOISE);
        lg = logf(d) + logv;
        if (boost) lg += logf(noise_u01(w3)) / alpha;
        lg = fmaxf(lg, -3.0e38f);   // a tiny alpha: finite, so that lg - max is never inf - inf
    }
    const float mx = wave_max_f(lg);
    const float ex = legal ? expf(lg - mx) : 0.0f;
    return ex / wave_sum_f(ex);
}

}  // namespace
}  // namespace rvz
