// rvz_dirichlet.hip.h — Dirichlet noise for the priors of a search root (rvz_search_root_noise,
// rvz_dirichlet_noise). Included by csrc/rvz_engine.hip inside its anonymous namespace, after the
// wave primitives (wave_max_f, wave_sum_f).
//
// eta ~ Dirichlet(alpha, ..., alpha) over the k legal squares of a root, one lane per square and
// one wave per game, as a pure function of (seed32, salt, tag, alpha, legal mask): a counter-based
// generator, so no state is carried and the values do not depend on the launch geometry, the
// schedule or which kernel asks.
//  * Philox4x32-10 (Salmon et al., SC'11; rvz_philox.hip.h, included by the translation unit
//    before this file), key (seed32, salt), counter (attempt, square, tag, 0).
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

// rvz_dirichlet_noise's exhaustion flag: the call has no engine, so its ERR_NOISE goes to this
// word of the device, which rvz_check of any engine of the device reports and clears
__device__ int32_t g_noise_err;

// rvz_dirichlet_noise: one wave per row, WPB rows per workgroup
template <int BS>
__global__ __launch_bounds__(256) void k_dirichlet(int n, const uint64_t* __restrict__ legal,
                                                   const uint32_t* __restrict__ seed32,
                                                   const int32_t* __restrict__ tag, uint32_t salt,
                                                   float alpha, float* __restrict__ out,
                                                   uint32_t* __restrict__ out_bits) {
    constexpr int NSQ = Geo<BS>::NSQ, NPOL = Geo<BS>::NPOL;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (r >= n) return;
    const uint64_t V = legal[r] & Geo<BS>::FULL;
    const uint32_t sd = seed32[r], tg = (uint32_t)tag[r];
    const float eta = dirichlet_eta(sd, salt, tg, alpha, V, lane, &g_noise_err);
    if (lane < NSQ) out[(size_t)r * NPOL + lane] = eta;
    if (lane == 0) out[(size_t)r * NPOL + NSQ] = 0.0f;
    if (out_bits && lane < NSQ)
        reinterpret_cast<uint4*>(out_bits)[(size_t)r * NSQ + lane] =
            philox4x32_10(sd, salt, 0u, (uint32_t)lane, tg, 0u);
}
