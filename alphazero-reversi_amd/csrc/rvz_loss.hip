// rvz_loss.hip — the policy/value loss on the full policy target, forward and backward in one
// call (rvz_policy_value_loss; contract and definition in include/rvz.h).
//
// All arithmetic is float64 on the float32 inputs; the row data is about 0.5 KB, so the call is
// bound by launches and by the latency of a row's exp / log chain, not by memory or occupancy:
// one wavefront per row, lane = action index, nothing in LDS but the reduction's 16 partials.
//
// Three kinds of launch on the caller's stream, no host step between them:
//   k_loss_rows    one wavefront per row: the malformed-row rules, then m, lse, S, Lp, H, Lv and
//                  the agreement, each wave sum a fixed float64 butterfly (rvz_wave.hip.h: every
//                  lane ends with the same bits). The row's {Lp, Lv, H} go to out_row; its six
//                  terms (w, w Lp, w Lv, w H, w agree, malformed) and {lse, S} go to the scratch.
//   k_loss_reduce  the cross-row tree, one launch per level: a workgroup of 1024 threads sums
//                  RED_CHUNK = 4096 consecutive items of each of the six terms (thread t adds
//                  items t, t + 1024, t + 2048, t + 3072 in that order; the 64 lanes of a wave by
//                  the butterfly; the 16 waves in order) into one item of the next level. The level
//                  of one workgroup is the last: it writes out_loss and W. One level up to 4096
//                  rows, two up to 2^24, three beyond. The order is a function of n alone.
//   k_loss_grads   (with gradients) one wavefront per row: p = exp(z - lse) again from the saved
//                  lse, then the two gradients, scaled by w / W.
// No floating-point atomics anywhere; every output element is written by exactly one lane.
// rvz_ownership_loss (the auxiliary ownership head's loss) runs its own two row kernels around the
// same k_loss_reduce, on the same scratch, and so does rvz_score_loss (the final-score head's loss).
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rvz.h"
#include "rvz_host.hip.h"
#include "rvz_wave.hip.h"

namespace {

using namespace rvz;

constexpr int LOSS_WAVES = 4;                    // rows per workgroup in the two row kernels
constexpr int LOSS_THREADS = LOSS_WAVES * 64;
constexpr int RED_THREADS = 1024;
constexpr int RED_ITEMS = 4;                     // items per thread and term
constexpr int RED_CHUNK = RED_THREADS * RED_ITEMS;
constexpr int NTERM = 6;                         // w, w Lp, w Lv, w H, w agree, malformed
constexpr int MAX_LEVELS = 3;                    // 4096^3 > 2^31 / 37

struct Layout {                                  // the scratch's parts
    double *hdr, *aux, *level[MAX_LEVELS];
    int64_t total = -1;                          // -1: bad arguments
    int32_t count[MAX_LEVELS + 1];               // items of each level; count[levels] == 1
    int32_t levels = 0;
    Layout(int32_t bs, int32_t n, void* scratch) {
        if (!board_ok(bs) || n < 0 || (int64_t)n * (bs * bs + 1) > INT32_MAX) return;
        Carver c(scratch);
        hdr = c.take<double>(8);                 // [0]: W
        aux = c.packed<double>(2 * (int64_t)n);  // {lse, S} per row
        int32_t m = n;
        do {                                     // level k: NTERM arrays of count[k] doubles
            count[levels] = m;
            level[levels] = c.packed<double>((int64_t)NTERM * m);
            m = (m + RED_CHUNK - 1) / RED_CHUNK;
            ++levels;
        } while (m > 1);
        count[levels] = 1;
        total = c.at;
    }
};

template <int BS>
struct LG {
    static constexpr int NPOL = BS * BS + 1;
    static constexpr int SLOTS = (NPOL + 63) / 64;      // entries a lane carries: lane, lane + 64
};

// the first maximum of a row: (value, index) under "larger value, then lower index"
__device__ __forceinline__ int wave_argmax(float v, int i) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ov = __shfl_xor(v, d, 64);
        const int oi = __shfl_xor(i, d, 64);
        const bool take = ov > v || (ov == v && oi < i);
        v = take ? ov : v;
        i = take ? oi : i;
    }
    return i;
}

__device__ __forceinline__ bool finite32(float x) { return fabsf(x) <= FLT_MAX; }   // NaN: false

template <int BS>
__global__ __launch_bounds__(LOSS_THREADS) void k_loss_rows(
    int n, const float* __restrict__ logits, const float* __restrict__ value,
    const float* __restrict__ policy_target, const float* __restrict__ value_target,
    const float* __restrict__ weight, double* __restrict__ aux, double* __restrict__ term,
    double* __restrict__ out_row) {
    constexpr int NPOL = LG<BS>::NPOL, SLOTS = LG<BS>::SLOTS;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r = blockIdx.x * LOSS_WAVES + wave;        // n * NPOL fits int32
    if (r >= n) return;                                  // wave-uniform
    const float* zrow = logits + (size_t)r * NPOL;
    const float* prow = policy_target + (size_t)r * NPOL;
    float z[SLOTS], pi[SLOTS];
    bool bad = false;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int e = lane + 64 * s;
        const bool in = e < NPOL;
        z[s] = in ? zrow[e] : -INFINITY;                 // an empty slot: never a maximum, exp 0
        pi[s] = in ? prow[e] : 0.0f;
        bad |= in && (!finite32(z[s]) || !(pi[s] >= 0.0f && pi[s] <= 1.0f));
    }
    const float yf = value[r], tf = value_target[r], wf = weight ? weight[r] : 1.0f;
    bad |= !finite32(yf) || !(tf >= -1.0f && tf <= 1.0f) || !(wf >= 0.0f && wf <= FLT_MAX);
    const bool ok = __ballot(bad) == 0;

    double lse = 0.0, S = 0.0, Lp = 0.0, H = 0.0, Lv = 0.0, w = 0.0, agree = 0.0;
    if (ok) {                                            // wave-uniform
        float zm = z[0], pm = pi[0];
        int zi = lane, pidx = lane;
#pragma unroll
        for (int s = 1; s < SLOTS; ++s) {                // lane + 64 s is the higher index
            if (z[s] > zm) { zm = z[s]; zi = lane + 64 * s; }
            if (pi[s] > pm) { pm = pi[s]; pidx = lane + 64 * s; }
        }
        const float mx = wave_reduce(zm, [](float a, float b) { return fmaxf(a, b); });
        const int zarg = wave_argmax(zm, zi);
        // an empty lane's pi is 0 at an index >= NPOL: ties go to the lower index, so it never wins
        const int parg = wave_argmax(pm, pidx);
        const double m = (double)mx;
        double se = 0.0, sp = 0.0;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            if (lane + 64 * s < NPOL) {
                se += exp((double)z[s] - m);
                sp += (double)pi[s];
            }
        }
        lse = m + log(wave_sum(se));
        S = wave_sum(sp);
        double lp = 0.0, h = 0.0;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            if (pi[s] > 0.0f) {                          // an empty slot holds 0
                const double q = (double)pi[s];
                lp += q * ((double)z[s] - lse);
                h += q * log(q);
            }
        }
        Lp = -wave_sum(lp);
        H = -wave_sum(h);
        const double dv = (double)yf - (double)tf;
        Lv = dv * dv;
        w = (double)wf;
        agree = zarg == parg ? 1.0 : 0.0;
    }
    if (lane == 0) {
        aux[2 * (size_t)r] = lse;
        aux[2 * (size_t)r + 1] = S;
        term[r] = w;
        term[(size_t)n + r] = w * Lp;
        term[2 * (size_t)n + r] = w * Lv;
        term[3 * (size_t)n + r] = w * H;
        term[4 * (size_t)n + r] = w * agree;
        term[5 * (size_t)n + r] = ok ? 0.0 : 1.0;
        if (out_row) {
            out_row[3 * (size_t)r] = Lp;
            out_row[3 * (size_t)r + 1] = Lv;
            out_row[3 * (size_t)r + 2] = H;
        }
    }
}

// one level of the cross-row tree: NTERM arrays of m items -> NTERM arrays of gridDim.x items
__global__ __launch_bounds__(RED_THREADS) void k_loss_reduce(
    int m, const double* __restrict__ src, double* __restrict__ dst, double policy_weight,
    double value_weight, double* __restrict__ hdr, double* __restrict__ out_loss) {
    __shared__ double part[NTERM][RED_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * RED_CHUNK + threadIdx.x;
#pragma unroll
    for (int q = 0; q < NTERM; ++q) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < RED_ITEMS; ++k) {
            const int64_t i = base + (int64_t)k * RED_THREADS;
            v += i < m ? src[(size_t)q * m + i] : 0.0;
        }
        v = wave_sum(v);
        if (lane == 0) part[q][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s[NTERM];
#pragma unroll
    for (int q = 0; q < NTERM; ++q) {
        double v = part[q][0];
        for (int k = 1; k < RED_THREADS / 64; ++k) v += part[q][k];
        s[q] = v;
    }
    if (gridDim.x > 1) {
#pragma unroll
        for (int q = 0; q < NTERM; ++q) dst[(size_t)q * gridDim.x + blockIdx.x] = s[q];
        return;
    }
    const double W = s[0];
    const bool any = W > 0.0;
    const double P = any ? s[1] / W : 0.0, V = any ? s[2] / W : 0.0;
    hdr[0] = W;
    out_loss[0] = policy_weight * P + value_weight * V;
    out_loss[1] = P;
    out_loss[2] = V;
    out_loss[3] = any ? s[3] / W : 0.0;
    out_loss[4] = W;
    out_loss[5] = any ? s[4] / W : 0.0;
    out_loss[6] = s[5];
    out_loss[7] = 0.0;
}

template <int BS>
__global__ __launch_bounds__(LOSS_THREADS) void k_loss_grads(
    int n, const float* __restrict__ logits, const float* __restrict__ value,
    const float* __restrict__ policy_target, const float* __restrict__ value_target,
    const double* __restrict__ aux, const double* __restrict__ term,
    const double* __restrict__ hdr, double policy_weight, double value_weight,
    float* __restrict__ grad_logits, float* __restrict__ grad_value) {
    constexpr int NPOL = LG<BS>::NPOL, SLOTS = LG<BS>::SLOTS;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r = blockIdx.x * LOSS_WAVES + wave;
    if (r >= n) return;                                  // wave-uniform
    const double W = hdr[0], w = term[r];                // w: 0 for a malformed row
    float* grow = grad_logits + (size_t)r * NPOL;
    if (!(W > 0.0) || !(w > 0.0)) {                      // wave-uniform: nothing of the row is read
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
            if (lane + 64 * s < NPOL) grow[lane + 64 * s] = 0.0f;
        if (lane == 0) grad_value[r] = 0.0f;
        return;
    }
    const double lse = aux[2 * (size_t)r], S = aux[2 * (size_t)r + 1];
    const double cp = policy_weight * w / W, cv = value_weight * w / W;
    const float* zrow = logits + (size_t)r * NPOL;
    const float* prow = policy_target + (size_t)r * NPOL;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int e = lane + 64 * s;
        if (e < NPOL) {
            const double p = exp((double)zrow[e] - lse);
            grow[e] = (float)(cp * (S * p - (double)prow[e]));
        }
    }
    if (lane == 0)
        grad_value[r] = (float)(cv * 2.0 * ((double)value[r] - (double)value_target[r]));
}

// ---------------------------------------------------------------- the ownership loss
// rvz_ownership_loss: the same three kinds of launch on the same scratch. A row is S*S squares,
// lane = square; its terms go into the six arrays of the tree in the policy loss's places (w,
// w L, 0, 0, w agree, malformed), so k_loss_reduce sums and finishes them as it is, with the
// weights 1 and 0: out_loss = {L, L, 0, 0, W, agreement, malformed, 0}.
template <int BS>
__global__ __launch_bounds__(LOSS_THREADS) void k_own_rows(
    int n, const float* __restrict__ logits, const float* __restrict__ target,
    const float* __restrict__ weight, double* __restrict__ term, double* __restrict__ out_row) {
    constexpr int NSQ = BS * BS;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r = blockIdx.x * LOSS_WAVES + wave;        // n * (NSQ + 1) fits int32
    if (r >= n) return;                                  // wave-uniform
    const bool in = lane < NSQ;
    const float o = in ? logits[(size_t)r * NSQ + lane] : 0.0f;
    const float t = in ? target[(size_t)r * NSQ + lane] : 0.0f;
    const float wf = weight ? weight[r] : 1.0f;
    const bool bad = !finite32(o) || !(t == -1.0f || t == 0.0f || t == 1.0f) ||
                     !(wf >= 0.0f && wf <= FLT_MAX);
    const bool ok = __ballot(bad) == 0;
    double L = 0.0, w = 0.0, agree = 0.0;
    if (ok) {                                            // wave-uniform
        const double d = in ? tanh((double)o) - (double)t : 0.0;
        L = wave_sum(d * d) / (double)NSQ;
        const int labelled = __popcll(__ballot(t != 0.0f));
        const int hits = __popcll(__ballot((t > 0.0f && o > 0.0f) || (t < 0.0f && o < 0.0f)));
        agree = labelled ? (double)hits / (double)labelled : 0.0;
        w = (double)wf;
    }
    if (lane == 0) {
        term[r] = w;
        term[(size_t)n + r] = w * L;
        term[2 * (size_t)n + r] = 0.0;
        term[3 * (size_t)n + r] = 0.0;
        term[4 * (size_t)n + r] = w * agree;
        term[5 * (size_t)n + r] = ok ? 0.0 : 1.0;
        if (out_row) {
            out_row[2 * (size_t)r] = L;
            out_row[2 * (size_t)r + 1] = agree;
        }
    }
}

template <int BS>
__global__ __launch_bounds__(LOSS_THREADS) void k_own_grads(
    int n, const float* __restrict__ logits, const float* __restrict__ target,
    const double* __restrict__ term, const double* __restrict__ hdr,
    float* __restrict__ grad_logits) {
    constexpr int NSQ = BS * BS;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r = blockIdx.x * LOSS_WAVES + wave;
    if (r >= n || lane >= NSQ) return;
    const double W = hdr[0], w = term[r];                // w: 0 for a malformed row
    const size_t at = (size_t)r * NSQ + lane;
    if (!(W > 0.0) || !(w > 0.0)) {                      // wave-uniform: nothing of the row is read
        grad_logits[at] = 0.0f;
        return;
    }
    const double th = tanh((double)logits[at]);
    grad_logits[at] =
        (float)((w / W) * (2.0 / (double)NSQ) * (th - (double)target[at]) * (1.0 - th * th));
}

// ---------------------------------------------------------------- the score loss
// rvz_score_loss: the same three kinds of launch on the same scratch. A row is K = 2 S*S + 1
// classes, class k the final margin k - S*S. A lane holds CPL consecutive classes (lane l the
// classes l * CPL .. l * CPL + CPL - 1: 3 a lane on 8x8, 2 on 6x6), so the cumulative distribution
// is a lane-local running sum on top of one wave scan of the lanes' totals; the strided layout of
// k_loss_rows would need a scan per slot. The row kernel saves {lse, Qr} in the scratch's aux
// pair; the gradient kernel recomputes p, C and e from lse by the same device function, so the
// two agree bit for bit. The terms go into the six arrays of the tree as w, w Lpdf, w Lcdf,
// w abserr, w agree, malformed, which k_loss_reduce sums and finishes as it is.
template <int BS>
struct SG {
    static constexpr int NSQ = BS * BS;
    static constexpr int K = 2 * NSQ + 1;
    static constexpr int CPL = (K + 63) / 64;            // classes a lane holds
};

// p[i] = exp(z[i] - lse), C[i] = the cumulative sum up to the lane's class i, e[i] = C[i] - T[i]
// for the thresholds j <= K - 2 and 0 beyond; c: the target class
template <int BS>
__device__ __forceinline__ void score_cdf(const float* z, double lse, int c, int lane,
                                          double* p, double* C, double* e) {
    constexpr int K = SG<BS>::K, CPL = SG<BS>::CPL;
    double run = 0.0;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        p[i] = lane * CPL + i < K ? exp((double)z[i] - lse) : 0.0;
        run = i == 0 ? p[0] : run + p[i];
        C[i] = run;                                      // the lane's own running sum so far
    }
    const double incl = wave_prefix_sum(run, lane);
    const double below = __shfl_up(incl, 1, 64);
    const double before = lane == 0 ? 0.0 : below;       // the lanes below this one
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int k = lane * CPL + i;
        C[i] = before + C[i];
        e[i] = k <= K - 2 ? C[i] - (k >= c ? 1.0 : 0.0) : 0.0;
    }
}

template <int BS>
__global__ __launch_bounds__(LOSS_THREADS) void k_score_rows(
    int n, const float* __restrict__ logits, const float* __restrict__ margin,
    const float* __restrict__ weight, double* __restrict__ aux, double* __restrict__ term,
    double* __restrict__ out_row) {
    constexpr int NSQ = SG<BS>::NSQ, K = SG<BS>::K, CPL = SG<BS>::CPL;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r = blockIdx.x * LOSS_WAVES + wave;        // n * K fits int32
    if (r >= n) return;                                  // wave-uniform
    const float* zrow = logits + (size_t)r * K;
    float z[CPL];
    bool bad = false;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int k = lane * CPL + i;
        const bool in = k < K;
        z[i] = in ? zrow[k] : -INFINITY;                 // an empty slot: never a maximum, exp 0
        bad |= in && !finite32(z[i]);
    }
    const float mf = margin[r], wf = weight ? weight[r] : 1.0f;
    bad |= !(mf >= -(float)NSQ && mf <= (float)NSQ) || mf != truncf(mf) ||
           !(wf >= 0.0f && wf <= FLT_MAX);               // NaN fails the range tests
    const bool ok = __ballot(bad) == 0;

    double lse = 0.0, Qr = 0.0, Lpdf = 0.0, Lcdf = 0.0, mean = 0.0, abserr = 0.0, w = 0.0,
           agree = 0.0;
    if (ok) {                                            // wave-uniform
        const int c = (int)mf + NSQ;
        float zm = z[0];
        int zi = lane * CPL;
#pragma unroll
        for (int i = 1; i < CPL; ++i)
            if (z[i] > zm) { zm = z[i]; zi = lane * CPL + i; }
        const float mx = wave_reduce(zm, [](float a, float b) { return fmaxf(a, b); });
        const int zarg = wave_argmax(zm, zi);            // an empty lane holds -inf: never wins
        const double m = (double)mx;
        double se = 0.0;
#pragma unroll
        for (int i = 0; i < CPL; ++i)
            if (lane * CPL + i < K) se += exp((double)z[i] - m);
        lse = m + log(wave_sum(se));
        double p[CPL], C[CPL], e[CPL];
        score_cdf<BS>(z, lse, c, lane, p, C, e);
        double sq = 0.0, q = 0.0, mu = 0.0;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            sq += e[i] * e[i];
            q += e[i] * C[i];
            mu += p[i] * (double)(lane * CPL + i - NSQ);
        }
        Lcdf = wave_sum(sq) / (double)(K - 1);
        Qr = wave_sum(q);
        mean = wave_sum(mu);
        Lpdf = lse - (double)zrow[c];                    // 0 <= c < K: the margin is in range
        abserr = fabs(mean - (double)mf);
        agree = zarg == c ? 1.0 : 0.0;
        w = (double)wf;
    }
    if (lane == 0) {
        aux[2 * (size_t)r] = lse;
        aux[2 * (size_t)r + 1] = Qr;
        term[r] = w;
        term[(size_t)n + r] = w * Lpdf;
        term[2 * (size_t)n + r] = w * Lcdf;
        term[3 * (size_t)n + r] = w * abserr;
        term[4 * (size_t)n + r] = w * agree;
        term[5 * (size_t)n + r] = ok ? 0.0 : 1.0;
        if (out_row) {
            out_row[4 * (size_t)r] = Lpdf;
            out_row[4 * (size_t)r + 1] = Lcdf;
            out_row[4 * (size_t)r + 2] = mean;
            out_row[4 * (size_t)r + 3] = agree;
        }
    }
}

template <int BS>
__global__ __launch_bounds__(LOSS_THREADS) void k_score_grads(
    int n, const float* __restrict__ logits, const float* __restrict__ margin,
    const double* __restrict__ aux, const double* __restrict__ term,
    const double* __restrict__ hdr, double pdf_weight, double cdf_weight,
    float* __restrict__ grad_logits) {
    constexpr int NSQ = SG<BS>::NSQ, K = SG<BS>::K, CPL = SG<BS>::CPL;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r = blockIdx.x * LOSS_WAVES + wave;
    if (r >= n) return;                                  // wave-uniform
    const double W = hdr[0], w = term[r];                // w: 0 for a malformed row
    float* grow = grad_logits + (size_t)r * K;
    if (!(W > 0.0) || !(w > 0.0)) {                      // wave-uniform: nothing of the row is read
#pragma unroll
        for (int i = 0; i < CPL; ++i)
            if (lane * CPL + i < K) grow[lane * CPL + i] = 0.0f;
        return;
    }
    const double lse = aux[2 * (size_t)r], Qr = aux[2 * (size_t)r + 1];
    const int c = (int)margin[r] + NSQ;                  // w > 0: the row is well-formed
    const float* zrow = logits + (size_t)r * K;
    float z[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) z[i] = lane * CPL + i < K ? zrow[lane * CPL + i] : -INFINITY;
    double p[CPL], C[CPL], e[CPL], R[CPL];
    score_cdf<BS>(z, lse, c, lane, p, C, e);
    double run = 0.0;                                    // R: the suffix sums of e, from the top
#pragma unroll
    for (int i = CPL - 1; i >= 0; --i) {
        run = i == CPL - 1 ? e[i] : run + e[i];
        R[i] = run;
    }
    const double incl = wave_suffix_sum(run, lane);
    const double above = __shfl_down(incl, 1, 64);
    const double after = lane == 63 ? 0.0 : above;       // the lanes above this one
    const double cw = cdf_weight * (2.0 / (double)(K - 1));
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int k = lane * CPL + i;
        if (k < K)
            grow[k] = (float)((w / W) * (pdf_weight * (p[i] - (k == c ? 1.0 : 0.0)) +
                                         cw * p[i] * ((after + R[i]) - Qr)));
    }
}

}  // namespace

extern "C" int64_t rvz_score_loss_scratch_size(int32_t bs, int32_t n) {
    if (!board_ok(bs) || n < 0 || (int64_t)n * (2 * bs * bs + 1) > INT32_MAX) return -1;
    return Layout(bs, n, nullptr).total;                 // the policy loss's scratch, as it is
}

extern "C" int rvz_score_loss(int32_t bs, int32_t n, const float* logits, const float* margin,
                              const float* weight, double pdf_weight, double cdf_weight,
                              void* scratch, double* out_loss, double* out_row,
                              float* grad_logits, void* stream) {
    if (rvz_score_loss_scratch_size(bs, n) < 0) return RVZ_EINVAL;
    if (!(pdf_weight >= 0.0 && pdf_weight <= DBL_MAX) ||
        !(cdf_weight >= 0.0 && cdf_weight <= DBL_MAX))
        return RVZ_EINVAL;
    if (n > 0 && (!logits || !margin || !scratch_ok(scratch) || !out_loss)) return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    const Layout L(bs, n, scratch);
    hipStream_t s = (hipStream_t)stream;
    const Geometry rows = wave_per_row(n, LOSS_WAVES);
    launch_bs_unchecked(bs, k_score_rows<8>, k_score_rows<6>, rows.grid, rows.block, s, n, logits,
                        margin, weight, L.aux, L.level[0], out_row);
    for (int k = 0; k < L.levels; ++k) {
        double* dst = k + 1 < L.levels ? L.level[k + 1] : nullptr;
        hipLaunchKernelGGL(k_loss_reduce, dim3(L.count[k + 1]), dim3(RED_THREADS), 0, s,
                           L.count[k], (const double*)L.level[k], dst, pdf_weight, cdf_weight,
                           L.hdr, out_loss);
    }
    if (!grad_logits) return last_launch();
    return launch_bs(bs, k_score_grads<8>, k_score_grads<6>, rows.grid, rows.block, s, n, logits,
                     margin, (const double*)L.aux, (const double*)L.level[0],
                     (const double*)L.hdr, pdf_weight, cdf_weight, grad_logits);
}

extern "C" int64_t rvz_ownership_loss_scratch_size(int32_t bs, int32_t n) {
    return Layout(bs, n, nullptr).total;                 // the policy loss's scratch, as it is
}

extern "C" int rvz_ownership_loss(int32_t bs,int32_t n, const float* logits, const float* target,
                                  const float* weight, void* scratch, double* out_loss,
                                  double* out_row, float* grad_logits, void* stream) {
    const Layout L(bs, n, scratch);
    if (L.total < 0) return RVZ_EINVAL;
    if (n > 0 && (!logits || !target || !scratch_ok(scratch) || !out_loss)) return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    hipStream_t s = (hipStream_t)stream;
    const Geometry rows = wave_per_row(n, LOSS_WAVES);
    launch_bs_unchecked(bs, k_own_rows<8>, k_own_rows<6>, rows.grid, rows.block, s, n, logits,
                        target, weight, L.level[0], out_row);
    for (int k = 0; k < L.levels; ++k) {
        double* dst = k + 1 < L.levels ? L.level[k + 1] : nullptr;
        hipLaunchKernelGGL(k_loss_reduce, dim3(L.count[k + 1]), dim3(RED_THREADS), 0, s,
                           L.count[k], (const double*)L.level[k], dst, 1.0, 0.0, L.hdr, out_loss);
    }
    if (!grad_logits) return last_launch();
    return launch_bs(bs, k_own_grads<8>, k_own_grads<6>, rows.grid, rows.block, s, n, logits,
                     target, (const double*)L.level[0], (const double*)L.hdr, grad_logits);
}

extern "C" int64_t rvz_loss_scratch_size(int32_t bs, int32_t n) {
    return Layout(bs, n, nullptr).total;
}

extern "C" int rvz_policy_value_loss(int32_t bs, int32_t n, const float* logits,
                                     const float* value, const float* policy_target,
                                     const float* value_target, const float* weight,
                                     double policy_weight, double value_weight, void* scratch,
                                     double* out_loss, double* out_row, float* grad_logits,
                                     float* grad_value, void* stream) {
    const Layout L(bs, n, scratch);
    if (L.total < 0) return RVZ_EINVAL;
    if (!(policy_weight >= 0.0 && policy_weight <= DBL_MAX) ||
        !(value_weight >= 0.0 && value_weight <= DBL_MAX))
        return RVZ_EINVAL;
    if (n > 0 && (!logits || !value || !policy_target || !value_target || !scratch_ok(scratch) ||
                  !out_loss || (grad_logits == nullptr) != (grad_value == nullptr)))
        return RVZ_EINVAL;
    if (n == 0) return RVZ_OK;
    hipStream_t s = (hipStream_t)stream;
    const Geometry rows = wave_per_row(n, LOSS_WAVES);

    launch_bs_unchecked(bs, k_loss_rows<8>, k_loss_rows<6>, rows.grid, rows.block, s, n, logits,
                        value, policy_target, value_target, weight, L.aux, L.level[0], out_row);
    for (int k = 0; k < L.levels; ++k) {
        double* dst = k + 1 < L.levels ? L.level[k + 1] : nullptr;
        hipLaunchKernelGGL(k_loss_reduce, dim3(L.count[k + 1]), dim3(RED_THREADS), 0, s,
                           L.count[k], (const double*)L.level[k], dst, policy_weight, value_weight,
                           L.hdr, out_loss);
    }
    if (!grad_logits) return last_launch();
    // the last launch: its error return answers for all of them
    return launch_bs(bs, k_loss_grads<8>, k_loss_grads<6>, rows.grid, rows.block, s, n, logits,
                     value, policy_target, value_target, (const double*)L.aux,
                     (const double*)L.level[0], (const double*)L.hdr, policy_weight, value_weight,
                     grad_logits, grad_value);
}
