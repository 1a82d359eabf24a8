// rvz_priority.hip — prioritized replay's two missing pieces (rvz_replay_is_weight,
// rvz_replay_priority; contract in include/rvz.h): the importance weights of a drawn batch from its
// out_prob, and the batch's loss rows written back into the ring as sampling weights.
//
// All arithmetic is float64, IEEE without contraction, and the power is rvz_pow::pow_cr (correctly
// rounded), so every output is a pure function of the inputs that a host reference reproduces bit
// for bit. Nothing floating-point is ever reduced across rows: the two reductions (the smallest
// probability, the largest priority) run on the bit patterns of non-negative floats, whose
// unsigned order is the floats' own, so they depend on no order.
//
// rvz_replay_is_weight, two launches: k_isw_min, one workgroup, reduces the bit patterns of the
// valid probabilities to their minimum (a stride over prob, a shuffle tree, the 16 waves through
// LDS) and leaves it in the scratch; k_isw_weight, a thread per row, the power.
//
// rvz_replay_priority, three launches: k_pri_clear empties a hash table of T >= 2 nb entries in
// the scratch; k_pri_rows, a thread per row, computes the row's priority, keeps it in the
// scratch and, for a valid row, enters (slot -> max r) into the table (the key claimed by an
// integer compare-and-swap, r by an integer atomicMax: where a key lands depends on arrival, what
// a lookup returns does not; rvz_slot_table.hip.h, shared with rvz_reanalyse.hip); k_pri_write, a thread per row, looks its slot up, and the row whose
// r the table holds is the slot's winner and stores the weight. No workgroup waits on another.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rvz.h"
#include "rvz_host.hip.h"
#include "rvz_pow.hip.h"
#include "rvz_slot_table.hip.h"
#include "rvz_wave.hip.h"

namespace {

using namespace rvz;

constexpr int ISW_THREADS = 1024;                // k_isw_min's one workgroup: 16 waves
constexpr uint32_t NO_PROB = 0x7f800000u;        // +inf's bits: above every valid probability
constexpr int PRI_THREADS = 256;
constexpr int PRI_HEAD = 16;                     // the scratch's header bytes: word 0 the max bits
constexpr int32_t PRI_MAX_NB = 1 << 30;          // T = 2^31 entries at most
constexpr double PRI_MIN_FLOOR = 0x1p-16, PRI_MAX_CAP = 65536.0;

// a drawn row's probability counts iff its slot is one and it is finite and above 0
__device__ __forceinline__ bool prob_ok(float p, int slot) {
    return slot >= 0 && p > 0.0f && p < INFINITY;                       // NaN fails both
}

__global__ __launch_bounds__(ISW_THREADS) void k_isw_min(int nb, const float* __restrict__ prob,
                                                         const int32_t* __restrict__ slot,
                                                         uint32_t* __restrict__ min_bits,
                                                         float* __restrict__ out_min_prob) {
    __shared__ uint32_t part[ISW_THREADS / 64];
    uint32_t m = NO_PROB;
    for (int r = threadIdx.x; r < nb; r += ISW_THREADS) {
        const float p = prob[r];
        if (prob_ok(p, slot[r])) {
            const uint32_t b = __float_as_uint(p);
            m = b < m ? b : m;
        }
    }
    m = block_reduce<1>(&m, threadIdx.x & 63, threadIdx.x >> 6, ISW_THREADS / 64, part,
                        [](uint32_t a, uint32_t b) { return b < a ? b : a; });
    if (threadIdx.x == 0) {
        *min_bits = m;
        if (out_min_prob) *out_min_prob = m == NO_PROB ? 0.0f : __uint_as_float(m);
    }
}

__global__ __launch_bounds__(PRI_THREADS) void k_isw_weight(int nb, const float* __restrict__ prob,
                                                            const int32_t* __restrict__ slot,
                                                            double beta,
                                                            const uint32_t* __restrict__ min_bits,
                                                            float* __restrict__ out_weight) {
    const int r = blockIdx.x * PRI_THREADS + threadIdx.x;
    if (r >= nb) return;
    const float p = prob[r];
    float w = 0.0f;
    if (prob_ok(p, slot[r]))                     // then *min_bits is a probability, at most p
        w = (float)rvz_pow::pow_cr((double)__uint_as_float(*min_bits) / (double)p, beta);
    out_weight[r] = w;
}

// ---------------------------------------------------------------- the priorities
// the scratch: the header, pri [nb], the table's key [T] and, right behind it, val [T]; T: the
// power of two >= max(2 nb, 64)
struct Layout {
    int64_t T, bytes;
    uint32_t *head, *key, *val;
    float* pri;
    Layout(int32_t nb, void* scratch) : T(slot_table_entries(nb)) {
        Carver c(scratch);
        head = c.take<uint32_t>(PRI_HEAD / 4);
        pri = c.take<float>(nb);
        key = c.take<uint32_t>(T);
        val = c.take<uint32_t>(T);
        bytes = c.at;
    }
};

__global__ __launch_bounds__(PRI_THREADS) void k_pri_clear(uint32_t* __restrict__ head,
                                                           uint32_t* __restrict__ table,
                                                           int64_t words) {
    const int64_t stride = (int64_t)gridDim.x * PRI_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * PRI_THREADS + threadIdx.x; i < words; i += stride)
        table[i] = 0u;
    if (blockIdx.x == 0 && threadIdx.x < PRI_HEAD / 4) head[threadIdx.x] = 0u;
}

// table: key[T] (slot + 1; 0: empty) then val[T] (the highest r + 1 entered under the key)
__global__ __launch_bounds__(PRI_THREADS) void k_pri_rows(
    int capacity, int nb, const int32_t* __restrict__ slot, const double* __restrict__ row,
    double policy_coef, double value_coef, int subtract_entropy, double alpha, double floor_,
    double cap, uint32_t* __restrict__ head, float* __restrict__ pri, uint32_t* __restrict__ key,
    uint32_t* __restrict__ val, uint32_t mask) {
    const int r = blockIdx.x * PRI_THREADS + threadIdx.x;
    uint32_t bits = 0u;
    if (r < nb) {
        const int s = slot[r];
        const double Lp = row[3 * (int64_t)r], Lv = row[3 * (int64_t)r + 1],
                     H = row[3 * (int64_t)r + 2];
        const double d = Lp - H;
        const double k = subtract_entropy ? (d > 0.0 ? d : 0.0) : Lp;
        const double a = policy_coef * k, b = value_coef * Lv;
        const double e = a + b;
        const bool valid = s >= 0 && s < capacity && isfinite(Lp) && isfinite(Lv) &&
                           isfinite(H) && Lp >= 0.0 && Lv >= 0.0 && isfinite(e);
        float p = 0.0f;
        if (valid) {
            double x = rvz_pow::pow_cr(e, alpha);
            x = x > floor_ ? x : floor_;
            x = x < cap ? x : cap;
            p = (float)x;
            bits = __float_as_uint(p);
            slot_table_enter(key, val, mask, s, r);
        }
        pri[r] = p;                              // 0: an invalid row (a valid one is >= floor > 0)
    }
    bits = wave_reduce(bits, [](uint32_t a, uint32_t b) { return b > a ? b : a; });
    if ((threadIdx.x & 63) == 0 && bits) atomicMax(&head[0], bits);
}

__global__ __launch_bounds__(PRI_THREADS) void k_pri_write(
    int nb, const int32_t* __restrict__ slot, const uint32_t* __restrict__ head,
    const float* __restrict__ pri, const uint32_t* __restrict__ key,
    const uint32_t* __restrict__ val, uint32_t mask, float* __restrict__ weight,
    float* __restrict__ max_priority, float* __restrict__ out_priority,
    int32_t* __restrict__ out_state) {
    const int r = blockIdx.x * PRI_THREADS + threadIdx.x;
    if (r == 0 && max_priority) {
        const uint32_t held = __float_as_uint(*max_priority), mine = head[0];
        *max_priority = __uint_as_float(mine > held ? mine : held);
    }
    if (r >= nb) return;
    const float p = pri[r];
    int state = -1;
    if (p > 0.0f) {                              // valid: its slot is in range and in the table
        const int s = slot[r];
        state = slot_table_wins(key, val, mask, s, r);     // k_pri_rows entered every valid slot
        if (state == 1) weight[s] = p;
    }
    if (out_priority) out_priority[r] = p;
    if (out_state) out_state[r] = state;
}

}  // namespace

extern "C" int64_t rvz_replay_is_weight_scratch_size(int32_t nb) { return nb < 0 ? -1 : 16; }

extern "C" int rvz_replay_is_weight(int32_t nb, const float* prob, const int32_t* slot,
                                    double beta, void* scratch, float* out_weight,
                                    float* out_min_prob, void* stream) {
    if (nb < 0 || !(beta >= 0.0 && beta <= 1.0)) return RVZ_EINVAL;     // NaN fails
    if (nb == 0) return RVZ_OK;
    if (!prob || !slot || !out_weight || !scratch_ok(scratch)) return RVZ_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* min_bits = (uint32_t*)scratch;
    hipLaunchKernelGGL(k_isw_min, dim3(1), dim3(ISW_THREADS), 0, s, nb, prob, slot, min_bits,
                       out_min_prob);
    const Geometry g = thread_per_row(nb);
    hipLaunchKernelGGL(k_isw_weight, g.grid, g.block, 0, s, nb, prob, slot, beta,
                       (const uint32_t*)min_bits, out_weight);
    return last_launch();
}

extern "C" int64_t rvz_replay_priority_scratch_size(int32_t nb) {
    if (nb < 0 || nb > PRI_MAX_NB) return -1;
    return Layout(nb, nullptr).bytes;
}

extern "C" int rvz_replay_priority(int32_t capacity, float* weight, int32_t nb,
                                   const int32_t* slot, const double* row, double policy_coef,
                                   double value_coef, int32_t subtract_entropy, double alpha,
                                   double floor_, double cap, void* scratch, float* max_priority,
                                   float* out_priority, int32_t* out_state, void* stream) {
    if (capacity < 1 || nb < 0 || nb > PRI_MAX_NB) return RVZ_EINVAL;
    if (!(policy_coef >= 0.0 && policy_coef < INFINITY) ||
        !(value_coef >= 0.0 && value_coef < INFINITY) || !(alpha >= 0.0 && alpha <= 1.0) ||
        !(floor_ >= PRI_MIN_FLOOR && floor_ <= cap && cap <= PRI_MAX_CAP))
        return RVZ_EINVAL;
    if (nb == 0) return RVZ_OK;
    if (!weight || !slot || !row || !scratch_ok(scratch)) return RVZ_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const Layout l(nb, scratch);
    const uint32_t mask = (uint32_t)(l.T - 1);
    const Geometry c = strided(2 * l.T, PRI_THREADS, PRI_THREADS);
    hipLaunchKernelGGL(k_pri_clear, c.grid, c.block, 0, s, l.head, l.key, 2 * l.T);
    const Geometry g = thread_per_row(nb);
    hipLaunchKernelGGL(k_pri_rows, g.grid, g.block, 0, s, capacity, nb, slot, row, policy_coef,
                       value_coef, subtract_entropy, alpha, floor_, cap, l.head, l.pri, l.key,
                       l.val, mask);
    hipLaunchKernelGGL(k_pri_write, g.grid, g.block, 0, s, nb, slot, (const uint32_t*)l.head,
                       (const float*)l.pri, (const uint32_t*)l.key, (const uint32_t*)l.val, mask,
                       weight, max_priority, out_priority, out_state);
    return last_launch();
}
