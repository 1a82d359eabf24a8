// rvz_replay.hip — a training minibatch drawn from a compact ring of records (rvz_replay_batch;
// contract in include/rvz.h).
//
// The ring holds a record as (mover bitboard, opponent bitboard, policy row, value): 280 B on 8x8
// against the 1028 B of its expanded planes and policy. k_replay_batch: one wavefront per output
// row, lane = output square. The wave draws its record and symmetry from one Philox4x32-10 block
// keyed by (seed, step, row), so the draw is wave-uniform and a pure function of those three;
// then it is k_training_rows' wave (rvz_symmetry.hip.h): three ballots give the image bitboards,
// one cross-lane read moves the policy, the planes go out as float4 and the policy as dwords,
// every output byte once. Nothing is recomputed and no table lives in memory.
//
// The draw of the logical row: i = mulhi(x.0, live), the multiply-high of a uniform 32-bit word.
// Of the 2^32 words, floor(2^32 / live) or one more map to each i, so a row's probability is
// within 2^-32 of 1 / live: a relative bias of at most live / 2^32 (0.05% at 2^21 rows).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rvz.h"
#include "rvz_host.hip.h"
#include "rvz_philox.hip.h"
#include "rvz_rules.hip.h"
#include "rvz_symmetry.hip.h"

namespace {

using namespace rvz;

template <int BS>
__global__ __launch_bounds__(SYM_THREADS) void k_replay_batch(
    int capacity, const uint64_t* __restrict__ mover, const uint64_t* __restrict__ opponent,
    const float* __restrict__ policy, const float* __restrict__ value, int start, int live, int nb,
    const int32_t* __restrict__ idx, const int32_t* __restrict__ sym, int random_sym, uint32_t key0,
    uint32_t key1, uint32_t step0, uint32_t step1, float* __restrict__ out_states,
    float* __restrict__ out_policy, float* __restrict__ out_value, int32_t* __restrict__ out_slot,
    int32_t* __restrict__ out_sym) {
    constexpr int NSQ = Geo<BS>::NSQ, NPOL = Geo<BS>::NPOL;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int stride = gridDim.x * SYM_WAVES;       // nb * NPOL fits int32, so r + stride does too
    for (int r = blockIdx.x * SYM_WAVES + wave; r < nb; r += stride) {  // wave-uniform trip count
        const uint4 x = philox4x32_10(key0, key1, (uint32_t)r, step0, step1, 0u);
        const int i = idx ? idx[r] : (int)__umulhi(x.x, (uint32_t)live);
        const int k = sym ? sym[r] : (random_sym ? (int)(x.y & 7u) : 0);
        const bool in = i >= 0 && i < live;
        const int64_t at = (int64_t)start + (in ? i : 0);              // below 2 * capacity
        const int slot = (int)(at >= capacity ? at - capacity : at);
        const bool ok = in && k >= 0 && k < 8;
        uint64_t P = 0ull, O = 0ull;
        float pv = 0.0f, pass = 0.0f, v = 0.0f;
        if (ok) {                                                       // wave-uniform
            P = mover[slot];
            O = opponent[slot];
            const float* prow = policy + (size_t)slot * NPOL;           // capacity * NPOL: 64-bit
            pv = lane < NSQ ? prow[lane] : 0.0f;
            pass = prow[NSQ];
            v = value[slot];
        }
        const uint64_t V = legal<BS>(P, O);
        write_image<BS>(lane, P, O, V, pv, pass, ok ? k : -1, (size_t)r, out_states, out_policy,
                        nullptr);
        if (lane == 0) {
            out_value[r] = v;
            out_slot[r] = in ? slot : -1;
            out_sym[r] = ok ? k : -1;
        }
    }
}

}  // namespace

extern "C" int rvz_replay_batch(int32_t bs, int32_t capacity, const uint64_t* mover,
                                const uint64_t* opponent, const float* policy, const float* value,
                                int32_t start, int32_t live, int32_t nb, const int32_t* idx,
                                const int32_t* sym, int32_t random_sym, uint64_t seed,
                                uint64_t step, float* out_states, float* out_policy,
                                float* out_value, int32_t* out_slot, int32_t* out_sym,
                                void* stream) {
    if (!board_ok(bs) || capacity < 1 || live < 1 || live > capacity || start < 0 ||
        start >= capacity || nb < 0)
        return RVZ_EINVAL;
    if ((int64_t)nb * (bs * bs + 1) > INT32_MAX) return RVZ_EINVAL;
    if (nb > 0 && (!mover || !opponent || !policy || !value || !out_states || !out_policy ||
                   !out_value || !out_slot || !out_sym ||
                   ((uintptr_t)out_states & 15u) != 0))                 // float4 stores
        return RVZ_EINVAL;
    if (nb == 0) return RVZ_OK;
    return launch_bs(bs, k_replay_batch<8>, k_replay_batch<6>,
                     dim3(sym_blocks_for(nb, SYM_WAVES)), dim3(SYM_THREADS), (hipStream_t)stream,
                     capacity, mover, opponent, policy, value, start, live, nb, idx, sym,
                     random_sym, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step,
                     (uint32_t)(step >> 32), out_states, out_policy, out_value, out_slot, out_sym);
}
