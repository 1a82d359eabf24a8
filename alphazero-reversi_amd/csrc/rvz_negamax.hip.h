// rvz_negamax.hip.h — what the two negamax lane machines, rvz_solve.hip (solve_rows<BS, MODE>)
// and rvz_alphabeta.hip (k_alphabeta<BS>), have in common around their loops: the launch
// geometry, the size of the LDS frame stack and its bound, the per-call row counter with the
// kernel that zeroes it, and what the host does before a launch (the launch itself is
// rvz_host.hip.h's launch_bs on dim3(wgs) x dim3(NM_THREADS)).
//
// Shape: one position per LANE. A batch is tens of thousands of small, unequal trees with at
// most ~12 root moves each, so a wave per position would idle most lanes; here the 64 lanes of a
// wave step one explicit-stack state machine in lockstep, each on its own position. Lanes are
// persistent: a lane whose row is done takes the next row index from a device counter in the
// same loop iteration, so a wave stays full until the batch drains; the grid is sized from the
// CU count. Nothing a row computes depends on which lane, wave or launch it landed in.
//
// Per lane, in registers: the current node and the row's bookkeeping. Per lane, in LDS: one frame
// per ply above the current node, [depth][field][lane] in dwords, so a wave's access to one
// field of one depth covers 64 consecutive banks: field f of depth d of the lane whose base is
// `my` (the stack plus the lane's index) is my[(d * FIELDS + f) * NM_THREADS]. No recursion and
// no run-time-indexed register array: no scratch.
//
// NOT here: the steps of the loop itself (row intake, the pass-root ladder, fold, the return to
// the parent, the descent). They were shared too, as forced-inline functions on a struct of the
// lane's registers, and every row's score, move and node count stayed equal, with fewer
// instructions and VGPRs in every kernel. The solver's times stayed inside its spread; but
// rvz_alphabeta at depth 8 took 74 s where the separate loops take 64 s, in both orders of an
// alternating run, and with only the once-per-row steps shared (lane struct, intake, ladder,
// root opening) depth 7 still took 72 s against 61 s (profiles/README.md, neg01_steps_* and
// neg02_screen_*; DESIGN.md, "One header around two lane machines"). At 2 waves per SIMD these
// loops are bound by the latency of one long dependent chain per iteration, and the compiler's
// register assignment along k_alphabeta's moved with the shape of source that is not even on
// that chain. A step only the solver used would not be shared, so each loop keeps its own text,
// and a fix to one of those steps still has to be made in both files.
//
// Everything with storage (the counters, the zeroing kernel, the host's slot counter) has
// internal linkage: each translation unit that includes this file has its own, so calls of the
// solver and of alpha-beta in flight at once never share a counter.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/rvz.h"
#include "rvz_host.hip.h"
#include "rvz_rules.hip.h"

namespace rvz {
namespace {

constexpr int NM_THREADS = 128;                    // 2 waves per workgroup
constexpr int NM_WG_PER_CU = 4;                    // 8 waves per CU by LDS
constexpr int NM_SLOTS = 32;                       // row counters: calls in flight at once

// the dwords of a workgroup's stack: FRAMES frames of FIELDS dwords per lane
template <int FRAMES, int FIELDS>
constexpr int stack_dwords() {
    static_assert(FRAMES * FIELDS * NM_THREADS * 4 * NM_WG_PER_CU <= 160 * 1024,
                  "2 waves per SIMD must fit in the CU's LDS");
    return FRAMES * FIELDS * NM_THREADS;
}

// the next row index of each call in flight; zeroed on the call's stream by k_negamax_zero
__device__ unsigned int g_next_row[NM_SLOTS];

__global__ void k_negamax_zero(int slot) { g_next_row[slot] = 0u; }

__device__ __forceinline__ unsigned next_row(int slot) { return atomicAdd(&g_next_row[slot], 1u); }

std::atomic<unsigned> g_slot{0};

// Before a launch over `units` > 0 units of work (rows or tasks): takes a counter slot, zeroes
// it on the stream and returns the grid size, or RVZ_EHIP.
inline int negamax_prepare(int64_t units, hipStream_t s, int* slot) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0)
        return RVZ_EHIP;
    *slot = (int)(g_slot.fetch_add(1u, std::memory_order_relaxed) % NM_SLOTS);
    hipLaunchKernelGGL(k_negamax_zero, dim3(1), dim3(1), 0, s, *slot);
    const int64_t need = (units + NM_THREADS - 1) / NM_THREADS;
    const int wgs = cus * NM_WG_PER_CU;
    return need < wgs ? (int)need : wgs;
}

}  // namespace
}  // namespace rvz
