// rvz_slot_table.hip.h — the last-row-wins slot table of the calls that scatter a batch's rows
// into the replay ring (rvz_priority.hip's rvz_replay_priority, rvz_reanalyse.hip's
// rvz_replay_refresh), written once. A batch can name one slot in several rows; what the
// sequential loop `for r: ring[slot[r]] = row r` leaves is the row with the highest r, and the
// table finds that row without an order between workgroups: a first launch enters
// (slot -> max r) for every valid row, a later launch looks its slot up, and the row whose r the
// table holds is the slot's winner. The key is claimed by an integer compare-and-swap, r by an
// integer atomicMax: where a key lands depends on arrival, what a lookup returns does not.
// The table: key[T] (slot + 1; 0: empty) and val[T] (the highest r + 1 entered under the key),
// uint32 words the caller cleared to 0 in a launch before the first enter; T a power of two with
// T >= 2 * (the rows that can enter), mask = T - 1. No storage here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rvz {

// T for a batch of nb rows: the power of two >= max(2 nb, 64)
inline int64_t slot_table_entries(int32_t nb) {
    int64_t T = 64;
    while (T < 2 * (int64_t)nb) T <<= 1;
    return T;
}

__device__ __forceinline__ uint32_t slot_hash(uint32_t s) {             // murmur3's finaliser
    s ^= s >> 16;
    s *= 0x85ebca6bu;
    s ^= s >> 13;
    s *= 0xc2b2ae35u;
    return s ^ (s >> 16);
}

// row r names slot s (s >= 0): the table's r for s becomes max(its r, r)
__device__ __forceinline__ void slot_table_enter(uint32_t* __restrict__ key,
                                                 uint32_t* __restrict__ val, uint32_t mask, int s,
                                                 int r) {
    const uint32_t want = (uint32_t)s + 1u;
    uint32_t h = slot_hash((uint32_t)s) & mask;
    for (uint32_t tries = 0; tries <= mask; ++tries, h = (h + 1u) & mask) {
        const uint32_t old = atomicCAS(&key[h], 0u, want);             // <= nb keys, T >= 2 nb
        if (old == 0u || old == want) {
            atomicMax(&val[h], (uint32_t)r + 1u);
            break;
        }
    }
}

// in a launch behind every enter: 1 if r is the highest row entered under slot s, else 0 (a later
// row superseded it, or s was never entered)
__device__ __forceinline__ int slot_table_wins(const uint32_t* __restrict__ key,
                                               const uint32_t* __restrict__ val, uint32_t mask,
                                               int s, int r) {
    const uint32_t want = (uint32_t)s + 1u;
    uint32_t h = slot_hash((uint32_t)s) & mask;
    for (uint32_t tries = 0; tries <= mask; ++tries, h = (h + 1u) & mask) {
        const uint32_t k = key[h];
        if (k == want) return val[h] == (uint32_t)r + 1u ? 1 : 0;
        if (k == 0u) break;
    }
    return 0;
}

}  // namespace rvz
