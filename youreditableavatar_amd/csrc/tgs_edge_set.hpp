// tgs_edge_set.hpp -- the deduplicating set of undirected vertex pairs of the geometry stage (tgs_mesh_geom.hip, tgs_marching_tets.hip,
// tgs_mesh_aa.hip): an open-addressing table keyed by (min << 32 | max), integer CAS, linear probing; and the way from the table to the sorted
// edge list: every key into its min vertex's run through a cursor, then one lane per vertex sorts its run by the max index, so the pairs stand
// in ascending (min, max) order whatever the slots and the cursors did.  The hash only dedupes: no output reads a slot number.  The capacity
// (a power of two, never full) is the including file's rule.  One copy; every kernel here is `static`, so each translation unit that includes
// the header has its own, used or not: a file that reads its table in place and sends nothing to runs (tgs_mesh_aa.hip) defines
// TGS_EDGE_SET_TABLE_ONLY and gets the table alone.
#pragma once
#include "tgs_device.hpp"
#ifndef TGS_EDGE_SET_TABLE_ONLY
#include "tgs_runs.hpp"
#endif

namespace tgs {

constexpr unsigned long long EDGE_EMPTY = ~0ull;                        // no key: min <= max < 2^31 never gives all ones
constexpr size_t EDGE_ABSENT = ~(size_t)0;                              // no slot

#ifdef __HIPCC__
__device__ __forceinline__ unsigned long long edge_key(long long lo, long long hi)            // 0 <= lo <= hi < 2^31
{
    return ((unsigned long long)lo << 32) | (unsigned long long)hi;
}
__device__ __forceinline__ unsigned long long edge_hash(unsigned long long k)     // (splitmix64's finaliser)
{
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    return k ^ (k >> 31);
}
// the slot that holds `key` after the call; claimed: this call put it there, so of all the calls with one key exactly one sees true
__device__ __forceinline__ size_t edge_insert(unsigned long long* __restrict__ keys, size_t cap, unsigned long long key, bool& claimed)
{
    size_t slot = (size_t)edge_hash(key) & (cap - 1);
    for (size_t probe = 0; probe < cap; probe++) {                      // (the table is never full: it ends at the key or at a free slot)
        const unsigned long long prev = atomicCAS(&keys[slot], EDGE_EMPTY, key);
        if (prev == EDGE_EMPTY || prev == key) { claimed = prev == EDGE_EMPTY; return slot; }
        slot = (slot + 1) & (cap - 1);
    }
    claimed = false;
    return EDGE_ABSENT;
}
// the slot that holds `key`, EDGE_ABSENT if none does (plain loads: for a launch after the inserts)
__device__ __forceinline__ size_t edge_find(const unsigned long long* __restrict__ keys, size_t cap, unsigned long long key)
{
    size_t slot = (size_t)edge_hash(key) & (cap - 1);
    for (size_t probe = 0; probe < cap; probe++) {
        const unsigned long long have = keys[slot];
        if (have == key) return slot;
        if (have == EDGE_EMPTY) break;
        slot = (slot + 1) & (cap - 1);
    }
    return EDGE_ABSENT;
}

#ifndef TGS_EDGE_SET_TABLE_ONLY
// one lane per slot: the key goes to its min vertex's run as the int64 pair (min, max), through the cursor end[min], which starts at the
// run's start (the scanned counts of the claims) and ends at its end
static __global__ __launch_bounds__(RUN_BLOCK) void k_edge_fill(int V, long long E, size_t cap, const unsigned long long* __restrict__ keys, uint32_t* __restrict__ end,
                                                                long long* __restrict__ pairs)
{
    const size_t s = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (s >= cap) return;
    const unsigned long long key = keys[s];
    if (key == EDGE_EMPTY) return;
    const long long a = (long long)(key >> 32), b = (long long)(key & 0xffffffffull);
    if (a >= V) return;
    const long long p = atomicAdd(&end[a], 1u);
    if (p < E) { pairs[2 * p] = a; pairs[2 * p + 1] = b; }
}
// end[v] is now the END of v's run (the start of v + 1's); one lane per vertex sorts its run by the max index
static __global__ __launch_bounds__(RUN_BLOCK) void k_edge_sort(int V, long long E, const uint32_t* __restrict__ end, long long* __restrict__ pairs)
{
    const size_t v = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (v >= (size_t)V) return;
    const Run run = run_bounds(end, v, (size_t)E);
    run_sort(pairs + 1, 2, (long long)run.lo, (long long)run.hi);
}
#endif
#endif

}  // namespace tgs
