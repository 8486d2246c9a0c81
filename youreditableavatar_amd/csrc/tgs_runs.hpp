// tgs_runs.hpp -- runs per vertex, as the geometry stage's kernels build and read them (tgs_mesh_geom.hip, tgs_marching_tets.hip,
// tgs_tet_grid.hip; tgs_edge_set.hpp): a count per vertex, the in-place exclusive scan over uint32 that turns the counts into the runs' starts
// (after a fill through cursors: their ends), the clamped bounds of one vertex's run, the sort of a run by one lane and the binary search in a
// sorted run.  One copy; every kernel here is `static`, so each translation unit that includes the header has its own.
#pragma once
#include "tgs_device.hpp"

namespace tgs {

constexpr int RUN_BLOCK = 256;
constexpr int RUN_SCAN_ITEMS = 8;
constexpr int RUN_SCAN_TILE = RUN_BLOCK * RUN_SCAN_ITEMS;               // elements one workgroup scans

__host__ __device__ inline size_t run_scan_scratch(size_t n)
{
    size_t s = 0;
    while (n > (size_t)RUN_SCAN_TILE) { n = (n + RUN_SCAN_TILE - 1) / RUN_SCAN_TILE; s += (n + 63) & ~(size_t)63; }
    return s + 64;
}
__host__ __device__ inline size_t run_blocks(size_t n) { return (n + RUN_BLOCK - 1) / RUN_BLOCK; }

#ifdef __HIPCC__
// exclusive scan over the workgroup's 256 lanes; total: the workgroup's sum.  lds: 4 words.
__device__ __forceinline__ uint32_t run_block_escan(uint32_t v, uint32_t& total, uint32_t* lds)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t inc = wave_iscan_u32(v, lane);
    if (lane == 63) lds[wv] = inc;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < RUN_BLOCK / 64; k++) { const uint32_t s = lds[k]; base += k < wv ? s : 0u; total += s; }
    __syncthreads();
    return base + inc - v;
}

// ---- exclusive scan of uint32 in place: workgroup sums, their scan (recursively), then every workgroup on its own tile ----
static __global__ __launch_bounds__(RUN_BLOCK) void k_run_scan_sums(const uint32_t* __restrict__ data, size_t n, uint32_t* __restrict__ sums)
{
    __shared__ uint32_t lds[4];
    const size_t first = (size_t)blockIdx.x * RUN_SCAN_TILE + (size_t)threadIdx.x * RUN_SCAN_ITEMS;
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < RUN_SCAN_ITEMS; k++) s += first + k < n ? data[first + k] : 0u;
    uint32_t total;
    run_block_escan(s, total, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
static __global__ __launch_bounds__(RUN_BLOCK) void k_run_scan_tile(uint32_t* __restrict__ data, size_t n, const uint32_t* __restrict__ sums, long long* __restrict__ total_out)
{
    __shared__ uint32_t lds[4];
    const size_t first = (size_t)blockIdx.x * RUN_SCAN_TILE + (size_t)threadIdx.x * RUN_SCAN_ITEMS;
    uint32_t v[RUN_SCAN_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < RUN_SCAN_ITEMS; k++) { v[k] = first + k < n ? data[first + k] : 0u; s += v[k]; }
    uint32_t total;
    uint32_t at = run_block_escan(s, total, lds) + (sums ? sums[blockIdx.x] : 0u);
#pragma unroll
    for (int k = 0; k < RUN_SCAN_ITEMS; k++) { if (first + k < n) data[first + k] = at; at += v[k]; }
    if (total_out && threadIdx.x == 0) *total_out = (long long)total;    // (only the one-workgroup launch at the top is given total_out)
}

// exclusive scan of data[0 .. n) in place on `st`; the sum goes to *total_out (device) if given
static void run_scan(hipStream_t st, uint32_t* data, size_t n, uint32_t* scratch, long long* total_out)
{
    if (n <= (size_t)RUN_SCAN_TILE) {
        hipLaunchKernelGGL(k_run_scan_tile, dim3(1), dim3(RUN_BLOCK), 0, st, data, n, (const uint32_t*)nullptr, total_out);
        return;
    }
    const size_t nb = (n + RUN_SCAN_TILE - 1) / RUN_SCAN_TILE;
    hipLaunchKernelGGL(k_run_scan_sums, dim3((unsigned)nb), dim3(RUN_BLOCK), 0, st, (const uint32_t*)data, n, scratch);
    run_scan(st, scratch, nb, scratch + ((nb + 63) & ~(size_t)63), total_out);
    hipLaunchKernelGGL(k_run_scan_tile, dim3((unsigned)nb), dim3(RUN_BLOCK), 0, st, data, n, (const uint32_t*)scratch, (long long*)nullptr);
}

static inline dim3 run_grid(size_t n) { return dim3((unsigned)run_blocks(n)); }

// ---- one vertex's run ----
// vertex v's run in an array of run ENDS (a scanned count array after the fill's cursors went over it), clamped to the n entries that exist:
// lo <= hi <= n whatever the array holds
struct Run { size_t lo, hi; };
__device__ __forceinline__ size_t run_start(const uint32_t* __restrict__ end, size_t v) { return v ? (size_t)end[v - 1] : 0; }     // (for a reader that has the run's length from elsewhere)
__device__ __forceinline__ Run run_bounds(const uint32_t* __restrict__ end, size_t v, size_t n)
{
    Run r = {run_start(end, v), (size_t)end[v]};
    if (r.hi > n) r.hi = n;
    if (r.lo > r.hi) r.lo = r.hi;
    return r;
}

// one lane sorts the run keys[stride * lo], keys[stride * (lo + 1)], ... keys[stride * (hi - 1)] ascending (insertion: the runs are short)
template <typename T>
__device__ __forceinline__ void run_sort(T* __restrict__ keys, int stride, long long lo, long long hi)
{
    for (long long i = lo + 1; i < hi; i++) {
        const T b = keys[stride * i];
        long long j = i;
        for (; j > lo && keys[stride * (j - 1)] > b; j--) keys[stride * j] = keys[stride * (j - 1)];
        keys[stride * j] = b;
    }
}
// the same for a run that holds repeats: every key is kept once -> the end of the sorted distinct keys, which stand at the front of the run.
// A key is looked up in the distinct keys before anything moves, so the work is (keys) x (distinct keys), not (keys)^2.
template <typename T>
__device__ __forceinline__ long long run_sort_unique(T* __restrict__ keys, long long lo, long long hi)
{
    long long n = lo;                                                   // [lo, n) is sorted and distinct; n <= i, so nothing unread is overwritten
    for (long long i = lo; i < hi; i++) {
        const T b = keys[i];
        long long j = n;
        while (j > lo && keys[j - 1] > b) j--;
        if (j > lo && keys[j - 1] == b) continue;
        for (long long k = n; k > j; k--) keys[k] = keys[k - 1];
        keys[j] = b;
        n++;
    }
    return n;
}
// the position of b in the sorted run [lo, hi) of keys, -1 if it is not there
template <typename T>
__device__ __forceinline__ long long run_search(const T* __restrict__ keys, int stride, long long lo, long long hi, long long b)
{
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        const long long have = (long long)keys[stride * mid];
        if (have == b) return mid;
        if (have < b) lo = mid + 1; else hi = mid;
    }
    return -1;
}
#endif

}  // namespace tgs
