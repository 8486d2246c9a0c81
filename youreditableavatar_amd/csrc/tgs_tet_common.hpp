// tgs_tet_common.hpp -- what the kernels over tetrahedral grids share (tgs_marching_tets.hip, tgs_tet_grid.hip): the workgroup scan and the
// in-place exclusive scan over uint32 built on it, a tetrahedron's row load and range check, the sort of one vertex's run by one lane and the
// binary search in a sorted run.  One copy; every kernel here is `static`, so each translation unit that includes the header has its own.
#pragma once
#include "tgs_device.hpp"

namespace tgs {

constexpr int MT_BLOCK = 256;
constexpr int MT_SCAN_ITEMS = 8;
constexpr int MT_SCAN_TILE = MT_BLOCK * MT_SCAN_ITEMS;                  // elements one workgroup scans

__host__ __device__ inline size_t mt_scan_scratch(size_t n)
{
    size_t s = 0;
    while (n > (size_t)MT_SCAN_TILE) { n = (n + MT_SCAN_TILE - 1) / MT_SCAN_TILE; s += (n + 63) & ~(size_t)63; }
    return s + 64;
}
__host__ __device__ inline size_t mt_blocks(size_t F) { return (F + MT_BLOCK - 1) / MT_BLOCK; }

#ifdef __HIPCC__
// exclusive scan over the workgroup's 256 lanes; total: the workgroup's sum.  lds: 4 words.
__device__ __forceinline__ uint32_t mt_block_escan(uint32_t v, uint32_t& total, uint32_t* lds)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t inc = wave_iscan_u32(v, lane);
    if (lane == 63) lds[wv] = inc;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < MT_BLOCK / 64; k++) { const uint32_t s = lds[k]; base += k < wv ? s : 0u; total += s; }
    __syncthreads();
    return base + inc - v;
}

// ---- exclusive scan of uint32 in place: workgroup sums, their scan (recursively), then every workgroup on its own tile ----
static __global__ __launch_bounds__(MT_BLOCK) void k_mt_scan_sums(const uint32_t* __restrict__ data, size_t n, uint32_t* __restrict__ sums)
{
    __shared__ uint32_t lds[4];
    const size_t first = (size_t)blockIdx.x * MT_SCAN_TILE + (size_t)threadIdx.x * MT_SCAN_ITEMS;
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < MT_SCAN_ITEMS; k++) s += first + k < n ? data[first + k] : 0u;
    uint32_t total;
    mt_block_escan(s, total, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
static __global__ __launch_bounds__(MT_BLOCK) void k_mt_scan_tile(uint32_t* __restrict__ data, size_t n, const uint32_t* __restrict__ sums, long long* __restrict__ total_out)
{
    __shared__ uint32_t lds[4];
    const size_t first = (size_t)blockIdx.x * MT_SCAN_TILE + (size_t)threadIdx.x * MT_SCAN_ITEMS;
    uint32_t v[MT_SCAN_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < MT_SCAN_ITEMS; k++) { v[k] = first + k < n ? data[first + k] : 0u; s += v[k]; }
    uint32_t total;
    uint32_t at = mt_block_escan(s, total, lds) + (sums ? sums[blockIdx.x] : 0u);
#pragma unroll
    for (int k = 0; k < MT_SCAN_ITEMS; k++) { if (first + k < n) data[first + k] = at; at += v[k]; }
    if (total_out && threadIdx.x == 0) *total_out = (long long)total;    // (only the one-workgroup launch at the top is given total_out)
}

template <typename Idx>
__device__ __forceinline__ void mt_load_tet(const Idx* __restrict__ tet, size_t f, long long t[4])
{
    if constexpr (sizeof(Idx) == 4) {
        const int4 r = reinterpret_cast<const int4*>(tet)[f];
        t[0] = r.x; t[1] = r.y; t[2] = r.z; t[3] = r.w;
    } else {
        const longlong2 r0 = reinterpret_cast<const longlong2*>(tet)[2 * f], r1 = reinterpret_cast<const longlong2*>(tet)[2 * f + 1];
        t[0] = r0.x; t[1] = r0.y; t[2] = r1.x; t[3] = r1.y;
    }
}
__device__ __forceinline__ bool mt_in_range(const long long t[4], int N)
{
    return (unsigned long long)t[0] < (unsigned long long)N && (unsigned long long)t[1] < (unsigned long long)N &&
           (unsigned long long)t[2] < (unsigned long long)N && (unsigned long long)t[3] < (unsigned long long)N;
}

// one lane sorts the run keys[stride * lo], keys[stride * (lo + 1)], ... keys[stride * (hi - 1)] ascending (insertion: the runs are short)
template <typename T>
__device__ __forceinline__ void mt_sort_run(T* __restrict__ keys, int stride, long long lo, long long hi)
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
__device__ __forceinline__ long long mt_sort_unique_run(T* __restrict__ keys, long long lo, long long hi)
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
__device__ __forceinline__ long long mt_search_run(const T* __restrict__ keys, int stride, long long lo, long long hi, long long b)
{
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        const long long have = (long long)keys[stride * mid];
        if (have == b) return mid;
        if (have < b) lo = mid + 1; else hi = mid;
    }
    return -1;
}

// exclusive scan of data[0 .. n) in place on `st`; the sum goes to *total_out (device) if given
static void mt_scan(hipStream_t st, uint32_t* data, size_t n, uint32_t* scratch, long long* total_out)
{
    if (n <= (size_t)MT_SCAN_TILE) {
        hipLaunchKernelGGL(k_mt_scan_tile, dim3(1), dim3(MT_BLOCK), 0, st, data, n, (const uint32_t*)nullptr, total_out);
        return;
    }
    const size_t nb = (n + MT_SCAN_TILE - 1) / MT_SCAN_TILE;
    hipLaunchKernelGGL(k_mt_scan_sums, dim3((unsigned)nb), dim3(MT_BLOCK), 0, st, (const uint32_t*)data, n, scratch);
    mt_scan(st, scratch, nb, scratch + ((nb + 63) & ~(size_t)63), total_out);
    hipLaunchKernelGGL(k_mt_scan_tile, dim3((unsigned)nb), dim3(MT_BLOCK), 0, st, data, n, (const uint32_t*)scratch, (long long*)nullptr);
}

static inline dim3 mt_grid(size_t n) { return dim3((unsigned)((n + MT_BLOCK - 1) / MT_BLOCK)); }
static inline bool mt_aligned(const void* tet) { return ((uintptr_t)tet & 15u) == 0; }              // rows are loaded as 16-byte vectors
#endif

}  // namespace tgs
