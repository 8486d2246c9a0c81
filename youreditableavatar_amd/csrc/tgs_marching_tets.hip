// tgs_marching_tets.hip -- marching tetrahedra for the geometry stage (tetgs_spatial/models/isosurface.py :112-184, `_forward`; the two
// marching_tetrahedra calls of models/geometry/base.py :350, :465), forward and backward, for gfx950.  Plain HIP, wave64.  Integer atomics only
// (the dedupe's CAS, integer counters and cursors); no float atomics anywhere; every output position comes from a prefix sum or a sorted run, so
// two runs give the same bits.  include/tgs_raster.h ("marching tetrahedra") has the rules in full; tests/mt_ref.py restates them.
//
// Three calls, because the output sizes depend on the data (the caller reads `counts` back after the first and after the second):
//   tgs_marching_tets_classify   k_mt_signs (sdf > 0 packed into a bitmap of N / 8 bytes: a wave's ballot is one 64-bit word), k_mt_classify (one
//                                lane per tetrahedron: 16 or 32 bytes of indices, four bits gathered from the bitmap, the range check, the case
//                                code into a byte per tetrahedron, valid_tets, and the workgroup's number of one- and two-triangle tetrahedra),
//                                two scans over the workgroup counts -> counts[0] = n_one, counts[1] = n_two, counts[2] = the index flag.
//   tgs_marching_tets_edges      the table is sized from n_one, n_two (3 n_one + 4 n_two crossing edges before dedupe).  k_mt_insert (the
//                                crossing edges of every valid tetrahedron into the edge set of tgs_edge_set.hpp; whoever claims a free slot
//                                adds one to the count of the edge's min vertex), one scan over N (tgs_runs.hpp) -> the run of every vertex's
//                                edges, counts[3] = M.
//   tgs_marching_tets_emit       k_edge_fill and k_edge_sort (tgs_edge_set.hpp: every key to its vertex's run, through a cursor, then one lane
//                                per vertex sorts its run by the max index: now interp_v is in ascending (min, max) order whatever the cursors
//                                did), k_mt_verts (one lane per edge), k_mt_faces (one lane per tetrahedron: the ranks among the one- and the
//                                two-triangle tetrahedra from a workgroup scan on top of the scanned workgroup counts; every corner's edge is
//                                found by a binary search in its min vertex's run).
// tgs_marching_tets_backward is a gather per grid row: k_mt_grad_count (edges per min and per max vertex), two scans, k_mt_grad_fill (edge
// numbers into the max side's runs), k_mt_grad (one lane per grid row: its run of interp_v as the min end, then its max-side list sorted by edge
// number, added in double and rounded once).
//
// The case table is written as the tetrahedron's corner pairs: a triangle corner is the crossing of the edge between local corners i and j, one
// byte 0xij, three bytes per triangle, the first triangle in the high half.  tests/golden/ref_mt_fixture.npz (cases16) pins it.
#include "tgs_tet_common.hpp"                                           // the row load; with it tgs_runs.hpp: the scans, the run bounds, sort and search
#include "tgs_edge_set.hpp"                                             // the edge set, its fill and its sort

namespace tgs {

constexpr long long MT_MAX_CROSSING = 1ll << 33;                        // 4 F with F < 2^31

#define MT_TRI(a, b, c) ((unsigned long long)(((a) << 16) | ((b) << 8) | (c)))
#define MT_ONE(a, b, c) (MT_TRI(a, b, c) << 24)
#define MT_TWO(a, b, c, d, e, f) ((MT_TRI(a, b, c) << 24) | MT_TRI(d, e, f))
__constant__ unsigned long long MT_CASES[16] = {
    0ull,
    MT_ONE(0x02, 0x01, 0x03),                                           // corner 0 inside
    MT_ONE(0x13, 0x01, 0x12),                                           // corner 1
    MT_TWO(0x02, 0x13, 0x03, 0x02, 0x12, 0x13),                         // 0, 1
    MT_ONE(0x12, 0x02, 0x23),                                           // corner 2
    MT_TWO(0x03, 0x12, 0x01, 0x03, 0x23, 0x12),                         // 0, 2
    MT_TWO(0x02, 0x13, 0x01, 0x02, 0x23, 0x13),                         // 1, 2
    MT_ONE(0x13, 0x03, 0x23),                                           // all but corner 3
    MT_ONE(0x13, 0x23, 0x03),                                           // corner 3
    MT_TWO(0x13, 0x02, 0x01, 0x13, 0x23, 0x02),                         // 0, 3
    MT_TWO(0x12, 0x03, 0x01, 0x12, 0x23, 0x03),                         // 1, 3
    MT_ONE(0x02, 0x12, 0x23),                                           // all but corner 2
    MT_TWO(0x13, 0x02, 0x03, 0x13, 0x12, 0x02),                         // 2, 3
    MT_ONE(0x12, 0x01, 0x13),                                           // all but corner 1
    MT_ONE(0x03, 0x01, 0x02),                                           // all but corner 0
    0ull,
};

struct MtWork {
    unsigned long long* bits;             // [(N + 63) / 64] sdf > 0, bit v & 63 of word v >> 6
    uint8_t* code;                        // [F] the case code of a valid tetrahedron, 0 otherwise
    uint32_t* blk_one;                    // [ceil(F / 256) + 1] one-triangle tetrahedra per workgroup of k_mt_classify; scanned (exclusive)
    uint32_t* blk_two;                    // likewise, two-triangle
    uint32_t* run;                        // [N + 1] crossing edges per min vertex; scanned: run[v] is where v's edges start; after k_edge_fill where they end
    uint32_t* scan;                       // scratch of the scans
};
__host__ __device__ inline size_t mt_carve(MtWork& w, char* base, size_t N, size_t F)
{
    char* p = base;
    const size_t big = N + 1 > run_blocks(F) + 1 ? N + 1 : run_blocks(F) + 1;
    carve(p, w.bits, (N + 63) / 64 + 1); carve(p, w.code, F + 1); carve(p, w.blk_one, run_blocks(F) + 1); carve(p, w.blk_two, run_blocks(F) + 1);
    carve(p, w.run, N + 1); carve(p, w.scan, run_scan_scratch(big));
    return (size_t)(p - base) + 256;
}
__host__ __device__ inline size_t mt_table_capacity(long long n_crossing)
{
    size_t cap = 64;                                                    // a power of two >= 2 n_crossing: load <= 1/2
    while (cap < 2 * (size_t)n_crossing) cap <<= 1;
    return cap;
}

struct MtGradWork {
    uint32_t* run_a;                      // [N + 1] edges per min vertex, scanned: interp_v rows run_a[v] .. run_a[v+1] have v as their min end
    uint32_t* run_b;                      // [N + 1] edges per max vertex, scanned; after the fill run_b[v] is where v's list ends
    uint32_t* list_b;                     // [M] edge numbers by max vertex
    uint32_t* scan;
};
__host__ __device__ inline size_t mt_grad_carve(MtGradWork& w, char* base, size_t N, size_t M)
{
    char* p = base;
    carve(p, w.run_a, N + 1); carve(p, w.run_b, N + 1); carve(p, w.list_b, M + 1); carve(p, w.scan, run_scan_scratch(N + 1));
    return (size_t)(p - base) + 256;
}

// ---- forward ----
__global__ __launch_bounds__(RUN_BLOCK) void k_mt_signs(int N, const float* __restrict__ sdf, unsigned long long* __restrict__ bits)
{
    const size_t v = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    const bool inside = v < (size_t)N && sdf[v] > 0.f;                  // NaN and 0 are outside
    const unsigned long long word = __ballot(inside);
    if ((threadIdx.x & 63) == 0 && v < (size_t)N) bits[v >> 6] = word;
}
__device__ __forceinline__ uint32_t mt_bit(const unsigned long long* __restrict__ bits, long long v)
{
    return (uint32_t)(bits[v >> 6] >> (v & 63)) & 1u;
}
template <typename Idx>
__global__ __launch_bounds__(RUN_BLOCK) void k_mt_classify(int N, int F, const Idx* __restrict__ tet, const unsigned long long* __restrict__ bits,
                                                          uint8_t* __restrict__ code, uint8_t* __restrict__ valid, uint32_t* __restrict__ blk_one,
                                                          uint32_t* __restrict__ blk_two, long long* __restrict__ counts)
{
    __shared__ uint32_t lds[4];
    const size_t f = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    uint32_t c = 0;
    if (f < (size_t)F) {
        long long t[4];
        mt_load_tet(tet, f, t);
        if (mt_in_range(t, N)) {
            c = mt_bit(bits, t[0]) | (mt_bit(bits, t[1]) << 1) | (mt_bit(bits, t[2]) << 2) | (mt_bit(bits, t[3]) << 3);
            if (c == 15u) c = 0;
        } else {
            atomicOr((unsigned long long*)&counts[2], 1ull);           // refused by the caller after the read-back; the tetrahedron is left out here
        }
        code[f] = (uint8_t)c;
        valid[f] = c != 0;
    }
    const bool two = __popc(c) == 2;
    const uint32_t pack = c == 0 ? 0u : two ? 0x10000u : 1u;            // both counts in one scan: at most 256 each
    uint32_t total;
    run_block_escan(pack, total, lds);
    if (threadIdx.x == 0) { blk_one[blockIdx.x] = total & 0xffffu; blk_two[blockIdx.x] = total >> 16; }
}

template <typename Idx>
__global__ __launch_bounds__(RUN_BLOCK) void k_mt_insert(int N, int F, const Idx* __restrict__ tet, const uint8_t* __restrict__ code, size_t cap,
                                                        unsigned long long* __restrict__ keys, uint32_t* __restrict__ run)
{
    const size_t f = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (f >= (size_t)F) return;
    const uint32_t c = code[f];
    if (c == 0) return;
    long long t[4];
    mt_load_tet(tet, f, t);
    if (!mt_in_range(t, N)) return;                                     // (never: code is this call sequence's own)
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = i + 1; j < 4; j++) {
            if ((((c >> i) ^ (c >> j)) & 1u) == 0) continue;             // both inside or both outside (an edge of equal indices is always that)
            const long long a = t[i] < t[j] ? t[i] : t[j], b = t[i] < t[j] ? t[j] : t[i];
            bool claimed;
            edge_insert(keys, cap, edge_key(a, b), claimed);
            if (claimed) atomicAdd(&run[a], 1u);
        }
}

// v = pos[a] w_a + pos[b] w_b with w_a = (-sdf[b]) / D, w_b = sdf[a] / D, D = sdf[a] + (-sdf[b]); every operation rounded on its own
__global__ __launch_bounds__(RUN_BLOCK) void k_mt_verts(int N, long long M, const float* __restrict__ pos, const float* __restrict__ sdf,
                                                       const long long* __restrict__ interp_v, float* __restrict__ verts)
{
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (e >= M) return;
    const long long a = interp_v[2 * e], b = interp_v[2 * e + 1];
    if ((unsigned long long)a >= (unsigned long long)N || (unsigned long long)b >= (unsigned long long)N) return;
    const float sa = sdf[a], nb = -sdf[b];
    const float D = sa + nb;
    const float wa = nb / D, wb = sa / D;
#pragma unroll
    for (int k = 0; k < 3; k++) verts[3 * e + k] = pos[3 * a + k] * wa + pos[3 * b + k] * wb;
}

// the row of interp_v that holds (a, b), -1 if none (never, for a crossing edge of this call sequence)
__device__ __forceinline__ long long mt_find(int N, long long M, const uint32_t* __restrict__ run, const long long* __restrict__ interp_v, long long a, long long b)
{
    const Run r = run_bounds(run, (size_t)a, (size_t)M);
    return run_search(interp_v + 1, 2, (long long)r.lo, (long long)r.hi, b);
}

template <typename Idx>
__global__ __launch_bounds__(RUN_BLOCK) void k_mt_faces(int N, int F, long long M, long long n_one, long long T, const Idx* __restrict__ tet,
                                                       const uint8_t* __restrict__ code, const uint32_t* __restrict__ blk_one, const uint32_t* __restrict__ blk_two,
                                                       const uint32_t* __restrict__ run, const long long* __restrict__ interp_v,
                                                       long long* __restrict__ faces, long long* __restrict__ face_to_tet)
{
    __shared__ uint32_t lds[4];
    const size_t f = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    const uint32_t c = f < (size_t)F ? code[f] : 0u;
    const bool two = __popc(c) == 2;
    const uint32_t pack = c == 0 ? 0u : two ? 0x10000u : 1u;
    uint32_t total;
    const uint32_t before = run_block_escan(pack, total, lds);
    if (c == 0) return;
    long long t[4];
    mt_load_tet(tet, f, t);
    if (!mt_in_range(t, N)) return;
    const long long first = two ? n_one + 2 * ((long long)blk_two[blockIdx.x] + (before >> 16)) : (long long)blk_one[blockIdx.x] + (before & 0xffffu);
    const unsigned long long tris = MT_CASES[c];
    const int n_tri = two ? 2 : 1;
    for (int k = 0; k < n_tri; k++) {
        const long long row = first + k;
        if (row >= T) return;
        const uint32_t tri = (uint32_t)(tris >> (k ? 0 : 24)) & 0xffffffu;
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const uint32_t ij = (tri >> (16 - 8 * q)) & 0xffu;
            const long long x = t[ij >> 4], y = t[ij & 3u];
            faces[3 * row + q] = mt_find(N, M, run, interp_v, x < y ? x : y, x < y ? y : x);
        }
        face_to_tet[row] = (long long)f;
    }
}

// ---- backward ----
__global__ __launch_bounds__(RUN_BLOCK) void k_mt_grad_count(int N, long long M, const long long* __restrict__ interp_v, uint32_t* __restrict__ run_a, uint32_t* __restrict__ run_b)
{
    const long long e = (long long)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (e >= M) return;
    const long long a = interp_v[2 * e], b = interp_v[2 * e + 1];
    if ((unsigned long long)a >= (unsigned long long)N || (unsigned long long)b >= (unsigned long long)N) return;
    atomicAdd(&run_a[a], 1u);
    atomicAdd(&run_b[b], 1u);
}
__global__ __launch_bounds__(RUN_BLOCK) void k_mt_grad_fill(int N, long long M, const long long* __restrict__ interp_v, uint32_t* __restrict__ run_b, uint32_t* __restrict__ list_b)
{
    const long long e = (long long)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (e >= M) return;
    const long long a = interp_v[2 * e], b = interp_v[2 * e + 1];
    if ((unsigned long long)a >= (unsigned long long)N || (unsigned long long)b >= (unsigned long long)N) return;
    const uint32_t p = atomicAdd(&run_b[b], 1u);
    if ((long long)p < M) list_b[p] = (uint32_t)e;
}

struct MtAcc { double p[3]; double s; };
// edge e's contribution to grid row `self`, its min end (as_a) or its max end
__device__ __forceinline__ void mt_grad_edge(int N, const float* __restrict__ pos, const float* __restrict__ sdf, const long long* __restrict__ interp_v,
                                             const float* __restrict__ g_verts, long long e, long long self, bool as_a, MtAcc& acc)
{
    const long long a = interp_v[2 * e], b = interp_v[2 * e + 1];
    if ((as_a ? a : b) != self || (unsigned long long)(as_a ? b : a) >= (unsigned long long)N) return;
    const double sa = sdf[a], sb = sdf[b], D = sa - sb;
    const double wa = -sb / D, wb = sa / D;
    double dot = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double g = g_verts[3 * e + k], pa = pos[3 * a + k], pb = pos[3 * b + k];
        const double v = pa * wa + pb * wb;
        acc.p[k] += g * (as_a ? wa : wb);
        dot += g * (as_a ? pb - v : v - pa);
    }
    acc.s += dot / D;
}
__global__ __launch_bounds__(RUN_BLOCK) void k_mt_grad(int N, long long M, const float* __restrict__ pos, const float* __restrict__ sdf,
                                                      const long long* __restrict__ interp_v, const float* __restrict__ g_verts, const uint32_t* __restrict__ run_a,
                                                      const uint32_t* __restrict__ run_b, uint32_t* __restrict__ list_b, float* __restrict__ d_pos, float* __restrict__ d_sdf)
{
    const size_t v = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (v >= (size_t)N) return;
    MtAcc acc = {{0.0, 0.0, 0.0}, 0.0};
    long long lo = run_a[v], hi = run_a[v + 1];
    if (hi > M) hi = M;
    for (long long e = lo; e < hi; e++) mt_grad_edge(N, pos, sdf, interp_v, g_verts, e, (long long)v, true, acc);
    const Run r = run_bounds(run_b, v, (size_t)M);                       // (the fill's cursors: ends)
    lo = (long long)r.lo; hi = (long long)r.hi;
    run_sort(list_b, 1, lo, hi);                                        // ascending edge number, whatever the cursors did
    for (long long i = lo; i < hi; i++) mt_grad_edge(N, pos, sdf, interp_v, g_verts, (long long)list_b[i], (long long)v, false, acc);
    if (d_pos) { d_pos[3 * v] = (float)acc.p[0]; d_pos[3 * v + 1] = (float)acc.p[1]; d_pos[3 * v + 2] = (float)acc.p[2]; }
    if (d_sdf) d_sdf[v] = (float)acc.s;
}

}  // namespace tgs

extern "C" {
#include "../../include/tgs_raster.h"

size_t tgs_marching_tets_workspace_bytes(int N, int F)
{
    tgs::MtWork w;
    if (N < 0 || F < 0) return 0;
    return tgs::mt_carve(w, nullptr, (size_t)N, (size_t)F);
}

size_t tgs_marching_tets_table_bytes(int64_t n_crossing)
{
    if (n_crossing < 0 || n_crossing > tgs::MT_MAX_CROSSING) return 0;
    return tgs::mt_table_capacity(n_crossing) * sizeof(unsigned long long) + 256;
}

int tgs_marching_tets_classify(void* stream, int N, int F, const float* sdf, const void* tet, int tet_is_int64, uint8_t* valid_tets, int64_t* counts,
                               void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (N < 0 || F < 0 || !counts || !workspace || (N > 0 && !sdf) || (F > 0 && (!tet || !valid_tets)) || (tet_is_int64 != 0 && tet_is_int64 != 1) || !mt_aligned(tet))
        return set_error(TGS_ERR_INVALID, "tgs_marching_tets_classify: N >= 0, F >= 0, tet_is_int64 in {0, 1} and non-NULL sdf / tet (16-byte aligned) / valid_tets / counts / workspace required");
    MtWork w;
    if (mt_carve(w, (char*)workspace, (size_t)N, (size_t)F) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_marching_tets_classify: workspace smaller than tgs_marching_tets_workspace_bytes(N, F)");
    if (hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), st) != hipSuccess) return hip_status("tgs_marching_tets_classify");
    if (F == 0) return TGS_OK;
    if (N > 0) hipLaunchKernelGGL(k_mt_signs, run_grid((size_t)N), dim3(RUN_BLOCK), 0, st, N, sdf, w.bits);
    long long* cnt = (long long*)counts;
    if (tet_is_int64) hipLaunchKernelGGL(k_mt_classify<long long>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, N, F, (const long long*)tet, w.bits, w.code, valid_tets, w.blk_one, w.blk_two, cnt);
    else              hipLaunchKernelGGL(k_mt_classify<int>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, N, F, (const int*)tet, w.bits, w.code, valid_tets, w.blk_one, w.blk_two, cnt);
    run_scan(st, w.blk_one, run_blocks((size_t)F), w.scan, cnt + 0);
    run_scan(st, w.blk_two, run_blocks((size_t)F), w.scan, cnt + 1);
    return hip_status("tgs_marching_tets_classify");
}

int tgs_marching_tets_edges(void* stream, int N, int F, const void* tet, int tet_is_int64, int64_t n_one, int64_t n_two, int64_t* counts,
                            void* workspace, size_t workspace_bytes, void* table, size_t table_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (N <= 0 || F <= 0 || !tet || !mt_aligned(tet) || !counts || !workspace || !table || (tet_is_int64 != 0 && tet_is_int64 != 1) || n_one < 0 || n_two < 0 || n_one + n_two > F || n_one + n_two == 0)
        return set_error(TGS_ERR_INVALID, "tgs_marching_tets_edges: N > 0, F > 0, 0 < n_one + n_two <= F as tgs_marching_tets_classify counted them and non-NULL tet / counts / "
                                          "workspace / table and a 16-byte aligned tet required");
    MtWork w;
    if (mt_carve(w, (char*)workspace, (size_t)N, (size_t)F) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_marching_tets_edges: workspace smaller than tgs_marching_tets_workspace_bytes(N, F)");
    const long long n_crossing = 3 * n_one + 4 * n_two;
    const size_t cap = mt_table_capacity(n_crossing);
    if (cap * sizeof(unsigned long long) + 256 > table_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_marching_tets_edges: table smaller than tgs_marching_tets_table_bytes(3 n_one + 4 n_two)");
    unsigned long long* keys = (unsigned long long*)(((uintptr_t)table + 255) & ~(uintptr_t)255);
    if (hipMemsetAsync(keys, 0xff, cap * sizeof(unsigned long long), st) != hipSuccess || hipMemsetAsync(w.run, 0, ((size_t)N + 1) * sizeof(uint32_t), st) != hipSuccess)
        return hip_status("tgs_marching_tets_edges");
    if (tet_is_int64) hipLaunchKernelGGL(k_mt_insert<long long>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, N, F, (const long long*)tet, w.code, cap, keys, w.run);
    else              hipLaunchKernelGGL(k_mt_insert<int>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, N, F, (const int*)tet, w.code, cap, keys, w.run);
    run_scan(st, w.run, (size_t)N + 1, w.scan, (long long*)counts + 3);
    return hip_status("tgs_marching_tets_edges");
}

int tgs_marching_tets_emit(void* stream, int N, int F, const float* pos, const float* sdf, const void* tet, int tet_is_int64, int64_t n_one, int64_t n_two, int64_t M,
                           float* verts, int64_t* interp_v, int64_t* faces, int64_t* face_to_tet_idx, void* workspace, size_t workspace_bytes, void* table, size_t table_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (N <= 0 || F <= 0 || !pos || !sdf || !tet || !mt_aligned(tet) || !verts || !interp_v || !faces || !face_to_tet_idx || !workspace || !table || (tet_is_int64 != 0 && tet_is_int64 != 1) ||
        n_one < 0 || n_two < 0 || n_one + n_two > F || n_one + n_two == 0 || M <= 0 || M > 3 * n_one + 4 * n_two)
        return set_error(TGS_ERR_INVALID, "tgs_marching_tets_emit: N > 0, F > 0, 0 < n_one + n_two <= F, 0 < M <= 3 n_one + 4 n_two as the two calls before counted them and "
                                          "non-NULL pos / sdf / tet (16-byte aligned) / verts / interp_v / faces / face_to_tet_idx / workspace / table required");
    MtWork w;
    if (mt_carve(w, (char*)workspace, (size_t)N, (size_t)F) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_marching_tets_emit: workspace smaller than tgs_marching_tets_workspace_bytes(N, F)");
    const size_t cap = mt_table_capacity(3 * n_one + 4 * n_two);
    if (cap * sizeof(unsigned long long) + 256 > table_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_marching_tets_emit: table smaller than tgs_marching_tets_table_bytes(3 n_one + 4 n_two)");
    const unsigned long long* keys = (const unsigned long long*)(((uintptr_t)table + 255) & ~(uintptr_t)255);
    const long long T = n_one + 2 * n_two;
    long long* iv = (long long*)interp_v;
    hipLaunchKernelGGL(k_edge_fill, run_grid(cap), dim3(RUN_BLOCK), 0, st, N, (long long)M, cap, keys, w.run, iv);
    hipLaunchKernelGGL(k_edge_sort, run_grid((size_t)N), dim3(RUN_BLOCK), 0, st, N, (long long)M, (const uint32_t*)w.run, iv);
    hipLaunchKernelGGL(k_mt_verts, run_grid((size_t)M), dim3(RUN_BLOCK), 0, st, N, (long long)M, pos, sdf, (const long long*)iv, verts);
    if (tet_is_int64)
        hipLaunchKernelGGL(k_mt_faces<long long>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, N, F, (long long)M, (long long)n_one, T, (const long long*)tet, (const uint8_t*)w.code,
                           (const uint32_t*)w.blk_one, (const uint32_t*)w.blk_two, (const uint32_t*)w.run, (const long long*)iv, (long long*)faces, (long long*)face_to_tet_idx);
    else
        hipLaunchKernelGGL(k_mt_faces<int>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, N, F, (long long)M, (long long)n_one, T, (const int*)tet, (const uint8_t*)w.code,
                           (const uint32_t*)w.blk_one, (const uint32_t*)w.blk_two, (const uint32_t*)w.run, (const long long*)iv, (long long*)faces, (long long*)face_to_tet_idx);
    return hip_status("tgs_marching_tets_emit");
}

size_t tgs_marching_tets_backward_workspace_bytes(int N, int64_t M)
{
    tgs::MtGradWork w;
    if (N < 0 || M < 0 || M > tgs::MT_MAX_CROSSING / 2) return 0;
    return tgs::mt_grad_carve(w, nullptr, (size_t)N, (size_t)M);
}

int tgs_marching_tets_backward(void* stream, int N, int64_t M, const float* pos, const float* sdf, const int64_t* interp_v, const float* dL_dverts,
                               float* dL_dpos, float* dL_dsdf, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (N < 0 || M < 0 || M > MT_MAX_CROSSING / 2 || !workspace || (M > 0 && (N == 0 || !pos || !sdf || !interp_v || !dL_dverts)))
        return set_error(TGS_ERR_INVALID, "tgs_marching_tets_backward: N >= 0, 0 <= M < 2^32 (N > 0 where M > 0) and non-NULL pos / sdf / interp_v / dL_dverts / workspace required");
    MtGradWork w;
    if (mt_grad_carve(w, (char*)workspace, (size_t)N, (size_t)M) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_marching_tets_backward: workspace smaller than tgs_marching_tets_backward_workspace_bytes(N, M)");
    if ((!dL_dpos && !dL_dsdf) || N == 0) return TGS_OK;
    if (M == 0) {                                                       // nothing reaches a row: zeros
        if ((dL_dpos && hipMemsetAsync(dL_dpos, 0, 3 * (size_t)N * sizeof(float), st) != hipSuccess) ||
            (dL_dsdf && hipMemsetAsync(dL_dsdf, 0, (size_t)N * sizeof(float), st) != hipSuccess)) return hip_status("tgs_marching_tets_backward");
        return TGS_OK;
    }
    if (hipMemsetAsync(w.run_a, 0, ((size_t)N + 1) * sizeof(uint32_t), st) != hipSuccess || hipMemsetAsync(w.run_b, 0, ((size_t)N + 1) * sizeof(uint32_t), st) != hipSuccess)
        return hip_status("tgs_marching_tets_backward");
    const long long* iv = (const long long*)interp_v;
    hipLaunchKernelGGL(k_mt_grad_count, run_grid((size_t)M), dim3(RUN_BLOCK), 0, st, N, (long long)M, iv, w.run_a, w.run_b);
    run_scan(st, w.run_a, (size_t)N + 1, w.scan, (long long*)nullptr);
    run_scan(st, w.run_b, (size_t)N + 1, w.scan, (long long*)nullptr);
    hipLaunchKernelGGL(k_mt_grad_fill, run_grid((size_t)M), dim3(RUN_BLOCK), 0, st, N, (long long)M, iv, w.run_b, w.list_b);
    hipLaunchKernelGGL(k_mt_grad, run_grid((size_t)N), dim3(RUN_BLOCK), 0, st, N, (long long)M, pos, sdf, iv, dL_dverts, (const uint32_t*)w.run_a, (const uint32_t*)w.run_b,
                       w.list_b, dL_dpos, dL_dsdf);
    return hip_status("tgs_marching_tets_backward");
}
}
