// tgs_tet_grid.hip -- the tetrahedral grid's own topology passes of the geometry stage (tetgs_spatial/models/isosurface.py :264-345,
// `compact_tets` and `batch_subdivide_volume`; :208-261, `mark_part_tets`), for gfx950.  Plain HIP, wave64.  Integer atomics only (atomicOr on
// bitmap words, integer counters and cursors); every output position comes from a prefix sum or a sorted run, so two runs give the same bits.
// include/tgs_raster.h ("tetrahedral grids") has the rules in full; tests/tet_ref.py restates them.
//
// compact, two calls around one read-back of (F', N', the index flag):
//   tgs_tet_compact_select   k_tg_select (one lane per tetrahedron: 16 or 32 bytes of indices, the range check, the rule -- the sdf mean against
//                            the threshold, or the caller's keep byte --, a flag byte, the workgroup's count, atomicOr of the kept corners into a
//                            bitmap of N bits), one scan over the workgroup counts, k_tg_popc (a word's popcount) and one scan over the words.
//   tgs_tet_compact_emit     k_tg_emit_tets (one lane per tetrahedron: its row from a workgroup scan on top of the scanned counts; a corner's new
//                            index is its word's prefix plus the popcount of the bits below it), k_tg_emit_verts (one lane per grid vertex whose
//                            bit is set: the old index, the gathered rows, and the membership in another call's bitmap).
// subdivide, two calls around one read-back of (E, the index flag).  No hash table: all 6 F edges go into their min vertex's run (a count per
// min vertex, one scan over N, a fill through cursors), one lane sorts its vertex's run and drops the repeats in place, and a second scan over
// the distinct counts ranks the edges.  24 bytes per tetrahedron of workspace where the open-addressing table of tgs_marching_tets.hip would
// take 96 (6 F keys of 8 bytes at load <= 1/2), no CAS, no table to clear, and the size is known before the call; the price is runs about five
// times as long for the one lane that sorts them (an interior edge of a grid is listed by four to six tetrahedra).
//   tgs_tet_subdivide_edges  k_ts_count, scan, k_ts_fill, k_ts_sort_unique, scan.  (The scans, the run bounds, the sort that drops repeats and the
//                            binary search are tgs_runs.hpp's, as in tgs_marching_tets.hip and tgs_mesh_geom.hip.)
//   tgs_tet_subdivide_emit   k_ts_edges (one lane per vertex writes its rows of `edges`), k_ts_verts (one lane per row of new_v and batch
//                            element: a copy, or the midpoint (a + b) * 0.5f; the mask row), k_ts_tets (one lane per tetrahedron: six binary
//                            searches, eight rows, eight parents).
#include "tgs_tet_common.hpp"                                           // the row load, shared with tgs_marching_tets.hip; with it tgs_runs.hpp

namespace tgs {

constexpr int TG_MAX_SUBDIV_F = 0x7fffffff / 8;                         // 8 F rows of new_tets stay below 2^31 (and 6 F candidates below 2^32)

struct TgCompactWork {
    unsigned long long* bits;             // [(N + 63) / 64 + 1] bit v & 63 of word v >> 6: a kept tetrahedron uses vertex v.  FIRST, so another call finds it
    uint8_t* kept;                        // [F] 1: the tetrahedron is kept
    uint32_t* blk;                        // [ceil(F / 256) + 1] kept tetrahedra per workgroup of k_tg_select; scanned (exclusive)
    uint32_t* wpre;                       // [(N + 63) / 64 + 1] popcount per bitmap word; scanned (exclusive)
    uint32_t* scan;
};
__host__ __device__ inline size_t tg_words(size_t N) { return (N + 63) / 64; }
__host__ __device__ inline size_t tg_compact_carve(TgCompactWork& w, char* base, size_t N, size_t F)
{
    char* p = base;
    const size_t big = tg_words(N) + 1 > run_blocks(F) + 1 ? tg_words(N) + 1 : run_blocks(F) + 1;
    carve(p, w.bits, tg_words(N) + 1); carve(p, w.kept, F + 1); carve(p, w.blk, run_blocks(F) + 1); carve(p, w.wpre, tg_words(N) + 1);
    carve(p, w.scan, run_scan_scratch(big));
    return (size_t)(p - base) + 256;
}

struct TgSubdivWork {
    uint32_t* run;                        // [N + 1] edges per min vertex; scanned: where v's run starts; after k_ts_fill where it ends
    uint32_t* urun;                       // [N + 1] distinct edges per min vertex; scanned: the number of v's first edge
    uint32_t* list;                       // [6 F] max indices by min vertex; after k_ts_sort_unique the first urun[v + 1] - urun[v] of a run are its distinct ones, ascending
    uint32_t* scan;
};
__host__ __device__ inline size_t tg_subdiv_carve(TgSubdivWork& w, char* base, size_t N, size_t F)
{
    char* p = base;
    carve(p, w.run, N + 1); carve(p, w.urun, N + 1); carve(p, w.list, 6 * F + 1); carve(p, w.scan, run_scan_scratch(N + 1));
    return (size_t)(p - base) + 256;
}

// mask element types: what the integer (or, after one subdivision, float) keep / edit mask may be stored as
enum { TG_MASK_I32 = 0, TG_MASK_I64 = 1, TG_MASK_F32 = 2, TG_MASK_U8 = 3 };
__host__ __device__ inline int tg_mask_bytes(int type) { return type == TG_MASK_I64 ? 8 : type == TG_MASK_U8 ? 1 : 4; }

// ---- compact ----
template <typename Idx>
__global__ __launch_bounds__(RUN_BLOCK) void k_tg_select(int N, int F, const float* __restrict__ sdf, const Idx* __restrict__ tet, const uint8_t* __restrict__ keep,
                                                        float threshold, unsigned long long* __restrict__ bits, uint8_t* __restrict__ kept,
                                                        uint32_t* __restrict__ blk, long long* __restrict__ counts)
{
#pragma clang fp contract(off)
    __shared__ uint32_t lds[4];
    const size_t f = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    uint32_t k = 0;
    if (f < (size_t)F) {
        long long t[4];
        mt_load_tet(tet, f, t);
        if (mt_in_range(t, N)) {
            if (keep) {
                k = keep[f] != 0;
            } else {
                const float mean = (((sdf[t[0]] + sdf[t[1]]) + sdf[t[2]]) + sdf[t[3]]) * 0.25f;
                k = fabsf(mean) <= threshold;                           // a NaN mean is dropped
            }
            if (k) {
#pragma unroll
                for (int c = 0; c < 4; c++) {                           // a vertex is shared by two dozen tetrahedra and a word by 64 vertices: look first.
                    const unsigned long long bit = 1ull << (t[c] & 63); // (bits are only ever set here, so a set bit that is seen is final and an unseen one costs one more atomic)
                    if (!(bits[t[c] >> 6] & bit)) atomicOr(&bits[t[c] >> 6], bit);
                }
            }
        } else {
            atomicOr((unsigned long long*)&counts[2], 1ull);           // refused by the caller after the read-back; the tetrahedron is left out here
        }
        kept[f] = (uint8_t)k;
    }
    uint32_t total;
    run_block_escan(k, total, lds);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}
__global__ __launch_bounds__(RUN_BLOCK) void k_tg_popc(size_t words, const unsigned long long* __restrict__ bits, uint32_t* __restrict__ wpre)
{
    const size_t w = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (w < words) wpre[w] = (uint32_t)__popcll(bits[w]);
}
// the number of set bits below v: v's row among the kept vertices
__device__ __forceinline__ long long tg_rank(const unsigned long long* __restrict__ bits, const uint32_t* __restrict__ wpre, long long v)
{
    const unsigned long long below = bits[v >> 6] & ((1ull << (v & 63)) - 1ull);
    return (long long)wpre[v >> 6] + __popcll(below);
}
template <typename Idx, typename Out>
__global__ __launch_bounds__(RUN_BLOCK) void k_tg_emit_tets(int N, int F, long long Fk, const Idx* __restrict__ tet, const uint8_t* __restrict__ kept,
                                                           const uint32_t* __restrict__ blk, const unsigned long long* __restrict__ bits,
                                                           const uint32_t* __restrict__ wpre, Out* __restrict__ new_tets, Out* __restrict__ idx_to_old)
{
    __shared__ uint32_t lds[4];
    const size_t f = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    const uint32_t k = f < (size_t)F ? kept[f] : 0u;
    uint32_t total;
    const long long row = (long long)blk[blockIdx.x] + run_block_escan(k, total, lds);
    if (!k || row >= Fk) return;
    long long t[4];
    mt_load_tet(tet, f, t);
    if (!mt_in_range(t, N)) return;                                     // (never: kept is this call sequence's own)
#pragma unroll
    for (int c = 0; c < 4; c++) new_tets[4 * row + c] = (Out)tg_rank(bits, wpre, t[c]);
    idx_to_old[row] = (Out)f;
}
template <typename Out>
__global__ __launch_bounds__(RUN_BLOCK) void k_tg_emit_verts(int N, long long Nk, const unsigned long long* __restrict__ bits, const uint32_t* __restrict__ wpre,
                                                            const float* __restrict__ pos, const float* __restrict__ sdf, const void* __restrict__ mask,
                                                            int mask_bytes, const unsigned long long* __restrict__ member_bits, Out* __restrict__ unique_vtx,
                                                            float* __restrict__ new_pos, float* __restrict__ new_sdf, void* __restrict__ new_mask,
                                                            int* __restrict__ member)
{
    const long long v = (long long)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (v >= N || !((bits[v >> 6] >> (v & 63)) & 1ull)) return;
    const long long r = tg_rank(bits, wpre, v);
    if (r >= Nk) return;
    unique_vtx[r] = (Out)v;
    if (pos) { new_pos[3 * r] = pos[3 * v]; new_pos[3 * r + 1] = pos[3 * v + 1]; new_pos[3 * r + 2] = pos[3 * v + 2]; }
    if (sdf) new_sdf[r] = sdf[v];
    if (mask) {                                                         // a bit copy of the element, whatever it holds
        if (mask_bytes == 8) ((unsigned long long*)new_mask)[r] = ((const unsigned long long*)mask)[v];
        else if (mask_bytes == 4) ((uint32_t*)new_mask)[r] = ((const uint32_t*)mask)[v];
        else ((uint8_t*)new_mask)[r] = ((const uint8_t*)mask)[v];
    }
    if (member_bits) member[r] = (int)((member_bits[v >> 6] >> (v & 63)) & 1ull);
}

// ---- subdivide ----
// 1 if corner i is the min end of the edge between corners i and j (equal indices: the lower corner), so each of the six edges has one min end
__device__ __forceinline__ uint32_t ts_min_end(const long long t[4], int i, int j)
{
    return (i != j && (t[i] < t[j] || (t[i] == t[j] && i < j))) ? 1u : 0u;
}
template <typename Idx>
__global__ __launch_bounds__(RUN_BLOCK) void k_ts_count(int N, int F, const Idx* __restrict__ tet, uint32_t* __restrict__ run, long long* __restrict__ counts)
{
    const size_t f = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (f >= (size_t)F) return;
    long long t[4];
    mt_load_tet(tet, f, t);
    if (!mt_in_range(t, N)) { atomicOr((unsigned long long*)&counts[1], 1ull); return; }
#pragma unroll
    for (int i = 0; i < 4; i++) {                                       // one atomic per corner that is the min end of an edge: three at the most
        uint32_t k = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) k += ts_min_end(t, i, j);
        if (k) atomicAdd(&run[t[i]], k);
    }
}
template <typename Idx>
__global__ __launch_bounds__(RUN_BLOCK) void k_ts_fill(int N, int F, const Idx* __restrict__ tet, uint32_t* __restrict__ run, uint32_t* __restrict__ list)
{
    const size_t f = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (f >= (size_t)F) return;
    long long t[4];
    mt_load_tet(tet, f, t);
    if (!mt_in_range(t, N)) return;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint32_t k = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) k += ts_min_end(t, i, j);
        if (!k) continue;
        size_t p = atomicAdd(&run[t[i]], k);                            // the cursor: run[a] ends at the start of a + 1's run
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (ts_min_end(t, i, j)) { if (p < 6 * (size_t)F) list[p] = (uint32_t)t[j]; p++; }
    }
}
// run[v] is now the END of v's run (the start of v + 1's); v's max indices are sorted and the repeats dropped, in place
__global__ __launch_bounds__(RUN_BLOCK) void k_ts_sort_unique(int N, int F, const uint32_t* __restrict__ run, uint32_t* __restrict__ list, uint32_t* __restrict__ urun)
{
    const size_t v = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (v > (size_t)N) return;
    if (v == (size_t)N) { urun[v] = 0; return; }
    const Run r = run_bounds(run, v, 6 * (size_t)F);
    urun[v] = (uint32_t)(run_sort_unique(list, (long long)r.lo, (long long)r.hi) - (long long)r.lo);
}
__global__ __launch_bounds__(RUN_BLOCK) void k_ts_edges(int N, long long E, const uint32_t* __restrict__ run, const uint32_t* __restrict__ urun,
                                                       const uint32_t* __restrict__ list, long long* __restrict__ edges)
{
    const size_t v = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (v >= (size_t)N) return;
    const long long lo = (long long)run_start(run, v), first = urun[v];
    long long last = urun[v + 1];
    if (last > E) last = E;
    for (long long e = first; e < last; e++) { edges[2 * e] = (long long)v; edges[2 * e + 1] = (long long)list[lo + (e - first)]; }
}
// 1 where the two end points' mask values sum to 2
__device__ __forceinline__ float tg_mask_mid(const void* __restrict__ mask, int type, long long a, long long b)
{
    if (type == TG_MASK_F32) return ((const float*)mask)[a] + ((const float*)mask)[b] == 2.f ? 1.f : 0.f;
    long long s;
    if (type == TG_MASK_I64) s = ((const long long*)mask)[a] + ((const long long*)mask)[b];
    else if (type == TG_MASK_I32) s = (long long)((const int*)mask)[a] + ((const int*)mask)[b];
    else s = (long long)((const uint8_t*)mask)[a] + ((const uint8_t*)mask)[b];
    return s == 2 ? 1.f : 0.f;
}
__device__ __forceinline__ float tg_mask_value(const void* __restrict__ mask, int type, long long v)
{
    return type == TG_MASK_F32 ? ((const float*)mask)[v] : type == TG_MASK_I64 ? (float)((const long long*)mask)[v]
         : type == TG_MASK_I32 ? (float)((const int*)mask)[v] : (float)((const uint8_t*)mask)[v];
}
// row r of batch element blockIdx.y: r < N a copy of pos and of the mask as float, else the midpoint of edge r - N
__global__ __launch_bounds__(RUN_BLOCK) void k_ts_verts(int N, long long E, const float* __restrict__ pos, const void* __restrict__ mask, int mask_type,
                                                       const long long* __restrict__ edges, float* __restrict__ new_v, float* __restrict__ new_mask)
{
#pragma clang fp contract(off)
    const long long r = (long long)blockIdx.x * RUN_BLOCK + threadIdx.x, R = (long long)N + E;
    if (r >= R) return;
    const size_t b = blockIdx.y;
    const float* p = pos + 3 * b * (size_t)N;
    float* out = new_v + 3 * (b * (size_t)R + (size_t)r);
    const void* m = mask ? (const char*)mask + b * (size_t)N * tg_mask_bytes(mask_type) : nullptr;
    if (r < N) {
        out[0] = p[3 * r]; out[1] = p[3 * r + 1]; out[2] = p[3 * r + 2];
        if (m) new_mask[b * (size_t)R + r] = tg_mask_value(m, mask_type, r);
        return;
    }
    const long long e = r - N, a = edges[2 * e], c = edges[2 * e + 1];
    if ((unsigned long long)a >= (unsigned long long)N || (unsigned long long)c >= (unsigned long long)N) return;   // (never: the edges are this call sequence's own)
#pragma unroll
    for (int k = 0; k < 3; k++) out[k] = (p[3 * a + k] + p[3 * c + k]) * 0.5f;
    if (m) new_mask[b * (size_t)R + r] = tg_mask_mid(m, mask_type, a, c);
}
// N + the number of edge (x, y); -1 if it is not there (never, for an edge of this call sequence)
__device__ __forceinline__ long long ts_mid(int N, long long E, const uint32_t* __restrict__ run, const uint32_t* __restrict__ urun, const uint32_t* __restrict__ list,
                                            long long x, long long y)
{
    const long long a = x < y ? x : y, b = x < y ? y : x;
    const long long lo = (long long)run_start(run, (size_t)a), first = urun[a];
    long long n = (long long)urun[a + 1] - first;
    if (first + n > E) n = E - first;
    const long long at = run_search(list, 1, lo, lo + n, b);
    return at < 0 ? -1 : (long long)N + first + (at - lo);
}
template <typename Idx>
__global__ __launch_bounds__(RUN_BLOCK) void k_ts_tets(int N, int F, long long E, const Idx* __restrict__ tet, const uint32_t* __restrict__ run,
                                                      const uint32_t* __restrict__ urun, const uint32_t* __restrict__ list, long long* __restrict__ new_tets,
                                                      long long* __restrict__ sub_to_parent)
{
    const size_t f = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (f >= (size_t)F) return;
    long long t[4];
    mt_load_tet(tet, f, t);
    if (!mt_in_range(t, N)) return;                                     // (never: the caller refused the call after the read-back)
    const long long a = t[0], b = t[1], c = t[2], d = t[3];
    const long long ab = ts_mid(N, E, run, urun, list, a, b), ac = ts_mid(N, E, run, urun, list, a, c), ad = ts_mid(N, E, run, urun, list, a, d);
    const long long bc = ts_mid(N, E, run, urun, list, b, c), bd = ts_mid(N, E, run, urun, list, b, d), cd = ts_mid(N, E, run, urun, list, c, d);
    const long long rows[8][4] = {{a, ab, ac, ad}, {b, bc, ab, bd}, {c, ac, bc, cd}, {d, ad, cd, bd}, {ab, ac, ad, bd}, {ab, ac, bd, bc}, {cd, ac, bd, ad}, {cd, ac, bc, bd}};
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const size_t row = (size_t)k * (size_t)F + f;
        longlong2* out = reinterpret_cast<longlong2*>(new_tets + 4 * row);
        out[0] = make_longlong2(rows[k][0], rows[k][1]);
        out[1] = make_longlong2(rows[k][2], rows[k][3]);
        sub_to_parent[row] = (long long)f;
    }
}

}  // namespace tgs

extern "C" {
#include "../../include/tgs_raster.h"

size_t tgs_tet_compact_workspace_bytes(int N, int F)
{
    tgs::TgCompactWork w;
    if (N < 0 || F < 0) return 0;
    return tgs::tg_compact_carve(w, nullptr, (size_t)N, (size_t)F);
}

int tgs_tet_compact_select(void* stream, int N, int F, const float* sdf, const void* tet, int tet_is_int64, const uint8_t* keep, float threshold, int64_t* counts,
                           void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (N < 0 || F < 0 || !counts || !workspace || (F > 0 && !tet) || (F > 0 && N > 0 && !sdf && !keep) || (tet_is_int64 != 0 && tet_is_int64 != 1) || !mt_aligned(tet))
        return set_error(TGS_ERR_INVALID, "tgs_tet_compact_select: N >= 0, F >= 0, tet_is_int64 in {0, 1} and non-NULL tet (16-byte aligned) / sdf or keep / counts / workspace required");
    TgCompactWork w;
    if (tg_compact_carve(w, (char*)workspace, (size_t)N, (size_t)F) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_tet_compact_select: workspace smaller than tgs_tet_compact_workspace_bytes(N, F)");
    const size_t words = tg_words((size_t)N) + 1;
    if (hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), st) != hipSuccess || hipMemsetAsync(w.bits, 0, words * sizeof(unsigned long long), st) != hipSuccess)
        return hip_status("tgs_tet_compact_select");
    if (F == 0) return TGS_OK;
    long long* cnt = (long long*)counts;
    if (tet_is_int64) hipLaunchKernelGGL(k_tg_select<long long>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, N, F, sdf, (const long long*)tet, keep, threshold, w.bits, w.kept, w.blk, cnt);
    else              hipLaunchKernelGGL(k_tg_select<int>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, N, F, sdf, (const int*)tet, keep, threshold, w.bits, w.kept, w.blk, cnt);
    run_scan(st, w.blk, run_blocks((size_t)F), w.scan, cnt + 0);
    hipLaunchKernelGGL(k_tg_popc, run_grid(words), dim3(RUN_BLOCK), 0, st, words, (const unsigned long long*)w.bits, w.wpre);
    run_scan(st, w.wpre, words, w.scan, cnt + 1);
    return hip_status("tgs_tet_compact_select");
}

int tgs_tet_compact_emit(void* stream, int N, int F, const void* tet, int tet_is_int64, int64_t n_tets, int64_t n_verts, const float* pos, const float* sdf,
                         const void* mask, int mask_type, const void* member_workspace, int out_is_int64, void* new_tets, void* new_tet_idx_to_old,
                         void* unique_vtx, float* new_pos, float* new_sdf, void* new_mask, int32_t* member, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (N <= 0 || F <= 0 || !tet || !mt_aligned(tet) || !workspace || (tet_is_int64 != 0 && tet_is_int64 != 1) || (out_is_int64 != 0 && out_is_int64 != 1) || n_tets <= 0 ||
        n_tets > F || n_verts <= 0 || n_verts > N || n_verts > 4 * n_tets || !new_tets || !new_tet_idx_to_old || !unique_vtx || (pos && !new_pos) || (sdf && !new_sdf) ||
        (mask && !new_mask) || (member_workspace && !member) || mask_type < TG_MASK_I32 || mask_type > TG_MASK_U8)
        return set_error(TGS_ERR_INVALID, "tgs_tet_compact_emit: N > 0, F > 0, 0 < n_tets <= F and 0 < n_verts <= min(N, 4 n_tets) as tgs_tet_compact_select counted them, "
                                          "tet_is_int64 / out_is_int64 in {0, 1}, mask_type in 0 .. 3, non-NULL tet (16-byte aligned) / new_tets / new_tet_idx_to_old / "
                                          "unique_vtx / workspace and an output for every given input required");
    TgCompactWork w, other;
    if (tg_compact_carve(w, (char*)workspace, (size_t)N, (size_t)F) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_tet_compact_emit: workspace smaller than tgs_tet_compact_workspace_bytes(N, F)");
    other.bits = nullptr;
    if (member_workspace) tg_compact_carve(other, (char*)member_workspace, (size_t)N, (size_t)F);
    const long long Fk = n_tets, Nk = n_verts;
#define TG_EMIT_TETS(I, O)                                                                                                                            \
    hipLaunchKernelGGL((k_tg_emit_tets<I, O>), run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, N, F, Fk, (const I*)tet, (const uint8_t*)w.kept, (const uint32_t*)w.blk, \
                       (const unsigned long long*)w.bits, (const uint32_t*)w.wpre, (O*)new_tets, (O*)new_tet_idx_to_old)
    if (tet_is_int64) { if (out_is_int64) TG_EMIT_TETS(long long, long long); else TG_EMIT_TETS(long long, int); }
    else              { if (out_is_int64) TG_EMIT_TETS(int, long long); else TG_EMIT_TETS(int, int); }
#undef TG_EMIT_TETS
    const int mbytes = tg_mask_bytes(mask_type);
    if (out_is_int64)
        hipLaunchKernelGGL(k_tg_emit_verts<long long>, run_grid((size_t)N), dim3(RUN_BLOCK), 0, st, N, Nk, (const unsigned long long*)w.bits, (const uint32_t*)w.wpre, pos, sdf, mask, mbytes,
                           (const unsigned long long*)other.bits, (long long*)unique_vtx, new_pos, new_sdf, new_mask, (int*)member);
    else
        hipLaunchKernelGGL(k_tg_emit_verts<int>, run_grid((size_t)N), dim3(RUN_BLOCK), 0, st, N, Nk, (const unsigned long long*)w.bits, (const uint32_t*)w.wpre, pos, sdf, mask, mbytes,
                           (const unsigned long long*)other.bits, (int*)unique_vtx, new_pos, new_sdf, new_mask, (int*)member);
    return hip_status("tgs_tet_compact_emit");
}

size_t tgs_tet_subdivide_workspace_bytes(int N, int F)
{
    tgs::TgSubdivWork w;
    if (N < 0 || F < 0 || F > tgs::TG_MAX_SUBDIV_F) return 0;
    return tgs::tg_subdiv_carve(w, nullptr, (size_t)N, (size_t)F);
}

int tgs_tet_subdivide_edges(void* stream, int N, int F, const void* tet, int tet_is_int64, int64_t* counts, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (N < 0 || F < 0 || F > TG_MAX_SUBDIV_F || !counts || !workspace || (F > 0 && !tet) || (tet_is_int64 != 0 && tet_is_int64 != 1) || !mt_aligned(tet))
        return set_error(TGS_ERR_INVALID, "tgs_tet_subdivide_edges: N >= 0, 0 <= F <= (2^31 - 1) / 8, tet_is_int64 in {0, 1} and non-NULL tet (16-byte aligned) / counts / workspace required");
    TgSubdivWork w;
    if (tg_subdiv_carve(w, (char*)workspace, (size_t)N, (size_t)F) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_tet_subdivide_edges: workspace smaller than tgs_tet_subdivide_workspace_bytes(N, F)");
    if (hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), st) != hipSuccess || hipMemsetAsync(w.run, 0, ((size_t)N + 1) * sizeof(uint32_t), st) != hipSuccess)
        return hip_status("tgs_tet_subdivide_edges");
    if (F == 0) return TGS_OK;
    long long* cnt = (long long*)counts;
    if (tet_is_int64) hipLaunchKernelGGL(k_ts_count<long long>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, N, F, (const long long*)tet, w.run, cnt);
    else              hipLaunchKernelGGL(k_ts_count<int>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, N, F, (const int*)tet, w.run, cnt);
    run_scan(st, w.run, (size_t)N + 1, w.scan, (long long*)nullptr);
    if (tet_is_int64) hipLaunchKernelGGL(k_ts_fill<long long>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, N, F, (const long long*)tet, w.run, w.list);
    else              hipLaunchKernelGGL(k_ts_fill<int>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, N, F, (const int*)tet, w.run, w.list);
    hipLaunchKernelGGL(k_ts_sort_unique, run_grid((size_t)N + 1), dim3(RUN_BLOCK), 0, st, N, F, (const uint32_t*)w.run, w.list, w.urun);
    run_scan(st, w.urun, (size_t)N + 1, w.scan, cnt + 0);
    return hip_status("tgs_tet_subdivide_edges");
}

int tgs_tet_subdivide_emit(void* stream, int N, int F, int B, int64_t E, const float* pos, const void* tet, int tet_is_int64, const void* mask, int mask_type,
                           float* new_v, int64_t* new_tets, float* new_mask, int64_t* sub_to_parent, int64_t* edges, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (N <= 0 || F <= 0 || F > TG_MAX_SUBDIV_F || B < 0 || B > 65535 || E <= 0 || E > 6ll * F || (long long)N + E > 0x7fffffffll || !tet || !mt_aligned(tet) || !workspace ||
        (tet_is_int64 != 0 && tet_is_int64 != 1) || mask_type < TG_MASK_I32 || mask_type > TG_MASK_U8 || !new_tets || !sub_to_parent || !edges || (B > 0 && (!pos || !new_v)) ||
        (mask && !new_mask))
        return set_error(TGS_ERR_INVALID, "tgs_tet_subdivide_emit: N > 0, 0 < F <= (2^31 - 1) / 8, 0 <= B < 65536, 0 < E <= 6 F as tgs_tet_subdivide_edges counted it, N + E < 2^31, "
                                          "tet_is_int64 in {0, 1}, mask_type in 0 .. 3 and non-NULL pos / tet (16-byte aligned) / new_v / new_tets / sub_to_parent / edges / "
                                          "workspace (new_mask with a mask) required");
    TgSubdivWork w;
    if (tg_subdiv_carve(w, (char*)workspace, (size_t)N, (size_t)F) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_tet_subdivide_emit: workspace smaller than tgs_tet_subdivide_workspace_bytes(N, F)");
    long long* ed = (long long*)edges;
    hipLaunchKernelGGL(k_ts_edges, run_grid((size_t)N), dim3(RUN_BLOCK), 0, st, N, (long long)E, (const uint32_t*)w.run, (const uint32_t*)w.urun, (const uint32_t*)w.list, ed);
    if (B > 0) {
        dim3 grid = run_grid((size_t)N + (size_t)E);
        grid.y = (unsigned)B;
        hipLaunchKernelGGL(k_ts_verts, grid, dim3(RUN_BLOCK), 0, st, N, (long long)E, pos, mask, mask_type, (const long long*)ed, new_v, new_mask);
    }
    if (tet_is_int64)
        hipLaunchKernelGGL(k_ts_tets<long long>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, N, F, (long long)E, (const long long*)tet, (const uint32_t*)w.run, (const uint32_t*)w.urun,
                           (const uint32_t*)w.list, (long long*)new_tets, (long long*)sub_to_parent);
    else
        hipLaunchKernelGGL(k_ts_tets<int>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, N, F, (long long)E, (const int*)tet, (const uint32_t*)w.run, (const uint32_t*)w.urun,
                           (const uint32_t*)w.list, (long long*)new_tets, (long long*)sub_to_parent);
    return hip_status("tgs_tet_subdivide_emit");
}
}
