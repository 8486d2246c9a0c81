// tgs_mesh_aa.hip -- the edge blend behind the mesh rasterizer: what tetgs_inpainter/mask_mesh_0822.py (:98, :139-141, :188, :356, :364) and
// tetgs_spatial/models/renderers/part_nvdiff_rasterizer.py (:108-191) ask of `antialias`, forward only, for gfx950.  Plain HIP, wave64, integer
// atomics in the topology build only, no float atomics anywhere.
//
// The rule (include/tgs_raster.h has it in full; tests/mesh_aa_ref.py restates it): every pair of horizontally or vertically adjacent pixels
// with two different triangle IDs takes the nearer triangle T (pixel P shows it, Q is the other one), looks for the first edge of T that the
// segment P -> Q leaves T through (all in int64 on the rasterizer's snapped coordinates), and if that edge is a silhouette (no neighbour, more
// than one, or a neighbour folded to T's side) blends by the crossing position t: a = t - 0.5 > 0 gives a (color[P] - color[Q]) to Q,
// a < 0 gives -a (color[Q] - color[P]) to P.
//
// Launches of tgs_mesh_antialias: k_aa_pairs (one lane per pixel analyses the pair with its right and its upper neighbour and writes two signed
// records: |a| with the receiving side in the sign, 0 for nothing) and k_aa_apply (one lane per output element gathers the four records around
// its pixel and adds the contributions in the fixed order left, right, below, above).  A pair is decided once, by one instruction sequence,
// so its two pixels cannot disagree; `color` is only read, so contributions never chain.  Neighbour IDs come by plain loads: the rows of
// `rast` are read coalesced and the right / upper neighbour's line is the lane's own or the one the wave above fetches (L1 / L2 hits); what a
// pair costs is its divergent analysis -- three dependent indexed reads (tri row, three pos rows, one topo entry) -- which an LDS tile of IDs
// would not shorten.
// Launches of tgs_mesh_topology: k_topo_clear, k_topo_insert (every edge of every usable triangle into the edge set of tgs_edge_set.hpp, keyed by
// its unordered vertex pair; on the key's slot: add for the count, min / max of the edge number 3 t + k), k_topo_resolve (count 1: -1,
// count 2: the opposite vertex of the other edge, which is the min or the max, more: -2).  Count, min and max do not depend on the order the
// lanes arrive in; the slot a key lands in does, but no output reads it.
#include "tgs_mesh_aa_pair.hpp"
#define TGS_EDGE_SET_TABLE_ONLY                                         // no runs here: count, min and max stay on the slot
#include "tgs_edge_set.hpp"                                             // the key, the hash, the insert and the lookup

namespace tgs {

struct TopoWork {
    unsigned long long* keys;             // [cap] (lo << 32 | hi) of the edge's vertex pair
    uint32_t* count;                      // [cap] edges with this key
    uint32_t* emin;                       // [cap] smallest and
    uint32_t* emax;                       // [cap] largest edge number 3 t + k among them
};
__host__ __device__ inline size_t topo_capacity(size_t F)
{
    size_t cap = 64;                                                              // a power of two >= 4 F: at most 3 F keys, load <= 3/4
    while (cap < 4 * F) cap <<= 1;
    return cap;
}
__host__ __device__ inline size_t topo_carve(TopoWork& w, char* base, size_t cap)
{
    char* p = base;
    carve(p, w.keys, cap); carve(p, w.count, cap); carve(p, w.emin, cap); carve(p, w.emax, cap);
    return (size_t)(p - base) + 256;
}

// usable as a neighbour: three different indices inside [0, V)
__device__ __forceinline__ bool topo_usable(int V, const int* __restrict__ tri, int t, int idx[3])
{
    idx[0] = tri[3 * (size_t)t]; idx[1] = tri[3 * (size_t)t + 1]; idx[2] = tri[3 * (size_t)t + 2];
    return (unsigned)idx[0] < (unsigned)V && (unsigned)idx[1] < (unsigned)V && (unsigned)idx[2] < (unsigned)V &&
           idx[0] != idx[1] && idx[1] != idx[2] && idx[2] != idx[0];
}
__device__ __forceinline__ unsigned long long topo_key(int a, int b)
{
    return edge_key((uint32_t)min(a, b), (uint32_t)max(a, b));
}

__global__ __launch_bounds__(256) void k_topo_clear(size_t cap, TopoWork w)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    w.keys[i] = EDGE_EMPTY; w.count[i] = 0u; w.emin[i] = 0xffffffffu; w.emax[i] = 0u;
}

__global__ __launch_bounds__(256) void k_topo_insert(int V, int F, const int* __restrict__ tri, size_t cap, TopoWork w)
{
    const int e = blockIdx.x * 256 + threadIdx.x;                                 // edge number 3 t + k < 3 * 2^24
    if (e >= 3 * F) return;
    const int t = e / 3, k = e - 3 * t;
    int idx[3];
    if (!topo_usable(V, tri, t, idx)) return;
    const unsigned long long key = topo_key(idx[k], idx[(k + 1) % 3]);
    bool claimed;
    const size_t slot = edge_insert(w.keys, cap, key, claimed);
    if (slot == EDGE_ABSENT) return;                                              // (never: the table is never full)
    atomicAdd(&w.count[slot], 1u);                                                // on the key's slot, whoever claimed it
    atomicMin(&w.emin[slot], (uint32_t)e);
    atomicMax(&w.emax[slot], (uint32_t)e);
}

__global__ __launch_bounds__(256) void k_topo_resolve(int V, int F, const int* __restrict__ tri, size_t cap, TopoWork w, int* __restrict__ topo)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * F) return;
    const int t = e / 3, k = e - 3 * t;
    int idx[3];
    int res = TOPO_NONE;
    if (topo_usable(V, tri, t, idx)) {
        const unsigned long long key = topo_key(idx[k], idx[(k + 1) % 3]);
        const size_t slot = edge_find(w.keys, cap, key);
        if (slot != EDGE_ABSENT) {                                                // (always: the edge was inserted by the launch before)
            const uint32_t n = w.count[slot];
            if (n > 2u) res = TOPO_MANY;
            else if (n == 2u) {
                const uint32_t lo = w.emin[slot], hi = w.emax[slot];
                const uint32_t other = lo == (uint32_t)e ? hi : lo;                // < 3 F: it was written by an edge of this launch
                const uint32_t ot = other / 3u, oe = other - 3u * ot;
                res = tri[3 * (size_t)ot + (oe + 2u) % 3u];
            }
        }
    }
    topo[e] = res;
}

// ---- antialias ------------------------------------------------------------------------------------------------------------------------
// The whole decision of one pair is aa_pair_full (tgs_mesh_aa_pair.hpp: the backward of tgs_mesh_grad.hip replays it); the forward keeps its
// record: +|a| the second pixel receives |a| (color[first] - color[second]), -|a| the first receives |a| (color[second] - color[first]),
// 0 nothing.
__global__ __launch_bounds__(256) void k_aa_pairs(int V, int F, const float4* __restrict__ pos, const int* __restrict__ tri, const int* __restrict__ topo,
                                                  int W, int H, const float4* __restrict__ rast, float* __restrict__ rec_h, float* __restrict__ rec_v)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)W * H) return;
    AaPair pr[2] = {aa_no_pair(), aa_no_pair()};
    aa_pixel_pairs(V, F, pos, tri, topo, W, H, rast, p, pr);
    rec_h[p] = pr[0].rec; rec_v[p] = pr[1].rec;
}

// out = (((color + left) + right) + below) + above, every contribution |a| (color[other] - color[self]) rounded on its own
__global__ __launch_bounds__(256) void k_aa_apply(int C, int W, int H, long long n_elems, const float* __restrict__ color, const float* __restrict__ rec_h,
                                                  const float* __restrict__ rec_v, float* __restrict__ out)
{
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_elems) return;
    const long long p = e / C;
    const int j = (int)(p / W), i = (int)(p - (long long)j * W);
    const float self = color[e];
    float res = self;
    const long long row = (long long)W * C;
    if (i > 0)     { const float r = rec_h[p - 1]; if (r > 0.f) res += r * (color[e - C] - self); }
    if (i + 1 < W) { const float r = rec_h[p];     if (r < 0.f) res += -r * (color[e + C] - self); }
    if (j > 0)     { const float r = rec_v[p - W]; if (r > 0.f) res += r * (color[e - row] - self); }
    if (j + 1 < H) { const float r = rec_v[p];     if (r < 0.f) res += -r * (color[e + row] - self); }
    out[e] = res;
}

struct AaWork { float* rec_h; float* rec_v; };
__host__ __device__ inline size_t aa_carve(AaWork& w, char* base, size_t N)
{
    char* p = base;
    carve(p, w.rec_h, N); carve(p, w.rec_v, N);
    return (size_t)(p - base) + 256;
}

}  // namespace tgs

extern "C" {
#include "../../include/tgs_raster.h"

size_t tgs_mesh_topology_workspace_bytes(int F)
{
    tgs::TopoWork w;
    if (!tgs::mesh_faces_ok(F)) return 0;
    return tgs::topo_carve(w, nullptr, tgs::topo_capacity((size_t)F));
}

int tgs_mesh_topology(void* stream, int V, int F, const int32_t* tri, int32_t* topo, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (V < 0 || !mesh_faces_ok(F) || !workspace || (F > 0 && (!tri || !topo)))
        return set_error(TGS_ERR_INVALID, "tgs_mesh_topology: V >= 0, 0 <= F < 2^24 and non-NULL tri / topo / workspace required");
    TopoWork w;
    const size_t cap = topo_capacity((size_t)F);
    if (topo_carve(w, (char*)workspace, cap) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_mesh_topology: workspace smaller than tgs_mesh_topology_workspace_bytes(F)");
    if (F == 0) return TGS_OK;
    const dim3 blk(256), egrid((unsigned)((3 * (size_t)F + 255) / 256));
    hipLaunchKernelGGL(k_topo_clear, dim3((unsigned)((cap + 255) / 256)), blk, 0, st, cap, w);
    hipLaunchKernelGGL(k_topo_insert, egrid, blk, 0, st, V, F, tri, cap, w);
    hipLaunchKernelGGL(k_topo_resolve, egrid, blk, 0, st, V, F, tri, cap, w, topo);
    return hip_status("tgs_mesh_topology");
}

size_t tgs_mesh_antialias_workspace_bytes(int width, int height)
{
    tgs::AaWork w;
    if (!tgs::mesh_dims_ok(width, height)) return 0;
    return tgs::aa_carve(w, nullptr, (size_t)width * (size_t)height);
}

int tgs_mesh_antialias(void* stream, int V, int F, int C, const float* pos, const int32_t* tri, const int32_t* topo, int width, int height, const float* rast,
                       const float* color, float* out, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (V < 0 || !mesh_faces_ok(F) || C < 1 || !mesh_dims_ok(width, height) || !rast || !color || !out || !workspace ||
        (F > 0 && V > 0 && (!pos || !tri || !topo)))
        return set_error(TGS_ERR_INVALID, "tgs_mesh_antialias: V >= 0, 0 <= F < 2^24, C >= 1, 1 <= width, height <= 8192 and non-NULL pos / tri / topo / rast / color / "
                                          "out / workspace required");
    if (out == color) return set_error(TGS_ERR_INVALID, "tgs_mesh_antialias: out may not alias color (every pixel reads its neighbours' colours)");
    const size_t N = (size_t)width * (size_t)height;
    if ((long long)N > MESH_MAX_ELEMS / C) return set_error(TGS_ERR_INVALID, "tgs_mesh_antialias: width * height * C too large for one launch");
    AaWork w;
    if (aa_carve(w, (char*)workspace, N) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_mesh_antialias: workspace smaller than tgs_mesh_antialias_workspace_bytes(width, height)");
    const long long n_elems = (long long)N * C;
    if (F == 0 || V == 0) {                                                       // no ID names a triangle: a copy
        if (hipMemcpyAsync(out, color, (size_t)n_elems * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return hip_status("tgs_mesh_antialias");
        return TGS_OK;
    }
    const dim3 blk(256);
    hipLaunchKernelGGL(k_aa_pairs, dim3((unsigned)((N + 255) / 256)), blk, 0, st, V, F, (const float4*)pos, tri, topo, width, height, (const float4*)rast, w.rec_h, w.rec_v);
    hipLaunchKernelGGL(k_aa_apply, dim3((unsigned)((n_elems + 255) / 256)), blk, 0, st, C, width, height, n_elems, color, w.rec_h, w.rec_v, out);
    return hip_status("tgs_mesh_antialias");
}
}
