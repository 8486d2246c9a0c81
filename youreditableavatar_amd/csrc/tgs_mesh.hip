// tgs_mesh.hip -- forward-only triangle rasterizer for the inpainter's mesh masks: what tetgs_inpainter/mask_mesh_0822.py asks of its
// third-party rasterizer (`rasterize` + `interpolate`, :94-134, :183-188, :350-364), for gfx950.  Plain HIP, wave64, integer atomics only.
//
// The rule (include/tgs_raster.h has it in full; tests/mesh_ref.py restates it in integers):
//   * vertices are snapped to a 1/256-pixel grid, X = rint((x/w * 0.5 + 0.5) * W * 256); pixel (i, j) has its centre at (256 i + 128, 256 j + 128);
//   * a triangle with a vertex at w <= 0, a non-finite coordinate or |X|, |Y| > 2^29 is dropped whole (no clipping);
//   * coverage is decided in int64 on the snapped vertices: the triangle is oriented so that its area is positive, a pixel is inside an
//     edge a->b when E > 0, or E == 0 and the edge owns its boundary (dy < 0, or dy == 0 and dx > 0) -- an edge and its reverse are never both
//     owners, so a shared edge gives every pixel on it to exactly one of its two triangles;
//   * depth z/w is linear in screen space, from the unsnapped coordinates; fragments outside [-1, 1] are discarded; the smallest depth wins,
//     the lower triangle index on equal bits: ONE 64-bit unsigned atomicMin on (order-preserving depth bits << 32 | index) per fragment, which
//     does not depend on the order the triangles arrive in.
//   * u, v are the perspective-correct barycentrics of vertices 0 and 1, clamped to [0, 1] and divided by max(u + v, 1).
// All float arithmetic of a fragment is written once (mesh_frag), contraction off: the coverage kernels and the resolve kernel round alike,
// and tests/mesh_ref.py evaluates the same sequence in float32 to measure its noise.
//
// Launches: k_mesh_clear (keys <- all ones, counter <- 0), k_mesh_small (one lane per triangle: a box of at most MESH_SMALL x MESH_SMALL
// pixels is walked by the lane itself, one of at most MESH_MEDIUM a side by the triangle's whole wave, anything larger is appended to a
// list with its number of MESH_REGION^2-pixel screen regions), k_mesh_large (persistent workgroups over the flattened (large triangle,
// region) items; a region is walked in 8x8-pixel blocks, one lane per pixel, four blocks per wave), k_mesh_resolve (one lane per pixel).
// No lane walks an unbounded box, and a screen-filling triangle becomes (W / 32) x (H / 32) independent items.
#include "tgs_mesh_snap.hpp"

namespace tgs {

constexpr int MESH_SMALL = 4;             // boxes up to this many pixels a side are walked by the triangle's own lane
constexpr int MESH_MEDIUM = 32;           // boxes up to this many pixels a side are walked by the triangle's wave
constexpr int MESH_REGION = 32;           // a work item of the large path: one workgroup, 16 blocks of 8x8 pixels
constexpr int MESH_LARGE_WGS = 2048;      // persistent workgroups of k_mesh_large
constexpr unsigned long long MESH_EMPTY = ~0ull;
constexpr unsigned long long MESH_ITEM_MASK = (1ull << 40) - 1ull;

struct MeshWork {
    unsigned long long* keys;             // [W*H] winner per pixel
    unsigned long long* counter;          // large triangles << 40 | items (one atomicAdd hands out both, so item offsets ascend with the slot)
    unsigned long long* item0;            // [F] first item of the large triangle in this slot
    uint32_t* ltri;                       // [F] its triangle index
};
__host__ __device__ inline size_t mesh_carve(MeshWork& w, char* base, size_t F, size_t N)
{
    char* p = base;
    carve(p, w.keys, N); carve(p, w.counter, 1); carve(p, w.item0, F); carve(p, w.ltri, F);
    return (size_t)(p - base) + 256;
}

struct MeshTri {
    int X[3], Y[3];                       // snapped, ORIENTED: positive area (vertices 1 and 2 swapped for the other winding)
    int bx0, by0, bx1, by1;               // pixels whose centre can be inside, clamped to the screen (empty: bx0 > bx1 or by0 > by1)
    float s0x, s0y, e1x, e1y, e2x, e2y, inv_area;     // screen position of vertex 0, edges to vertices 1 and 2 (pixels, unsnapped, input order)
    float zw0, dz1, dz2, iw0, iw1, iw2;
};

__device__ __forceinline__ int floor_div256(int a) { return a >> 8; }              // arithmetic shift: floor for negative a as well

// Everything about triangle t that does not depend on the pixel.  false: the triangle produces nothing.
__device__ __forceinline__ bool mesh_setup(int V, const float4* __restrict__ pos, const int* __restrict__ tri, int t, int W, int H, MeshTri& s)
{
#pragma clang fp contract(off)
    const int i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return false;       // nothing is read through a bad index
    const float4 p[3] = {pos[i0], pos[i1], pos[i2]};
    float sx[3], sy[3], zw[3], iw[3];
    int X[3], Y[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (!mesh_snap(p[k], W, H, sx[k], sy[k], X[k], Y[k])) return false;
        zw[k] = p[k].z / p[k].w;
        iw[k] = 1.0f / p[k].w;
    }
    const long long A = (long long)(X[1] - X[0]) * (long long)(Y[2] - Y[0]) - (long long)(X[2] - X[0]) * (long long)(Y[1] - Y[0]);
    if (A == 0) return false;
    const bool ccw = A > 0;
    s.X[0] = X[0]; s.Y[0] = Y[0];
    s.X[1] = ccw ? X[1] : X[2]; s.Y[1] = ccw ? Y[1] : Y[2];
    s.X[2] = ccw ? X[2] : X[1]; s.Y[2] = ccw ? Y[2] : Y[1];
    const int xmin = min(X[0], min(X[1], X[2])), xmax = max(X[0], max(X[1], X[2]));
    const int ymin = min(Y[0], min(Y[1], Y[2])), ymax = max(Y[0], max(Y[1], Y[2]));
    s.bx0 = max(0, floor_div256(xmin - 128 + 255)); s.bx1 = min(W - 1, floor_div256(xmax - 128));
    s.by0 = max(0, floor_div256(ymin - 128 + 255)); s.by1 = min(H - 1, floor_div256(ymax - 128));
    if (s.bx0 > s.bx1 || s.by0 > s.by1) return false;
    s.s0x = sx[0]; s.s0y = sy[0];
    s.e1x = sx[1] - sx[0]; s.e1y = sy[1] - sy[0];
    s.e2x = sx[2] - sx[0]; s.e2y = sy[2] - sy[0];
    const float area = s.e1x * s.e2y - s.e1y * s.e2x;
    s.inv_area = 1.0f / area;
    s.zw0 = zw[0]; s.dz1 = zw[1] - zw[0]; s.dz2 = zw[2] - zw[0];
    s.iw0 = iw[0]; s.iw1 = iw[1]; s.iw2 = iw[2];
    return true;
}

// E >= 0 for an owning edge, E >= 1 for the other kind: the integer form of "E > 0, or E == 0 and the edge owns its boundary"
__device__ __forceinline__ bool mesh_inside_edge(int Xa, int Ya, int Xb, int Yb, int Px, int Py)
{
    const int dx = Xb - Xa, dy = Yb - Ya;
    const long long E = (long long)dx * (long long)(Py - Ya) - (long long)dy * (long long)(Px - Xa);
    const bool owner = dy < 0 || (dy == 0 && dx > 0);
    return E >= (owner ? 0ll : 1ll);
}
__device__ __forceinline__ bool mesh_covers(const MeshTri& s, int i, int j)
{
    const int Px = 256 * i + 128, Py = 256 * j + 128;
    return mesh_inside_edge(s.X[0], s.Y[0], s.X[1], s.Y[1], Px, Py) && mesh_inside_edge(s.X[1], s.Y[1], s.X[2], s.Y[2], Px, Py) &&
           mesh_inside_edge(s.X[2], s.Y[2], s.X[0], s.Y[0], Px, Py);
}

// The float part of a fragment: screen-space barycentrics of vertices 1 and 2 at the centre of pixel (i, j), and z/w
__device__ __forceinline__ void mesh_frag(const MeshTri& s, int i, int j, float& b1, float& b2, float& zw)
{
#pragma clang fp contract(off)
    const float px = ((float)i + 0.5f) - s.s0x, py = ((float)j + 0.5f) - s.s0y;
    b1 = (px * s.e2y - py * s.e2x) * s.inv_area;
    b2 = (s.e1x * py - s.e1y * px) * s.inv_area;
    zw = (s.zw0 + b1 * s.dz1) + b2 * s.dz2;
}
__device__ __forceinline__ void mesh_uv(const MeshTri& s, float b1, float b2, float& u, float& v)
{
#pragma clang fp contract(off)
    const float b0 = (1.0f - b1) - b2;
    const float q0 = b0 * s.iw0, q1 = b1 * s.iw1, q2 = b2 * s.iw2;
    const float d = (q0 + q1) + q2;
    u = fminf(fmaxf(q0 / d, 0.f), 1.f);
    v = fminf(fmaxf(q1 / d, 0.f), 1.f);
    const float sum = fmaxf(u + v, 1.0f);
    u = u / sum; v = v / sum;
}

// float bits -> unsigned that orders like the float (negative values below positive ones)
__device__ __forceinline__ uint32_t mesh_order_bits(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float mesh_unorder_bits(uint32_t o)
{
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__device__ __forceinline__ void mesh_fragment(const MeshTri& s, int t, int i, int j, int W, unsigned long long* __restrict__ keys)
{
    if (!mesh_covers(s, i, j)) return;
    float b1, b2, zw;
    mesh_frag(s, i, j, b1, b2, zw);
    if (!(zw >= -1.0f && zw <= 1.0f)) return;                                     // (NaN: discarded)
    const unsigned long long key = ((unsigned long long)mesh_order_bits(zw) << 32) | (uint32_t)t;
    unsigned long long* dst = keys + (size_t)j * W + i;
    // keys only ever decrease during the pass: a fragment that loses against what a plain load sees loses against the final value too
    if (key < *dst) atomicMin(dst, key);
}

__global__ __launch_bounds__(256) void k_mesh_clear(size_t n, unsigned long long* keys, unsigned long long* counter)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = MESH_EMPTY;
    if (i == 0) *counter = 0ull;
}

// triangle setup of lane k (wave-uniform k) in every lane
__device__ __forceinline__ int mesh_lane_i(int v, int k) { return __builtin_amdgcn_readlane(v, k); }
__device__ __forceinline__ float mesh_lane_f(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }
__device__ __forceinline__ MeshTri mesh_of_lane(const MeshTri& s, int k)
{
    MeshTri r;
#pragma unroll
    for (int e = 0; e < 3; e++) { r.X[e] = mesh_lane_i(s.X[e], k); r.Y[e] = mesh_lane_i(s.Y[e], k); }
    r.bx0 = mesh_lane_i(s.bx0, k); r.by0 = mesh_lane_i(s.by0, k); r.bx1 = mesh_lane_i(s.bx1, k); r.by1 = mesh_lane_i(s.by1, k);
    r.s0x = mesh_lane_f(s.s0x, k); r.s0y = mesh_lane_f(s.s0y, k); r.e1x = mesh_lane_f(s.e1x, k); r.e1y = mesh_lane_f(s.e1y, k);
    r.e2x = mesh_lane_f(s.e2x, k); r.e2y = mesh_lane_f(s.e2y, k); r.inv_area = mesh_lane_f(s.inv_area, k);
    r.zw0 = mesh_lane_f(s.zw0, k); r.dz1 = mesh_lane_f(s.dz1, k); r.dz2 = mesh_lane_f(s.dz2, k);
    r.iw0 = mesh_lane_f(s.iw0, k); r.iw1 = mesh_lane_f(s.iw1, k); r.iw2 = mesh_lane_f(s.iw2, k);
    return r;
}

// One lane per triangle: every lane sets its triangle up, then
//   large  (a box wider or taller than MESH_MEDIUM pixels): appended to the list, ONE atomic per wave (ballot, a wave scan of the item
//          counts, the leader adds the wave's totals, every lane takes its rank);
//   medium (more than MESH_SMALL, at most MESH_MEDIUM a side): walked by the whole wave, one after the other, in 8x8-pixel blocks with one
//          lane per pixel -- the setup is already in the owner's registers and reaches the other lanes by v_readlane, so a medium triangle
//          costs no memory round trip of its own (as a list walked one wave per triangle it was three dependent ones: 192 us for the
//          sphere of tools/mesh_raster_loop.py at 2048^2, where half of the visible faces are 5 pixels wide);
//   small  walked by its own lane.
// No lane leaves before the wave-level steps: they see all 64 lanes.
__global__ __launch_bounds__(256) void k_mesh_small(int V, int F, const float4* __restrict__ pos, const int* __restrict__ tri, int W, int H, MeshWork w)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    MeshTri s = {};
    const bool ok = t < F && mesh_setup(V, pos, tri, t, W, H, s);
    const int bw = ok ? s.bx1 - s.bx0 + 1 : 0, bh = ok ? s.by1 - s.by0 + 1 : 0;
    const bool small = ok && bw <= MESH_SMALL && bh <= MESH_SMALL;
    const bool medium = ok && !small && bw <= MESH_MEDIUM && bh <= MESH_MEDIUM;
    const bool large = ok && !small && !medium;
    {
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(large);
        if (bal != 0ull) {                                                        // (wave-uniform)
            const unsigned long long items = large ? (unsigned long long)(s.bx1 / MESH_REGION - s.bx0 / MESH_REGION + 1) *
                                                     (unsigned long long)(s.by1 / MESH_REGION - s.by0 / MESH_REGION + 1) : 0ull;
            const unsigned long long incl = wave_iscan_u64(items, lane);
            const unsigned long long total = __shfl(incl, 63, 64);
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            const int leader = __builtin_ctzll(bal);
            unsigned long long old = 0ull;
            if (lane == leader) old = atomicAdd(w.counter, ((unsigned long long)__builtin_popcountll(bal) << 40) + total);
            old = __shfl(old, leader, 64);
            if (large) {
                const size_t slot = (size_t)(old >> 40) + rank;                   // < F: every triangle is appended at most once
                w.item0[slot] = (old & MESH_ITEM_MASK) + (incl - items);          // ascends with the slot, inside the wave as between waves
                w.ltri[slot] = (uint32_t)t;
            }
        }
    }
    for (unsigned long long mb = __builtin_amdgcn_ballot_w64(medium); mb != 0ull; mb &= mb - 1ull) {
        const int k = __builtin_ctzll(mb);
        const MeshTri m = mesh_of_lane(s, k);
        const int tk = t - lane + k;
        for (int by = m.by0 >> 3; by <= (m.by1 >> 3); by++)
            for (int bx = m.bx0 >> 3; bx <= (m.bx1 >> 3); bx++) {
                const int i = 8 * bx + (lane & 7), j = 8 * by + (lane >> 3);
                if (i >= m.bx0 && i <= m.bx1 && j >= m.by0 && j <= m.by1) mesh_fragment(m, tk, i, j, W, w.keys);
            }
    }
    if (small)
        for (int j = s.by0; j <= s.by1; j++)
            for (int i = s.bx0; i <= s.bx1; i++) mesh_fragment(s, t, i, j, W, w.keys);
}

__global__ __launch_bounds__(256) void k_mesh_large(int V, const float4* __restrict__ pos, const int* __restrict__ tri, int W, int H, MeshWork w)
{
    const unsigned long long c = *w.counter;
    const unsigned long long total = c & MESH_ITEM_MASK;
    const uint32_t nlarge = (uint32_t)(c >> 40);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (unsigned long long item = blockIdx.x; item < total; item += gridDim.x) {
        // the last slot whose first item is not behind `item` (item0 ascends with the slot; item0[0] == 0)
        uint32_t lo = 0, hi = nlarge;
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (w.item0[mid] <= item) lo = mid; else hi = mid;
        }
        const int t = (int)w.ltri[lo];
        MeshTri s;
        if (!mesh_setup(V, pos, tri, t, W, H, s)) continue;                       // (it passed in k_mesh_small: never taken)
        const uint32_t local = (uint32_t)(item - w.item0[lo]);
        const uint32_t rx0 = (uint32_t)(s.bx0 / MESH_REGION), nrx = (uint32_t)(s.bx1 / MESH_REGION) - rx0 + 1u;
        const int ox = (int)(rx0 + local % nrx) * MESH_REGION, oy = (int)((uint32_t)(s.by0 / MESH_REGION) + local / nrx) * MESH_REGION;
        for (int b = wave; b < 16; b += 4) {                                      // 4 x 4 blocks of 8 x 8 pixels
            const int x0 = ox + 8 * (b & 3), y0 = oy + 8 * (b >> 2);
            if (x0 > s.bx1 || x0 + 7 < s.bx0 || y0 > s.by1 || y0 + 7 < s.by0) continue;       // (wave-uniform)
            const int i = x0 + (lane & 7), j = y0 + (lane >> 3);
            if (i >= s.bx0 && i <= s.bx1 && j >= s.by0 && j <= s.by1) mesh_fragment(s, t, i, j, W, w.keys);
        }
    }
}

__global__ __launch_bounds__(256) void k_mesh_resolve(int V, int F, const float4* __restrict__ pos, const int* __restrict__ tri, int W, int H,
                                                      const unsigned long long* __restrict__ keys, float4* __restrict__ rast)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)W * H) return;
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    const unsigned long long key = keys[p];
    const uint32_t t = (uint32_t)key;
    MeshTri s;
    if (key != MESH_EMPTY && t < (uint32_t)F && mesh_setup(V, pos, tri, (int)t, W, H, s)) {
        const int j = (int)(p / (size_t)W), i = (int)(p - (size_t)j * W);
        float b1, b2, zw, u, v;
        mesh_frag(s, i, j, b1, b2, zw);
        mesh_uv(s, b1, b2, u, v);
        out = make_float4(u, v, mesh_unorder_bits((uint32_t)(key >> 32)), (float)(t + 1u));      // the depth the fragment won with (the same bits as zw)
    }
    rast[p] = out;
}

// out[p, c] = u a0 + v a1 + (1 - u - v) a2 of triangle id - 1; exactly 0 where id == 0 (or names no triangle / no vertex)
__global__ __launch_bounds__(256) void k_mesh_interpolate(int V, int F, int C, const float* __restrict__ attr, const int* __restrict__ tri, long long n_elems,
                                                          const float4* __restrict__ rast, float* __restrict__ out)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_elems) return;
    const long long p = e / C;
    const int c = (int)(e - p * C);
    const float4 r = rast[p];
    float res = 0.f;
    int idx[3];
    if (mesh_pixel_triangle(r.w, F, V, tri, idx) >= 0) {
        // in double, rounded once: where u + v is close to 1 the float subtraction's rounding, times a large a2, would exceed the sum of
        // the three products' own roundings (the kernel moves 16 + 4 C bytes per pixel: the arithmetic is free)
        const double u = (double)r.x, v = (double)r.y;
        res = (float)(u * (double)attr[(size_t)idx[0] * C + c] + v * (double)attr[(size_t)idx[1] * C + c] + (1.0 - u - v) * (double)attr[(size_t)idx[2] * C + c]);
    }
    out[e] = res;
}

}  // namespace tgs

extern "C" {
#include "../../include/tgs_raster.h"

size_t tgs_mesh_workspace_bytes(int F, int width, int height)
{
    tgs::MeshWork w;
    if (F < 0 || !tgs::mesh_dims_ok(width, height)) return 0;
    return tgs::mesh_carve(w, nullptr, (size_t)F, (size_t)width * (size_t)height);
}

int tgs_mesh_rasterize(void* stream, int V, int F, const float* pos, const int32_t* tri, int width, int height, float* rast, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (V < 0 || !mesh_faces_ok(F) || !mesh_dims_ok(width, height) || !rast || !workspace || (F > 0 && (!tri || (V > 0 && !pos))))
        return set_error(TGS_ERR_INVALID, "tgs_mesh_rasterize: V >= 0, 0 <= F < 2^24, 1 <= width, height <= 8192 and non-NULL pos / tri / rast / workspace required");
    MeshWork w;
    const size_t N = (size_t)width * (size_t)height;
    if (mesh_carve(w, (char*)workspace, (size_t)F, N) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_mesh_rasterize: workspace smaller than tgs_mesh_workspace_bytes(F, width, height)");
    const dim3 pgrid((unsigned)((N + 255) / 256)), blk(256);
    hipLaunchKernelGGL(k_mesh_clear, pgrid, blk, 0, st, N, w.keys, w.counter);
    if (F > 0 && V > 0) {
        hipLaunchKernelGGL(k_mesh_small, dim3((unsigned)((F + 255) / 256)), blk, 0, st, V, F, (const float4*)pos, tri, width, height, w);
        hipLaunchKernelGGL(k_mesh_large, dim3(MESH_LARGE_WGS), blk, 0, st, V, (const float4*)pos, tri, width, height, w);
    }
    hipLaunchKernelGGL(k_mesh_resolve, pgrid, blk, 0, st, V, F, (const float4*)pos, tri, width, height, w.keys, (float4*)rast);
    return hip_status("tgs_mesh_rasterize");
}

int tgs_mesh_interpolate(void* stream, int V, int F, int C, const float* attr, const int32_t* tri, int64_t n_pixels, const float* rast, float* out)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (n_pixels == 0) return TGS_OK;
    if (V < 0 || F < 0 || C < 1 || n_pixels < 0 || !rast || !out || (F > 0 && V > 0 && (!attr || !tri)))
        return set_error(TGS_ERR_INVALID, "tgs_mesh_interpolate: V, F >= 0, C >= 1, n_pixels >= 0 and non-NULL attr / tri / rast / out required");
    if (n_pixels > MESH_MAX_ELEMS / C) return set_error(TGS_ERR_INVALID, "tgs_mesh_interpolate: n_pixels * C too large for one launch");
    const long long n_elems = (long long)n_pixels * C;
    // (F == 0 or V == 0: no ID names a triangle, the kernel writes zeros and reads neither attr nor tri)
    hipLaunchKernelGGL(k_mesh_interpolate, dim3((unsigned)((n_elems + 255) / 256)), dim3(256), 0, st, V, V > 0 ? F : 0, C, attr, tri, n_elems, (const float4*)rast, out);
    return hip_status("tgs_mesh_interpolate");
}
}
