// tgs_mesh_snap.hpp -- what the mesh rasterizer's three files (tgs_mesh.hip, tgs_mesh_aa.hip, tgs_mesh_grad.hip) share, each written once: the
// limits and the entry points' range tests, the snapping of one clip-space vertex (all of them decide in integers on the SAME snapped
// coordinates, so the float sequence that produces them stands here), and the interpolate rule's decode of a pixel's triangle ID.
#pragma once
#include "tgs_device.hpp"

namespace tgs {

constexpr int MESH_MAX_DIM = 8192;        // width / height: (8192 / 32)^2 = 2^16 regions, times < 2^24 triangles, fits the 40-bit item count
constexpr int MESH_MAX_FACES = (1 << 24) - 1;     // the triangle ID travels in a float
constexpr float MESH_SNAP_MAX = 536870912.0f;     // 2^29
constexpr long long MESH_MAX_ELEMS = 0x7fffffffll * 256;      // pixels * channels of one launch: one lane per element, 256 lanes per workgroup

// host: the ranges the entry points test before anything else
inline bool mesh_dims_ok(int width, int height) { return width > 0 && height > 0 && width <= MESH_MAX_DIM && height <= MESH_MAX_DIM; }
inline bool mesh_faces_ok(int F) { return F >= 0 && F <= MESH_MAX_FACES; }
inline bool mesh_pixels_ok(long long n_pixels) { return n_pixels >= 0 && n_pixels <= (long long)MESH_MAX_DIM * MESH_MAX_DIM; }

__device__ __forceinline__ bool mesh_finite4(float4 p)
{
    return fabsf(p.x) <= 3.4028234e38f && fabsf(p.y) <= 3.4028234e38f && fabsf(p.z) <= 3.4028234e38f && fabsf(p.w) <= 3.4028234e38f;      // (false for NaN)
}

// The `ok` test of a vertex and its snap: screen position (sx, sy) in pixels, (X, Y) on the 1/256-pixel grid.  false: w <= 0, a non-finite
// coordinate, or |X| or |Y| above 2^29 (nothing is written that may be used).
__device__ __forceinline__ bool mesh_snap(float4 p, int W, int H, float& sx, float& sy, int& X, int& Y)
{
#pragma clang fp contract(off)
    if (!mesh_finite4(p) || !(p.w > 0.f)) return false;
    sx = (p.x / p.w * 0.5f + 0.5f) * (float)W;
    sy = (p.y / p.w * 0.5f + 0.5f) * (float)H;
    const float fx = rintf(sx * 256.0f), fy = rintf(sy * 256.0f);
    if (!(fabsf(fx) <= MESH_SNAP_MAX) || !(fabsf(fy) <= MESH_SNAP_MAX)) return false;
    X = (int)fx; Y = (int)fy;
    return true;
}

// The interpolate rule's decode of a pixel's ID (rast.w), forward and backward: -> t = id - 1 when 1 <= id <= F and the three indices of triangle t,
// which idx receives, lie in [0, V); else -1 (nothing may be read through idx).  Antialias decodes by its own rule, aa_id of tgs_mesh_aa_pair.hpp.
__device__ __forceinline__ int mesh_pixel_triangle(float id, int F, int V, const int* __restrict__ tri, int idx[3])
{
    int t = -1;
    if (id >= 1.0f && id <= (float)F) {
        const size_t tt = (size_t)((int)id - 1);
        __builtin_assume((int)tt >= 0);                                           // (id >= 1: a caller's `t >= 0` is the two tests here, not a third)
        idx[0] = tri[3 * tt]; idx[1] = tri[3 * tt + 1]; idx[2] = tri[3 * tt + 2];
        if ((unsigned)idx[0] < (unsigned)V && (unsigned)idx[1] < (unsigned)V && (unsigned)idx[2] < (unsigned)V) t = (int)tt;
    }
    return t;
}

}  // namespace tgs
