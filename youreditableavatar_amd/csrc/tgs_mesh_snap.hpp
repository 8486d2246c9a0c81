// tgs_mesh_snap.hpp -- the snapping of one clip-space vertex, shared by the mesh rasterizer (tgs_mesh.hip) and the antialias pass (tgs_mesh_aa.hip):
// both decide in integers on the SAME snapped coordinates, so the float sequence that produces them is written once.
#pragma once
#include "tgs_device.hpp"

namespace tgs {

constexpr int MESH_MAX_DIM = 8192;        // width / height: (8192 / 32)^2 = 2^16 regions, times < 2^24 triangles, fits the 40-bit item count
constexpr int MESH_MAX_FACES = (1 << 24) - 1;     // the triangle ID travels in a float
constexpr float MESH_SNAP_MAX = 536870912.0f;     // 2^29

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

}  // namespace tgs
