// tgs_replay.hpp -- what the passes that walk a finished frame's tile lists with one lane per pixel have in common and can share as plain
// functions: k_render_bwd_det* (tgs_backward.hip), k_depth_fwd / k_depth_bwd (tgs_depth.hip), k_feat_fwd / k_feat_bwd (tgs_feature.hip).
//
// Geometry: 256 threads per tile, wave w owns the 8x8-pixel quadrant w (replay_lane).  Which pairs were blended is replayed, not stored: list
// positions 1 .. n_contrib[pixel] that pass the two cut-offs (power > 0, alpha < 1/255), with alpha from the instruction sequence of the render
// kernels (replay_pair_alpha; k_render_bwd_det spells the same sequence with literal constants) -- every pair falls on the side of 1/255 it
// fell on in the colour frame; a tile is walked up to its deepest contributor (tile_deepest).  From dL_dalpha the six geometry terms
// (geometry_terms); the passes that add into slab rows written by the colour backward do it with slab_row_add (hi + lo conic, in double).
// The staging round, the quadrant walk, the per-wave partial store and the wave-ordered sum of the flush stay written out in each kernel:
// moved into helpers (callables for the loop bodies) hipcc lays the loops out differently and the depth and feature passes lose 3-6 %.
#pragma once
#include "tgs_device.hpp"

namespace tgs {

constexpr int RCOMP = 9;               // wave_reduce36 sums RUNROLL entries x RCOMP components: v[u * RCOMP + k]

// ---- a lane's place in the tile of this workgroup (tile_desc[blockIdx.x]) ----
struct ReplayLane {
    uint32_t tile, start, n;           // the tile, the first position of its list and the list's length
    int wv, lane;                      // wave = 8x8-pixel quadrant, lane = pixel of the quadrant
    bool inside;                       // the pixel lies in the image
    float pixfx, pixfy;
    size_t pix_id;
};
__device__ __forceinline__ ReplayLane replay_lane(const ImgState& s, uint32_t gx, int W, int H)
{
    ReplayLane q;
    const uint4 td = s.tile_desc[blockIdx.x];
    q.tile = td.x;
    const uint32_t tx = q.tile % gx, ty = q.tile / gx;
    q.wv = threadIdx.x >> 6; q.lane = threadIdx.x & 63;
    const int px = tx * TILE + (q.wv & 1) * 8 + (q.lane & 7);
    const int py = ty * TILE + (q.wv >> 1) * 8 + (q.lane >> 3);
    q.inside = px < W && py < H;
    q.pixfx = (float)px; q.pixfy = (float)py;
    q.start = td.y; q.n = td.z - td.y;
    q.pix_id = (size_t)W * py + px;
    return q;
}

// ---- pair replay ----
// alpha of one (pixel, entry) pair from the UNSCALED record, rounded as the render kernels round it; G = exp(power)
__device__ __forceinline__ float replay_pair_alpha(const float4& a, const float4& bb, float dx, float dy, float& G, bool& cut)
{
#if TGS_FAST_MATH
    float4 sa = a, sb = bb;
    stage_conic_a(sa); stage_conic_b(sb);
    const float power = pair_power2(sa.z, sa.w, sb.x, dx, dy);
    G = __builtin_amdgcn_exp2f(power);
#else
    const float power = -0.5f * (a.z * dx * dx + bb.x * dy * dy) - a.w * dx * dy;
    G = tgs_exp(power);
#endif
    const float alpha = fminf(0.99f, bb.y * G);
    cut = (power > 0.0f) || (alpha < 1.0f / 255.0f);
    return alpha;
}

// the deepest list position any pixel of the tile blended (the maximum of n_contrib over the workgroup's 256 lanes)
__device__ __forceinline__ uint32_t tile_deepest(uint32_t last_contributor, uint32_t* wmax, int wv, int lane)
{
    const uint32_t mq = wave_max_u32(last_contributor);
    if (lane == 0) wmax[wv] = mq;
    __syncthreads();
    return max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
}

// ---- per-pair gradient terms ----
// from dL_dalpha of entry u: mean2D x / y, conic xx / xy / yy, opacity (backward.cu:537-555) into v[u * STRIDE + OFFSET + 0 .. 5]
template <int STRIDE, int OFFSET>
__device__ __forceinline__ void geometry_terms(float (&v)[RUNROLL * RCOMP], int u, const float4& a, const float4& bb, float dx, float dy, float G, float dL_dalpha,
                                               float ddelx_dx, float ddely_dy)
{
    const float dL_dG = bb.y * dL_dalpha;
    const float gdx = G * dx, gdy = G * dy;
    const float dG_ddelx = -gdx * a.z - gdy * a.w;
    const float dG_ddely = -gdy * bb.x - gdx * a.w;
    v[u * STRIDE + OFFSET + 0] = dL_dG * dG_ddelx * ddelx_dx;
    v[u * STRIDE + OFFSET + 1] = dL_dG * dG_ddely * ddely_dy;
    v[u * STRIDE + OFFSET + 2] = -0.5f * gdx * dx * dL_dG;
    v[u * STRIDE + OFFSET + 3] = -0.5f * gdx * dy * dL_dG;
    v[u * STRIDE + OFFSET + 4] = -0.5f * gdy * dy * dL_dG;
    v[u * STRIDE + OFFSET + 5] = G * dL_dalpha;
}

// ---- the flush of a pass that adds into slab rows ----
// slab row <- row + (mean2D x / y = r[0], r[1]; opacity = r[5]; conic = rc): the row was written by k_render_bwd* in front of the caller on
// the same stream and has one writer, the tile's workgroup.  The conic shares lie in the row as hi + lo: add in double, split again.
template <int NR>
__device__ __forceinline__ void slab_row_add(float4* row, const float (&r)[NR], const double (&rc)[3])
{
    float4 r0 = row[0], r1 = row[1], r2 = row[2];
    const double c5 = ((double)r1.y + (double)r2.y) + rc[0], c6 = ((double)r1.z + (double)r2.z) + rc[1], c7 = ((double)r1.w + (double)r2.w) + rc[2];
    r0.w += r[0];
    r1.x += r[1];
    r1.y = (float)c5; r1.z = (float)c6; r1.w = (float)c7;
    r2.x += r[5];
    r2.y = (float)(c5 - (double)r1.y); r2.z = (float)(c6 - (double)r1.z); r2.w = (float)(c7 - (double)r1.w);
    row[0] = r0; row[1] = r1; row[2] = r2;
}

}  // namespace tgs
