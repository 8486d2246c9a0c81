// tgs_mesh_aa_pair.hpp -- the whole decision of one antialias pair, shared by the forward (tgs_mesh_aa.hip) and the backward
// (tgs_mesh_grad.hip): which triangle, which exit edge, silhouette or not, which pixel receives.  It is written once so that the backward
// differentiates exactly the pairs the forward blended: every integer decision is the forward's, on the rasterizer's snapped coordinates.
// aa_pixel_pairs is the per-pixel prologue of both: the pairs a pixel has with its right and its upper neighbour.
#pragma once
#include "tgs_mesh_snap.hpp"

namespace tgs {

constexpr int TOPO_NONE = -1, TOPO_MANY = -2;

// the ID of a pixel: rast.w truncated; 0 (no triangle) for anything that is not a number of at most 2^24 in magnitude
__device__ __forceinline__ int aa_id(float w) { return fabsf(w) <= 16777216.0f ? (int)w : 0; }

struct AaVertex { int X, Y; bool ok; };
__device__ __forceinline__ AaVertex aa_vertex(const float4* __restrict__ pos, int i, int W, int H)
{
    AaVertex v = {0, 0, false};
    float sx, sy;
    v.ok = mesh_snap(pos[i], W, H, sx, sy, v.X, v.Y);
    return v;
}

// What a pair decided.  rec: +|a| the second pixel receives |a| (color[first] - color[second]), -|a| the first receives
// |a| (color[second] - color[first]), 0 nothing.  With rec != 0: va, vb the vertex indices of the exit edge a -> b (inside [0, V), both ok),
// (Px, Py) the centre of the pixel that shows the triangle and (ux, uy) the step to the other one, in snapped units, first: that pixel is the
// pair's first one.
struct AaPair { float rec; int va, vb, Px, Py, ux, uy; bool first; };
__device__ __forceinline__ AaPair aa_no_pair() { return {0.f, -1, -1, 0, 0, 0, 0, false}; }

// (i, j) is the pair's first pixel, (i + di, j + dj) its second, (di, dj) = (1, 0) or (0, 1); r1, r2 are (z/w, ID) of the two.
__device__ __forceinline__ AaPair aa_pair_full(int V, int F, const float4* __restrict__ pos, const int* __restrict__ tri, const int* __restrict__ topo,
                                               int W, int H, int i, int j, int di, int dj, float2 r1, float2 r2)
{
#pragma clang fp contract(off)
    AaPair res = aa_no_pair();
    // The antialias rule's own decode, NOT mesh_pixel_triangle: an ID that is not an integer or lies outside [1, F] is truncated (aa_id), not
    // rejected, as the header's antialias rule states -- for F + 0.5 antialias still sees triangle F where interpolate sees nothing.
    const int id1 = aa_id(r1.y), id2 = aa_id(r2.y);
    if (id1 == id2) return res;
    // T: the only one with an ID, else the smaller z/w, else (equal or unordered) the lower ID
    const bool first = (id1 != 0 && id2 != 0) ? (r1.x < r2.x || (!(r2.x < r1.x) && id1 < id2)) : id1 != 0;
    const int id = first ? id1 : id2;
    if (id < 1 || id > F) return res;
    const size_t T = (size_t)(id - 1);
    const int idx[3] = {tri[3 * T], tri[3 * T + 1], tri[3 * T + 2]};
    if ((unsigned)idx[0] >= (unsigned)V || (unsigned)idx[1] >= (unsigned)V || (unsigned)idx[2] >= (unsigned)V) return res;
    const AaVertex v[3] = {aa_vertex(pos, idx[0], W, H), aa_vertex(pos, idx[1], W, H), aa_vertex(pos, idx[2], W, H)};
    if (!v[0].ok || !v[1].ok || !v[2].ok) return res;
    // every factor below is a difference of two coordinates of magnitude <= 2^29 (or a pixel centre, < 2^22): it fits an int, and a product
    // is one 32 x 32 -> 64-bit multiply-add; the sign s is applied by negation.
    const long long A = (long long)(v[1].X - v[0].X) * (v[2].Y - v[0].Y) - (long long)(v[2].X - v[0].X) * (v[1].Y - v[0].Y);
    if (A == 0) return res;
    const bool ccw = A > 0;                                                       // s = +1
    // P shows T, Q is the other pixel; u = Q - P in snapped units
    const int pi = first ? i : i + di, pj = first ? j : j + dj;
    const int Px = 256 * pi + 128, Py = 256 * pj + 128;
    const int ux = (first ? 256 : -256) * di, uy = (first ? 256 : -256) * dj;
    int kexit = -1, dXe = 0, dYe = 0;
    long long Ee = 0, De = 0;
#pragma unroll
    for (int k = 2; k >= 0; k--) {                                                // descending: the FIRST qualifying k is what remains
        const AaVertex a = v[k], b = v[(k + 1) % 3];
        const int dX = b.X - a.X, dY = b.Y - a.Y;
        const long long Du = (long long)dX * uy - (long long)dY * ux, Eu = (long long)dX * (Py - a.Y) - (long long)dY * (Px - a.X);
        const long long D = ccw ? Du : -Du, E = ccw ? Eu : -Eu;
        const bool extent = dj == 0 ? (min(a.Y, b.Y) <= Py && Py <= max(a.Y, b.Y)) : (min(a.X, b.X) <= Px && Px <= max(a.X, b.X));
        if (D < 0 && E >= 0 && E <= -D && extent) { kexit = k; Ee = E; De = D; dXe = dX; dYe = dY; }
    }
    if (kexit < 0) return res;
    const int o = topo[3 * T + kexit];
    if (o >= 0) {                                                                 // one neighbour: a silhouette only if it folds to T's side
        if (o >= V) return res;
        const AaVertex vo = aa_vertex(pos, o, W, H);
        if (!vo.ok) return res;
        const AaVertex a = v[kexit];
        const long long Eo = (long long)dXe * (vo.Y - a.Y) - (long long)dYe * (vo.X - a.X);
        if ((ccw ? Eo : -Eo) < 0) return res;
    } else if (o != TOPO_NONE && o != TOPO_MANY) return res;
    const float t = (float)((double)Ee / (double)(-De));
    const float a = t - 0.5f;
    if (a == 0.f) return res;
    // a > 0: Q receives; a < 0: P receives.  The record is positive when the receiver is the pair's second pixel.
    const bool second_receives = (a > 0.f) == first;
    res.rec = second_receives ? fabsf(a) : -fabsf(a);
    res.va = kexit == 0 ? idx[0] : kexit == 1 ? idx[1] : idx[2];
    res.vb = kexit == 0 ? idx[1] : kexit == 1 ? idx[2] : idx[0];
    res.Px = Px; res.Py = Py; res.ux = ux; res.uy = uy; res.first = first;
    return res;
}

// The two pairs that pixel p = (i, j) of the W x H image is the first pixel of: pr[0] with its right neighbour, pr[1] with the one above it
// (pr holds aa_no_pair() on entry and keeps it at the image's edge).  One lane per pixel, in the forward's pair kernel and in the backward's.
__device__ __forceinline__ void aa_pixel_pairs(int V, int F, const float4* pos, const int* tri, const int* topo, int W, int H, const float4* rast, size_t p, AaPair pr[2])
{
    const int j = (int)(p / (size_t)W), i = (int)(p - (size_t)j * W);
    const auto zw_id = [](float4 r) { return make_float2(r.z, r.w); };
    const float2 me = zw_id(rast[p]);
    if (i + 1 < W) pr[0] = aa_pair_full(V, F, pos, tri, topo, W, H, i, j, 1, 0, me, zw_id(rast[p + 1]));
    if (j + 1 < H) pr[1] = aa_pair_full(V, F, pos, tri, topo, W, H, i, j, 0, 1, me, zw_id(rast[p + W]));
}

}  // namespace tgs
