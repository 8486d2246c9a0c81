// tgs_mesh_grad.hip -- the backward of the mesh rasterizer's three calls (rasterize, interpolate, antialias), for gfx950: what the geometry
// stage trains through (tetgs_spatial/utils/rasterize.py; models/renderers/part_nvdiff_rasterizer.py :101-198).  Plain HIP, wave64, integer
// atomics only, no float atomics anywhere.
//
// The rules (include/tgs_raster.h, "mesh rasterizer: gradients", has them in full; tests/mesh_grad_ref.py restates them in torch float64):
//   interpolate  vertex 0's row of dL_dattr receives u g, vertex 1's v g, vertex 2's (1 - u - v) g; dL_drast = (g . (a0 - a2), g . (a1 - a2), 0, 0);
//   rasterize    the derivative of the forward's u, v expressions (mesh_frag / mesh_uv of tgs_mesh.hip) with respect to x, y, w of the winning
//                triangle's vertices, recomputed from the pixel's ID and the unsnapped pos; clamp and max pass the gradient inside and at
//                their bounds;
//   antialias    dL_dcolor is a gather with the forward's pair records as weights; dL_dpos differentiates the blend weight through
//                t~ = E(P) / (-D) on the real-valued screen coordinates, with every integer decision the forward's (aa_pair_full).
// The smooth parts are evaluated in double from the fp32 inputs: the kernels move tens of bytes per pixel, the arithmetic is free, and what
// remains of the error is the fixed point's resolution and one rounding to fp32.
//
// The scatters into [V,C] and [V,4] rows -- fixed point with one exponent per call:
//   bound        a device-side B >= max |contribution|: an integer atomicMax on the float's bits (k_grad_max_abs over the upstream for
//                dL_dattr, whose weights lie in [0, 1]; a measuring pass of the same kernel for the two pos gradients), never read back;
//   accumulate   with 2^(e-1) <= B < 2^e every contribution c becomes llrint(c 2^(GRAD_FRAC - e)), |.| <= 2^34: 2^28 of them stay below 2^63.
//                The lanes of a wave are pre-reduced in integers over runs of equal destination (wave_runs / run_sum: the ballot of heads of
//                k_surface_votes, a segmented shuffle sum), then ONE no-return 64-bit integer atomic per run and element;
//   convert      k_grad_convert turns the accumulators into fp32, one rounding.
// Integer sums commute: the bits do not depend on the order in which pixels were processed, two runs give the same bits.  A bound that is not
// finite (a NaN or an infinity in a contribution) makes every element of that gradient NaN; a bound of 0 leaves exact zeros.
// Resolution: an element that n contributions reach is off by at most n 2^(e - GRAD_FRAC - 1) <= n B 2^-GRAD_FRAC before the last rounding.
#include "tgs_mesh_aa_pair.hpp"
#include "tgs_grad_fixed.hpp"

namespace tgs {

struct GradWork {
    uint32_t* bound;                      // [64] bits of the largest |contribution| (word 0)
    unsigned long long* acc;              // [V * max(C, 4)] fixed-point sums (two's complement)
    float* rec_h;                         // [n_pixels] antialias: the pair records, as the forward's
    float* rec_v;
};
__host__ __device__ inline size_t grad_carve(GradWork& w, char* base, size_t V, size_t C, size_t N)
{
    char* p = base;
    carve(p, w.bound, 64); carve(p, w.acc, V * (C > 4 ? C : 4)); carve(p, w.rec_h, N); carve(p, w.rec_v, N);
    return (size_t)(p - base) + 256;
}

// ---- interpolate ---------------------------------------------------------------------------------------------------------------------
// One lane per pixel.  dL_drast is stored per pixel; dL_dattr goes through the accumulators, runs keyed by the triangle.
template <bool ATTR, bool RAST>
__global__ __launch_bounds__(256) void k_interp_bwd(int V, int F, int C, const float* __restrict__ attr, const int* __restrict__ tri, long long n_pixels,
                                                    const float4* __restrict__ rast, const float* __restrict__ g, float4* __restrict__ drast,
                                                    unsigned long long* __restrict__ acc, const uint32_t* __restrict__ bound)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int t = -1, idx[3] = {0, 0, 0};
    double u = 0.0, v = 0.0;
    if (p < n_pixels) {
        const float4 r = rast[p];
        t = mesh_pixel_triangle(r.w, F, V, tri, idx);
        if (t >= 0) { u = (double)r.x; v = (double)r.y; }
    }
    double scale = 0.0;
    const bool add = ATTR && grad_scale(*bound, scale);                           // (uniform)
    WaveRuns runs = {true, 0, false};
    if (add) runs = wave_runs((long long)t, lane);
    const double w2 = 1.0 - u - v;
    double du = 0.0, dv = 0.0;
    for (int c = 0; c < C; c++) {
        const double gc = t >= 0 ? (double)g[p * C + c] : 0.0;
        if (RAST && t >= 0) {
            const double a2 = (double)attr[(size_t)idx[2] * C + c];
            du += gc * ((double)attr[(size_t)idx[0] * C + c] - a2);
            dv += gc * ((double)attr[(size_t)idx[1] * C + c] - a2);
        }
        if (add) {
            const long long s0 = run_sum(t >= 0 ? grad_fixed(u * gc, scale) : 0ll, lane, runs);
            const long long s1 = run_sum(t >= 0 ? grad_fixed(v * gc, scale) : 0ll, lane, runs);
            const long long s2 = run_sum(t >= 0 ? grad_fixed(w2 * gc, scale) : 0ll, lane, runs);
            if (runs.head && t >= 0) {
                grad_add(acc + (size_t)idx[0] * C + c, s0);
                grad_add(acc + (size_t)idx[1] * C + c, s1);
                grad_add(acc + (size_t)idx[2] * C + c, s2);
            }
        }
    }
    if (RAST && p < n_pixels) drast[p] = make_float4((float)du, (float)dv, 0.f, 0.f);
}

// ---- rasterize -----------------------------------------------------------------------------------------------------------------------
// The nine derivatives of L through (u, v) of pixel (i, j) with respect to (x, y, w) of the three vertices p[k]: d[3 k + 0 / 1 / 2].
__device__ __forceinline__ void rast_uv_grad(const float4 p[3], int W, int H, int i, int j, double gu, double gv, double d[9])
{
    double sx[3], sy[3], iw[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        iw[k] = 1.0 / (double)p[k].w;
        sx[k] = ((double)p[k].x * iw[k] * 0.5 + 0.5) * (double)W;
        sy[k] = ((double)p[k].y * iw[k] * 0.5 + 0.5) * (double)H;
    }
    const double e1x = sx[1] - sx[0], e1y = sy[1] - sy[0], e2x = sx[2] - sx[0], e2y = sy[2] - sy[0];
    const double inv = 1.0 / (e1x * e2y - e1y * e2x);
    const double px = ((double)i + 0.5) - sx[0], py = ((double)j + 0.5) - sy[0];
    const double n1 = px * e2y - py * e2x, n2 = e1x * py - e1y * px;
    const double b1 = n1 * inv, b2 = n2 * inv, b0 = (1.0 - b1) - b2;
    const double q0 = b0 * iw[0], q1 = b1 * iw[1], q2 = b2 * iw[2];
    const double dd = (q0 + q1) + q2;
    const double u0 = q0 / dd, v0 = q1 / dd;
    const double uc = fmin(fmax(u0, 0.0), 1.0), vc = fmin(fmax(v0, 0.0), 1.0);
    const double s = fmax(uc + vc, 1.0);
    // u = uc / s, v = vc / s; s = max(uc + vc, 1)
    double g_uc = gu / s, g_vc = gv / s;
    if (uc + vc >= 1.0) { const double g_s = -(gu * uc + gv * vc) / (s * s); g_uc += g_s; g_vc += g_s; }
    const double g_u0 = (u0 >= 0.0 && u0 <= 1.0) ? g_uc : 0.0, g_v0 = (v0 >= 0.0 && v0 <= 1.0) ? g_vc : 0.0;
    // u0 = q0 / dd, v0 = q1 / dd
    const double g_dd = -(g_u0 * u0 + g_v0 * v0) / dd;
    const double g_q0 = g_u0 / dd + g_dd, g_q1 = g_v0 / dd + g_dd, g_q2 = g_dd;
    const double g_iw[3] = {g_q0 * b0, g_q1 * b1, g_q2 * b2};
    const double g_b0 = g_q0 * iw[0];
    const double g_b1 = g_q1 * iw[1] - g_b0, g_b2 = g_q2 * iw[2] - g_b0;
    const double g_n1 = g_b1 * inv, g_n2 = g_b2 * inv;
    const double g_area = -(g_b1 * n1 + g_b2 * n2) * inv * inv;
    const double g_e1x = g_area * e2y + g_n2 * py, g_e1y = -g_area * e2x - g_n2 * px;
    const double g_e2x = -g_area * e1y - g_n1 * py, g_e2y = g_area * e1x + g_n1 * px;
    const double g_px = g_n1 * e2y - g_n2 * e1y, g_py = -g_n1 * e2x + g_n2 * e1x;
    const double g_sx[3] = {-g_e1x - g_e2x - g_px, g_e1x, g_e2x}, g_sy[3] = {-g_e1y - g_e2y - g_py, g_e1y, g_e2y};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double ax = g_sx[k] * 0.5 * (double)W * iw[k], ay = g_sy[k] * 0.5 * (double)H * iw[k];
        d[3 * k] = ax; d[3 * k + 1] = ay;
        d[3 * k + 2] = -(ax * (double)p[k].x + ay * (double)p[k].y) * iw[k] - g_iw[k] * iw[k] * iw[k];
    }
}

// One lane per pixel.  MEASURE: the largest |contribution| goes to the bound; else the contributions go to the accumulators [V,4]
// (columns x, y, w; the z column is never touched), runs keyed by the triangle.
template <bool MEASURE>
__global__ __launch_bounds__(256) void k_rast_bwd(int V, int F, const float4* __restrict__ pos, const int* __restrict__ tri, int W, int H,
                                                  const float4* __restrict__ rast, const float4* __restrict__ g, unsigned long long* __restrict__ acc,
                                                  uint32_t* __restrict__ bound)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int t = -1, idx[3] = {0, 0, 0};
    double d[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (p < (size_t)W * H) {
        const int tt = mesh_pixel_triangle(rast[p].w, F, V, tri, idx);
        if (tt >= 0) {
            const float4 q[3] = {pos[idx[0]], pos[idx[1]], pos[idx[2]]};
            float sx, sy;
            int X, Y;
            if (mesh_snap(q[0], W, H, sx, sy, X, Y) && mesh_snap(q[1], W, H, sx, sy, X, Y) && mesh_snap(q[2], W, H, sx, sy, X, Y)) {
                const int j = (int)(p / (size_t)W), i = (int)(p - (size_t)j * W);
                const float4 gp = g[p];
                t = tt;
                rast_uv_grad(q, W, H, i, j, (double)gp.x, (double)gp.y, d);
            }
        }
    }
    if (MEASURE) {
        uint32_t m = 0u;
#pragma unroll
        for (int k = 0; k < 9; k++) m = max(m, grad_abs_bits(d[k]));
        grad_bound_max(m, lane, bound);
    } else {
        double scale = 0.0;
        if (!grad_scale(*bound, scale)) return;                                   // (uniform)
        const WaveRuns runs = wave_runs((long long)t, lane);
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const long long s = run_sum(t >= 0 ? grad_fixed(d[3 * k + c], scale) : 0ll, lane, runs);
                if (runs.head && t >= 0) grad_add(acc + 4 * (size_t)idx[k] + (c == 2 ? 3 : c), s);
            }
    }
}

// ---- antialias -----------------------------------------------------------------------------------------------------------------------
// The six derivatives of one blended pair with respect to (x, y, w) of the exit edge's vertices a (d[0..2]) and b (d[3..5]).
// first_pix / second_pix: the pair's pixels; the receiver R is the second one for rec > 0.
__device__ __forceinline__ void aa_pair_grad(const AaPair& pr, const float4* __restrict__ pos, int C, int W, int H, size_t first_pix, size_t second_pix,
                                             const float* __restrict__ color, const float* __restrict__ g, double boost, double d[6])
{
    const size_t R = pr.rec > 0.f ? second_pix : first_pix, O = pr.rec > 0.f ? first_pix : second_pix;
    double gt = 0.0;
    for (int c = 0; c < C; c++) gt += (double)g[R * C + c] * ((double)color[O * C + c] - (double)color[R * C + c]);
    const bool a_positive = (pr.rec > 0.f) == pr.first;                           // a > 0: Q receives
    gt = (a_positive ? gt : -gt) * boost;
    const float4 pa = pos[pr.va], pb = pos[pr.vb];
    const double iwa = 1.0 / (double)pa.w, iwb = 1.0 / (double)pb.w;
    const double kx = 128.0 * (double)W, ky = 128.0 * (double)H;                  // X = (x/w 0.5 + 0.5) width 256
    const double Xa = (double)pa.x * iwa * kx + kx, Ya = (double)pa.y * iwa * ky + ky;
    const double Xb = (double)pb.x * iwb * kx + kx, Yb = (double)pb.y * iwb * ky + ky;
    const double dX = Xb - Xa, dY = Yb - Ya, rx = (double)pr.Px - Xa, ry = (double)pr.Py - Ya;
    const double E = dX * ry - dY * rx, D = dX * (double)pr.uy - dY * (double)pr.ux;      // (the orientation sign cancels in E / -D)
    const double gE = -gt / D, gD = gt * E / (D * D);
    const double g_dX = gE * ry + gD * (double)pr.uy, g_dY = -gE * rx - gD * (double)pr.ux;
    const double gXa = -g_dX + gE * dY, gYa = -g_dY - gE * dX, gXb = g_dX, gYb = g_dY;
    const double ax = gXa * kx * iwa, ay = gYa * ky * iwa, bx = gXb * kx * iwb, by = gYb * ky * iwb;
    d[0] = ax; d[1] = ay; d[2] = -(ax * (double)pa.x + ay * (double)pa.y) * iwa;
    d[3] = bx; d[4] = by; d[5] = -(bx * (double)pb.x + by * (double)pb.y) * iwb;
}

// One lane per pixel analyses the pair with its right and its upper neighbour, as k_aa_pairs does.
// MODE 0: the records only; 1: the records, and the largest |pos contribution| to the bound; 2: the pos contributions to the accumulators,
// runs keyed by the exit edge.
template <int MODE>
__global__ __launch_bounds__(256) void k_aa_bwd(int V, int F, int C, const float4* __restrict__ pos, const int* __restrict__ tri, const int* __restrict__ topo,
                                                int W, int H, const float4* __restrict__ rast, const float* __restrict__ color, const float* __restrict__ g,
                                                double boost, float* __restrict__ rec_h, float* __restrict__ rec_v, unsigned long long* __restrict__ acc,
                                                uint32_t* __restrict__ bound)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = p < (size_t)W * H;
    AaPair pr[2] = {aa_no_pair(), aa_no_pair()};
    double d[2][6] = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
    if (live) {
        aa_pixel_pairs(V, F, pos, tri, topo, W, H, rast, p, pr);
        if (MODE < 2) { rec_h[p] = pr[0].rec; rec_v[p] = pr[1].rec; }
        if (MODE > 0) {
            if (pr[0].rec != 0.f) aa_pair_grad(pr[0], pos, C, W, H, p, p + 1, color, g, boost, d[0]);
            if (pr[1].rec != 0.f) aa_pair_grad(pr[1], pos, C, W, H, p, p + W, color, g, boost, d[1]);
        }
    }
    if (MODE == 1) {
        uint32_t m = 0u;
#pragma unroll
        for (int k = 0; k < 6; k++) m = max(m, max(grad_abs_bits(d[0][k]), grad_abs_bits(d[1][k])));
        grad_bound_max(m, lane, bound);
    }
    if (MODE == 2) {
        double scale = 0.0;
        if (!grad_scale(*bound, scale)) return;                                   // (uniform)
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const bool on = pr[h].rec != 0.f;
            const WaveRuns runs = wave_runs(on ? (long long)(((unsigned long long)(uint32_t)pr[h].va << 32) | (uint32_t)pr[h].vb) : -1ll, lane);
#pragma unroll
            for (int k = 0; k < 6; k++) {
                const long long s = run_sum(on ? grad_fixed(d[h][k], scale) : 0ll, lane, runs);
                if (runs.head && on) grad_add(acc + 4 * (size_t)(k < 3 ? pr[h].va : pr[h].vb) + (k % 3 == 2 ? 3 : k % 3), s);
            }
        }
    }
}

// dL_dcolor = (((g + left) + right) + below) + above: per pair the receiver's own row loses |a| g[receiver], the other pixel's gains it
__global__ __launch_bounds__(256) void k_aa_bwd_color(int C, int W, int H, long long n_elems, const float* __restrict__ g, const float* __restrict__ rec_h,
                                                      const float* __restrict__ rec_v, float* __restrict__ dcolor)
{
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_elems) return;
    const long long p = e / C;
    const int j = (int)(p / W), i = (int)(p - (long long)j * W);
    const float self = g[e];
    float res = self;
    const long long row = (long long)W * C;
    // a pair with the pixel as its SECOND one (left, below): rec > 0 the pixel receives, rec < 0 the neighbour does
    if (i > 0)     { const float r = rec_h[p - 1]; if (r > 0.f) res += -r * self; else if (r < 0.f) res += -r * g[e - C]; }
    // a pair with the pixel as its FIRST one (right, above): rec < 0 the pixel receives, rec > 0 the neighbour does
    if (i + 1 < W) { const float r = rec_h[p];     if (r < 0.f) res += r * self;  else if (r > 0.f) res += r * g[e + C]; }
    if (j > 0)     { const float r = rec_v[p - W]; if (r > 0.f) res += -r * self; else if (r < 0.f) res += -r * g[e - row]; }
    if (j + 1 < H) { const float r = rec_v[p];     if (r < 0.f) res += r * self;  else if (r > 0.f) res += r * g[e + row]; }
    dcolor[e] = res;
}

// The scatter protocol of one gradient out[n] (the head of this file has the reasons): zero the bound and n accumulators, the caller's measuring
// launch (w.bound <- max |contribution|), its accumulating launch (w.acc), k_grad_convert into out.  false: a memset was refused (hip_status says why).
template <class Measure, class Accumulate>
inline bool grad_scatter(hipStream_t st, const GradWork& w, size_t n, float* out, Measure measure, Accumulate accumulate)
{
    if (hipMemsetAsync(w.bound, 0, 64 * sizeof(uint32_t), st) != hipSuccess || hipMemsetAsync(w.acc, 0, n * sizeof(unsigned long long), st) != hipSuccess) return false;
    measure(); accumulate();
    hipLaunchKernelGGL(k_grad_convert, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (long long)n, w.acc, w.bound, out);
    return true;
}

}  // namespace tgs

extern "C" {
#include "../../include/tgs_raster.h"

size_t tgs_mesh_grad_workspace_bytes(int V, int C, int64_t n_pixels)
{
    tgs::GradWork w;
    if (V < 0 || C < 1 || !tgs::mesh_pixels_ok(n_pixels)) return 0;
    return tgs::grad_carve(w, nullptr, (size_t)V, (size_t)C, (size_t)n_pixels);
}

int tgs_mesh_interpolate_backward(void* stream, int V, int F, int C, const float* attr, const int32_t* tri, int64_t n_pixels, const float* rast,
                                  const float* dL_dout, float* dL_dattr, float* dL_drast, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (V < 0 || !mesh_faces_ok(F) || C < 1 || !mesh_pixels_ok(n_pixels) || !workspace || (n_pixels > 0 && (!rast || !dL_dout)) ||
        (F > 0 && V > 0 && n_pixels > 0 && (!attr || !tri)))
        return set_error(TGS_ERR_INVALID, "tgs_mesh_interpolate_backward: V >= 0, 0 <= F < 2^24, C >= 1, 0 <= n_pixels <= 8192^2 and non-NULL attr / tri / rast / "
                                          "dL_dout / workspace required");
    if (n_pixels > MESH_MAX_ELEMS / C) return set_error(TGS_ERR_INVALID, "tgs_mesh_interpolate_backward: n_pixels * C too large for one launch");
    GradWork w;
    if (grad_carve(w, (char*)workspace, (size_t)V, (size_t)C, (size_t)n_pixels) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_mesh_interpolate_backward: workspace smaller than tgs_mesh_grad_workspace_bytes(V, C, n_pixels)");
    const size_t n_attr = (size_t)V * (size_t)C;
    const bool empty = F == 0 || V == 0 || n_pixels == 0;
    if (dL_dattr && n_attr && empty && hipMemsetAsync(dL_dattr, 0, n_attr * sizeof(float), st) != hipSuccess) return hip_status("tgs_mesh_interpolate_backward");
    if (dL_drast && n_pixels && empty && hipMemsetAsync(dL_drast, 0, (size_t)n_pixels * 4 * sizeof(float), st) != hipSuccess)
        return hip_status("tgs_mesh_interpolate_backward");
    if (empty || (!dL_dattr && !dL_drast)) return TGS_OK;
    const long long n_elems = (long long)n_pixels * C;
    const dim3 blk(256), pgrid((unsigned)((n_pixels + 255) / 256));
    const auto pixels = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, pgrid, blk, 0, st, V, F, C, attr, tri, (long long)n_pixels, (const float4*)rast, dL_dout, (float4*)dL_drast, w.acc, w.bound);
    };
    if (!dL_dattr) pixels(k_interp_bwd<false, true>);
    else if (!grad_scatter(st, w, n_attr, dL_dattr,                               // (the weights lie in [0, 1]: the upstream's largest |g| is the bound)
                           [&] { hipLaunchKernelGGL(k_grad_max_abs, dim3((unsigned)((n_elems + 255) / 256)), blk, 0, st, n_elems, dL_dout, w.bound); },
                           [&] { if (dL_drast) pixels(k_interp_bwd<true, true>); else pixels(k_interp_bwd<true, false>); }))
        return hip_status("tgs_mesh_interpolate_backward");
    return hip_status("tgs_mesh_interpolate_backward");
}

int tgs_mesh_rasterize_backward(void* stream, int V, int F, const float* pos, const int32_t* tri, int width, int height, const float* rast,
                                const float* dL_drast, float* dL_dpos, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (V < 0 || !mesh_faces_ok(F) || !mesh_dims_ok(width, height) || !rast || !dL_drast || !workspace || (V > 0 && !dL_dpos) || (F > 0 && V > 0 && (!pos || !tri)))
        return set_error(TGS_ERR_INVALID, "tgs_mesh_rasterize_backward: V >= 0, 0 <= F < 2^24, 1 <= width, height <= 8192 and non-NULL pos / tri / rast / dL_drast / "
                                          "dL_dpos / workspace required");
    GradWork w;
    const size_t N = (size_t)width * (size_t)height;
    if (grad_carve(w, (char*)workspace, (size_t)V, 4, N) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_mesh_rasterize_backward: workspace smaller than tgs_mesh_grad_workspace_bytes(V, 4, width * height)");
    if (V == 0) return TGS_OK;
    const size_t n_pos = 4 * (size_t)V;
    if (F == 0) {
        if (hipMemsetAsync(dL_dpos, 0, n_pos * sizeof(float), st) != hipSuccess) return hip_status("tgs_mesh_rasterize_backward");
        return TGS_OK;
    }
    const dim3 blk(256), pgrid((unsigned)((N + 255) / 256));
    const float4 *p4 = (const float4*)pos, *r4 = (const float4*)rast, *g4 = (const float4*)dL_drast;
    const auto pixels = [&](auto kernel) { hipLaunchKernelGGL(kernel, pgrid, blk, 0, st, V, F, p4, tri, width, height, r4, g4, w.acc, w.bound); };
    if (!grad_scatter(st, w, n_pos, dL_dpos, [&] { pixels(k_rast_bwd<true>); }, [&] { pixels(k_rast_bwd<false>); })) return hip_status("tgs_mesh_rasterize_backward");
    return hip_status("tgs_mesh_rasterize_backward");
}

int tgs_mesh_antialias_backward(void* stream, int V, int F, int C, const float* pos, const int32_t* tri, const int32_t* topo, int width, int height,
                                const float* rast, const float* color, const float* dL_dout, float* dL_dcolor, float* dL_dpos, float pos_gradient_boost,
                                void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (V < 0 || !mesh_faces_ok(F) || C < 1 || !mesh_dims_ok(width, height) || !rast || !color || !dL_dout || !workspace ||
        (F > 0 && V > 0 && (!pos || !tri || !topo)))
        return set_error(TGS_ERR_INVALID, "tgs_mesh_antialias_backward: V >= 0, 0 <= F < 2^24, C >= 1, 1 <= width, height <= 8192 and non-NULL pos / tri / topo / rast / "
                                          "color / dL_dout / workspace required");
    if (dL_dcolor && dL_dcolor == dL_dout)
        return set_error(TGS_ERR_INVALID, "tgs_mesh_antialias_backward: dL_dcolor may not alias dL_dout (every pixel reads its neighbours' upstream rows)");
    const size_t N = (size_t)width * (size_t)height;
    if ((long long)N > MESH_MAX_ELEMS / C) return set_error(TGS_ERR_INVALID, "tgs_mesh_antialias_backward: width * height * C too large for one launch");
    GradWork w;
    if (grad_carve(w, (char*)workspace, (size_t)V, (size_t)C, N) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_mesh_antialias_backward: workspace smaller than tgs_mesh_grad_workspace_bytes(V, C, width * height)");
    const long long n_elems = (long long)N * C;
    const size_t n_pos = 4 * (size_t)V;
    if (F == 0 || V == 0) {                                                       // the forward was a copy
        if (dL_dcolor && hipMemcpyAsync(dL_dcolor, dL_dout, (size_t)n_elems * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
            return hip_status("tgs_mesh_antialias_backward");
        if (dL_dpos && n_pos && hipMemsetAsync(dL_dpos, 0, n_pos * sizeof(float), st) != hipSuccess) return hip_status("tgs_mesh_antialias_backward");
        return TGS_OK;
    }
    if (!dL_dcolor && !dL_dpos) return TGS_OK;
    const dim3 blk(256);
    const auto pixels = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((N + 255) / 256)), blk, 0, st, V, F, C, (const float4*)pos, tri, topo, width, height, (const float4*)rast, color,
                           dL_dout, (double)pos_gradient_boost, w.rec_h, w.rec_v, w.acc, w.bound);
    };
    if (dL_dpos) {
        if (!grad_scatter(st, w, n_pos, dL_dpos, [&] { pixels(k_aa_bwd<1>); }, [&] { pixels(k_aa_bwd<2>); })) return hip_status("tgs_mesh_antialias_backward");
    } else
        pixels(k_aa_bwd<0>);                                                      // the records alone, for dL_dcolor
    if (dL_dcolor)
        hipLaunchKernelGGL(k_aa_bwd_color, dim3((unsigned)((n_elems + 255) / 256)), blk, 0, st, C, width, height, n_elems, dL_dout, w.rec_h, w.rec_v, dL_dcolor);
    return hip_status("tgs_mesh_antialias_backward");
}
}
