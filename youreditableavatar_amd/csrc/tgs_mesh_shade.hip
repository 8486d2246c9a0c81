// tgs_mesh_shade.hip -- the body of the geometry stage's renderer between `interpolate` and `antialias`, for gfx950: the packed map
// (mask, normal, depth) of one image in one forward and one backward call (tetgs_spatial/models/renderers/part_nvdiff_rasterizer.py :112-148,
// models/geometry/implicit_sdf.py :291-317).  Plain HIP, wave64, integer atomics only, no float atomics anywhere, nothing read back.
//
// The rules (include/tgs_raster.h, "mesh shading", has them in full; tests/mesh_shade_ref.py restates them in torch):
//   forward   per covered pixel m = u a0 + v a1 + (1 - u - v) a2 of the vertex normals; world: n = m / max(|m|, 1e-12) stored as (n.y, n.z, n.x);
//             camera: m' = R^-1 m (adjugate over determinant, per image, in double), flipped to m'.z >= 0 on request, normalised; the stored
//             value is (n + 1) / 2 behind the mask's 1.  Depth: d = 1 / (z + 1e-7) of the interpolated clip z, stored as
//             (d - dmin) / (dmax - dmin + 1e-7) over the image's covered pixels.  An uncovered pixel stores zeros.
//   extremes  dmin and dmax come from a first pass: the order-preserving 64-bit image of the double (its complement for the minimum), a wave's
//             lanes reduced by shuffles, integer atomicMax per wave.  A maximum commutes: the result does not depend on the order of arrival.
//   backward  the chain above differentiated by hand, F.normalize's clamp and torch.max / torch.min's even share among ties included; the
//             sums over the image that the depth's normalisation needs (S1, S2 and the two tie counts) are per-workgroup partial sums in
//             double, added in ascending workgroup order (tgs_hashgrid.hip's k_hg_field_reduce).
// Everything smooth is evaluated in double from the fp32 inputs and rounded once on store: the kernels move tens of bytes per pixel, the
// arithmetic is free (tgs_mesh_grad.hip's choice).  The scatters into dL_dvn[V,3] and dL_dzattr[V] are tgs_grad_fixed.hpp's fixed point, the
// machinery of tgs_mesh_grad.hip: a measuring pass for the bound, llrint(c 2^(34 - e)), runs of equal triangle pre-reduced in the wave, one
// no-return 64-bit integer atomic per run and element, a converting pass.  Two runs give the same bits.
#include "tgs_mesh_snap.hpp"
#include "tgs_grad_fixed.hpp"

namespace tgs {

struct ShadeWork {
    uint32_t* bound;                      // [64] word 0: the bound of the dL_dvn scatter, word 1: of the dL_dzattr scatter
    unsigned long long* ext;              // [8]  word 0: the COMPLEMENT of dmin's key, word 1: dmax's key -- both grow, and both start from a cleared word
    double* sums;                         // [8]  S1, S2, the number of pixels at dmax, at dmin
    unsigned long long* acc;              // [4 V] fixed-point sums: [V,3] for dL_dvn, then [V] for dL_dzattr
    double* partial;                      // [4 G] the workgroups' S1, S2 and tie counts, G = ceil(n_pixels / 256)
};
__host__ __device__ inline size_t shade_carve(ShadeWork& w, char* base, size_t V, size_t N)
{
    char* p = base;
    carve(p, w.bound, 64); carve(p, w.ext, 8); carve(p, w.sums, 8); carve(p, w.acc, 4 * V); carve(p, w.partial, 4 * ((N + 255) / 256));
    return (size_t)(p - base) + 256;
}

// ---- the rules' pieces, each written once ------------------------------------------------------------------------------------------------
// the order-preserving image of a double: a < b  <=>  key(a) < key(b) (unsigned); -0 below +0; a NaN of positive sign above +inf
__device__ __forceinline__ unsigned long long shade_key(double d)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double shade_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? k & 0x7fffffffffffffffull : ~k));
}
__device__ __forceinline__ double shade_dmin(const unsigned long long* __restrict__ ext) { return shade_unkey(~ext[0]); }
__device__ __forceinline__ double shade_dmax(const unsigned long long* __restrict__ ext) { return shade_unkey(ext[1]); }

// d of a covered pixel.  No contraction: the extremes' pass and the passes that compare with them evaluate the same operations.
__device__ __forceinline__ double shade_depth(double u, double v, const float* __restrict__ zattr, const int idx[3])
{
#pragma clang fp contract(off)
    const double z = (u * (double)zattr[idx[0]] + v * (double)zattr[idx[1]]) + ((1.0 - u) - v) * (double)zattr[idx[2]];
    return 1.0 / (z + 1e-7);
}

// R^-1 of the image's rotation by adjugate over determinant; a determinant that is zero or not finite gives NaNs
__device__ __forceinline__ void shade_inverse(const float* __restrict__ rot, double inv[9])
{
    const double a = rot[0], b = rot[1], c = rot[2], d = rot[3], e = rot[4], f = rot[5], g = rot[6], h = rot[7], i = rot[8];
    const double A = e * i - f * h, B = f * g - d * i, C = d * h - e * g;
    const double det = a * A + b * B + c * C;
    const double s = (det != 0.0 && fabs(det) <= 1.7976931348623157e308) ? 1.0 / det : __longlong_as_double(0x7ff8000000000000ll);
    inv[0] = A * s; inv[1] = (c * h - b * i) * s; inv[2] = (b * f - c * e) * s;
    inv[3] = B * s; inv[4] = (a * i - c * g) * s; inv[5] = (c * d - a * f) * s;
    inv[6] = C * s; inv[7] = (b * g - a * h) * s; inv[8] = (a * e - b * d) * s;
}

struct ShadeNormal { double n[3]; double len; bool flipped; };
// the interpolated normal of a covered pixel through the mode's transform: n = m' / max(|m'|, 1e-12), len = |m'|
__device__ __forceinline__ ShadeNormal shade_normal(double u, double v, const float* __restrict__ vn, const int idx[3], bool camera, const double inv[9], bool flip)
{
    const double w2 = (1.0 - u) - v;
    double m[3];
#pragma unroll
    for (int c = 0; c < 3; c++) m[c] = (u * (double)vn[3 * (size_t)idx[0] + c] + v * (double)vn[3 * (size_t)idx[1] + c]) + w2 * (double)vn[3 * (size_t)idx[2] + c];
    ShadeNormal r;
    r.flipped = false;
    if (camera) {
        double t[3];
#pragma unroll
        for (int c = 0; c < 3; c++) t[c] = (inv[3 * c] * m[0] + inv[3 * c + 1] * m[1]) + inv[3 * c + 2] * m[2];
        r.flipped = flip && t[2] < 0.0;
#pragma unroll
        for (int c = 0; c < 3; c++) m[c] = r.flipped ? -t[c] : t[c];
    }
    r.len = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
    const double q = 1.0 / fmax(r.len, 1e-12);
#pragma unroll
    for (int c = 0; c < 3; c++) r.n[c] = m[c] * q;
    return r;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = (unsigned long long)__shfl_xor((long long)v, o, 64); v = t > v ? t : v; }
    return v;
}

// ---- the extremes of d ---------------------------------------------------------------------------------------------------------------
// One lane per pixel; two atomicMax per wave that holds a covered pixel (0 says "no covered pixel yet": no number's key or complemented key is 0, only a NaN of one payload's).
__global__ __launch_bounds__(256) void k_shade_extremes(int V, int F, const int* __restrict__ tri, const float* __restrict__ zattr, long long n_pixels,
                                                        const float4* __restrict__ rast, unsigned long long* __restrict__ ext)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long lo = 0ull, hi = 0ull;
    if (p < n_pixels) {
        const float4 r = rast[p];
        int idx[3];
        if (mesh_pixel_triangle(r.w, F, V, tri, idx) >= 0) { hi = shade_key(shade_depth((double)r.x, (double)r.y, zattr, idx)); lo = ~hi; }
    }
    lo = wave_max_u64(lo); hi = wave_max_u64(hi);
    if ((threadIdx.x & 63) == 0 && hi != 0ull) { atomicMax(ext, lo); atomicMax(ext + 1, hi); }
}

// ---- forward -------------------------------------------------------------------------------------------------------------------------
// One lane per pixel.  C = 4: one 16-byte store; C = 5: the depth behind it.
template <bool DEPTH>
__global__ __launch_bounds__(256) void k_shade_fwd(int V, int F, const int* __restrict__ tri, const float* __restrict__ vn, const float* __restrict__ zattr,
                                                   int camera, const float* __restrict__ rot, int flip, long long n_pixels, const float4* __restrict__ rast,
                                                   const unsigned long long* __restrict__ ext, float* __restrict__ out)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pixels) return;
    double inv[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (camera) shade_inverse(rot, inv);                                          // (uniform: nine scalar loads)
    const float4 r = rast[p];
    int idx[3];
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    float od = 0.f;
    if (mesh_pixel_triangle(r.w, F, V, tri, idx) >= 0) {
        const double u = (double)r.x, v = (double)r.y;
        const ShadeNormal s = shade_normal(u, v, vn, idx, camera != 0, inv, flip != 0);
        const int c0 = camera ? 0 : 1, c1 = camera ? 1 : 2, c2 = camera ? 2 : 0;
        o = make_float4(1.f, (float)((s.n[c0] + 1.0) * 0.5), (float)((s.n[c1] + 1.0) * 0.5), (float)((s.n[c2] + 1.0) * 0.5));
        if (DEPTH) {
            const double dmin = shade_dmin(ext), dmax = shade_dmax(ext);
            od = (float)((shade_depth(u, v, zattr, idx) - dmin) / ((dmax - dmin) + 1e-7));
        }
    }
    if (DEPTH) {
        float* q = out + 5 * p;
        q[0] = o.x; q[1] = o.y; q[2] = o.z; q[3] = o.w; q[4] = od;
    } else
        ((float4*)out)[p] = o;
}

// ---- backward ------------------------------------------------------------------------------------------------------------------------
// The sums of the depth's normalisation, per workgroup: S1 = sum g, S2 = sum g (d - dmin), the pixels at dmax, the pixels at dmin.  A wave adds
// its lanes in a fixed tree, the workgroup its four waves in ascending order.
__global__ __launch_bounds__(256) void k_shade_depth_partial(int V, int F, const int* __restrict__ tri, const float* __restrict__ zattr, long long n_pixels,
                                                             const float4* __restrict__ rast, const float* __restrict__ g, const unsigned long long* __restrict__ ext,
                                                             double* __restrict__ partial)
{
    __shared__ double part[4][4];
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (p < n_pixels) {
        const float4 r = rast[p];
        int idx[3];
        if (mesh_pixel_triangle(r.w, F, V, tri, idx) >= 0) {
            const double d = shade_depth((double)r.x, (double)r.y, zattr, idx), gd = (double)g[5 * p + 4];
            const unsigned long long k = shade_key(d);
            s[0] = gd; s[1] = gd * (d - shade_dmin(ext)); s[2] = k == ext[1] ? 1.0 : 0.0; s[3] = ~k == ext[0] ? 1.0 : 0.0;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[q] += __shfl_xor(s[q], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 4; q++) part[threadIdx.x >> 6][q] = s[q];
    }
    __syncthreads();
    if (threadIdx.x < 4) partial[4 * (size_t)blockIdx.x + threadIdx.x] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
}

// the workgroups' partial sums added in ascending workgroup order: lane q adds quantity q
__global__ __launch_bounds__(64) void k_shade_depth_reduce(long long n_groups, const double* __restrict__ partial, double* __restrict__ sums)
{
    if (threadIdx.x >= 4) return;
    double s = 0.0;
#pragma unroll 8
    for (long long b = 0; b < n_groups; b++) s += partial[4 * b + threadIdx.x];
    sums[threadIdx.x] = s;
}

// One lane per pixel.  MEASURE: the largest |contribution| to dL_dvn and to dL_dzattr go to bound[0] and bound[1]; else the contributions go
// to the accumulators, runs keyed by the triangle, and dL_drast is stored.  g_m is the gradient of the interpolated normal, g_z of the
// interpolated clip z; from there the rules are interpolate's backward.
template <bool MEASURE>
__global__ __launch_bounds__(256) void k_shade_bwd(int V, int F, int C, const int* __restrict__ tri, const float* __restrict__ vn, const float* __restrict__ zattr,
                                                   int camera, const float* __restrict__ rot, int flip, long long n_pixels, const float4* __restrict__ rast,
                                                   const float* __restrict__ g, const unsigned long long* __restrict__ ext, const double* __restrict__ sums,
                                                   int want_vn, int want_z, float4* __restrict__ drast, unsigned long long* __restrict__ acc, uint32_t* __restrict__ bound)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool depth = C == 5 && (want_z || drast);                               // (dL_dvn alone does not pass through the depth)
    int t = -1, idx[3] = {0, 0, 0};
    double u = 0.0, v = 0.0, gm[3] = {0.0, 0.0, 0.0}, gz = 0.0;
    if (p < n_pixels) {
        const float4 r = rast[p];
        t = mesh_pixel_triangle(r.w, F, V, tri, idx);
        if (t >= 0) {
            u = (double)r.x; v = (double)r.y;
            double inv[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
            if (camera) shade_inverse(rot, inv);
            const ShadeNormal s = shade_normal(u, v, vn, idx, camera != 0, inv, flip != 0);
            // the stored channels back to g_n: (n + 1) / 2 halves it, world mode stored (n.y, n.z, n.x)
            const float* gp = g + (size_t)C * p;
            double gn[3];
            if (camera) { gn[0] = 0.5 * (double)gp[1]; gn[1] = 0.5 * (double)gp[2]; gn[2] = 0.5 * (double)gp[3]; }
            else        { gn[1] = 0.5 * (double)gp[1]; gn[2] = 0.5 * (double)gp[2]; gn[0] = 0.5 * (double)gp[3]; }
            double gt[3];
            if (s.len >= 1e-12) {
                const double dot = (s.n[0] * gn[0] + s.n[1] * gn[1]) + s.n[2] * gn[2];
#pragma unroll
                for (int c = 0; c < 3; c++) gt[c] = (gn[c] - s.n[c] * dot) / s.len;
            } else {
#pragma unroll
                for (int c = 0; c < 3; c++) gt[c] = gn[c] / 1e-12;
            }
            if (s.flipped) { gt[0] = -gt[0]; gt[1] = -gt[1]; gt[2] = -gt[2]; }
#pragma unroll
            for (int c = 0; c < 3; c++) gm[c] = camera ? (inv[c] * gt[0] + inv[3 + c] * gt[1]) + inv[6 + c] * gt[2] : gt[c];       // R^-T
            if (depth) {
                const double dmin = shade_dmin(ext), dmax = shade_dmax(ext), rr = (dmax - dmin) + 1e-7;
                const double d = shade_depth(u, v, zattr, idx);
                const unsigned long long k = shade_key(d);
                double gd = (double)gp[4] / rr;
                if (k == ext[1]) gd += -sums[1] / (rr * rr) / sums[2];
                if (~k == ext[0]) gd += (-sums[0] / rr + sums[1] / (rr * rr)) / sums[3];
                gz = -gd * d * d;
            }
        }
    }
    const double w[3] = {u, v, (1.0 - u) - v};
    if (MEASURE) {
        uint32_t mn = 0u, mz = 0u;
        if (t >= 0) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
#pragma unroll
                for (int c = 0; c < 3; c++) mn = max(mn, grad_abs_bits(w[k] * gm[c]));
                mz = max(mz, grad_abs_bits(w[k] * gz));
            }
        }
        if (want_vn) grad_bound_max(mn, lane, bound);
        if (want_z) grad_bound_max(mz, lane, bound + 1);
    } else {
        if (drast && p < n_pixels) {
            double du = 0.0, dv = 0.0;
            if (t >= 0) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const double a2 = (double)vn[3 * (size_t)idx[2] + c];
                    du += gm[c] * ((double)vn[3 * (size_t)idx[0] + c] - a2);
                    dv += gm[c] * ((double)vn[3 * (size_t)idx[1] + c] - a2);
                }
                if (depth) {
                    const double z2 = (double)zattr[idx[2]];
                    du += gz * ((double)zattr[idx[0]] - z2);
                    dv += gz * ((double)zattr[idx[1]] - z2);
                }
            }
            drast[p] = make_float4((float)du, (float)dv, 0.f, 0.f);
        }
        double scale_n = 0.0, scale_z = 0.0;
        const bool add_n = want_vn && grad_scale(bound[0], scale_n), add_z = want_z && grad_scale(bound[1], scale_z);      // (uniform)
        if (!add_n && !add_z) return;
        const WaveRuns runs = wave_runs((long long)t, lane);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (add_n) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const long long s = run_sum(t >= 0 ? grad_fixed(w[k] * gm[c], scale_n) : 0ll, lane, runs);
                    if (runs.head && t >= 0) grad_add(acc + 3 * (size_t)idx[k] + c, s);
                }
            }
            if (add_z) {
                const long long s = run_sum(t >= 0 ? grad_fixed(w[k] * gz, scale_z) : 0ll, lane, runs);
                if (runs.head && t >= 0) grad_add(acc + 3 * (size_t)V + (size_t)idx[k], s);
            }
        }
    }
}

// the extremes of d into w.ext, which the caller has cleared
inline void shade_extremes(hipStream_t st, const ShadeWork& w, int V, int F, const int32_t* tri, const float* zattr, long long n_pixels, const float* rast)
{
    hipLaunchKernelGGL(k_shade_extremes, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, st, V, F, tri, zattr, n_pixels, (const float4*)rast, w.ext);
}

}  // namespace tgs

extern "C" {
#include "../../include/tgs_raster.h"

size_t tgs_meshshade_workspace_bytes(int V, int C, int64_t n_pixels)
{
    tgs::ShadeWork w;
    if (V < 0 || (C != 4 && C != 5) || !tgs::mesh_pixels_ok(n_pixels)) return 0;
    return tgs::shade_carve(w, nullptr, (size_t)V, (size_t)n_pixels);
}

int tgs_meshshade(void* stream, int V, int F, const int32_t* tri, const float* vn, const float* zattr, int camera, const float* rot, int flip, int64_t n_pixels,
                   const float* rast, float* out, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (V < 0 || !mesh_faces_ok(F) || !mesh_pixels_ok(n_pixels) || (camera != 0 && camera != 1) || (flip != 0 && flip != 1) || !workspace ||
        (n_pixels > 0 && (!rast || !out)) || (camera && !rot) || (F > 0 && V > 0 && n_pixels > 0 && (!tri || !vn)))
        return set_error(TGS_ERR_INVALID, "tgs_meshshade: V >= 0, 0 <= F < 2^24, 0 <= n_pixels <= 8192^2, camera and flip 0 or 1, and non-NULL tri / vn / rot (camera "
                                          "mode) / rast / out / workspace required");
    const int C = zattr ? 5 : 4;
    ShadeWork w;
    if (shade_carve(w, (char*)workspace, (size_t)V, (size_t)n_pixels) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_meshshade: workspace smaller than tgs_meshshade_workspace_bytes(V, C, n_pixels)");
    if (n_pixels == 0) return TGS_OK;
    if (F == 0 || V == 0) {                                                       // nothing is covered
        if (hipMemsetAsync(out, 0, (size_t)n_pixels * C * sizeof(float), st) != hipSuccess) return hip_status("tgs_meshshade");
        return TGS_OK;
    }
    const dim3 blk(256), grid((unsigned)((n_pixels + 255) / 256));
    if (zattr) {
        if (hipMemsetAsync(w.ext, 0, 8 * sizeof(unsigned long long), st) != hipSuccess) return hip_status("tgs_meshshade");
        shade_extremes(st, w, V, F, tri, zattr, (long long)n_pixels, rast);
        hipLaunchKernelGGL(k_shade_fwd<true>, grid, blk, 0, st, V, F, tri, vn, zattr, camera, rot, flip, (long long)n_pixels, (const float4*)rast, w.ext, out);
    } else
        hipLaunchKernelGGL(k_shade_fwd<false>, grid, blk, 0, st, V, F, tri, vn, zattr, camera, rot, flip, (long long)n_pixels, (const float4*)rast, w.ext, out);
    return hip_status("tgs_meshshade");
}

int tgs_meshshade_backward(void* stream, int V, int F, const int32_t* tri, const float* vn, const float* zattr, int camera, const float* rot, int flip,
                            int64_t n_pixels, const float* rast, const float* dL_dout, float* dL_dvn, float* dL_dzattr, float* dL_drast, void* workspace,
                            size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (V < 0 || !mesh_faces_ok(F) || !mesh_pixels_ok(n_pixels) || (camera != 0 && camera != 1) || (flip != 0 && flip != 1) || !workspace ||
        (n_pixels > 0 && (!rast || !dL_dout)) || (camera && !rot) || (F > 0 && V > 0 && n_pixels > 0 && (!tri || !vn)) || (dL_dzattr && !zattr))
        return set_error(TGS_ERR_INVALID, "tgs_meshshade_backward: V >= 0, 0 <= F < 2^24, 0 <= n_pixels <= 8192^2, camera and flip 0 or 1, non-NULL tri / vn / rot "
                                          "(camera mode) / rast / dL_dout / workspace, and zattr with dL_dzattr required");
    const int C = zattr ? 5 : 4;
    ShadeWork w;
    if (shade_carve(w, (char*)workspace, (size_t)V, (size_t)n_pixels) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_meshshade_backward: workspace smaller than tgs_meshshade_workspace_bytes(V, C, n_pixels)");
    const bool empty = F == 0 || V == 0 || n_pixels == 0;
    if (empty) {
        if (dL_dvn && V && hipMemsetAsync(dL_dvn, 0, 3 * (size_t)V * sizeof(float), st) != hipSuccess) return hip_status("tgs_meshshade_backward");
        if (dL_dzattr && V && hipMemsetAsync(dL_dzattr, 0, (size_t)V * sizeof(float), st) != hipSuccess) return hip_status("tgs_meshshade_backward");
        if (dL_drast && n_pixels && hipMemsetAsync(dL_drast, 0, (size_t)n_pixels * 4 * sizeof(float), st) != hipSuccess) return hip_status("tgs_meshshade_backward");
        return TGS_OK;
    }
    if (!dL_dvn && !dL_dzattr && !dL_drast) return TGS_OK;
    const dim3 blk(256), grid((unsigned)((n_pixels + 255) / 256));
    const long long n = (long long)n_pixels;
    // one clear: the bounds, the extremes, the sums and the accumulators lie behind one another
    if (hipMemsetAsync(w.bound, 0, (size_t)((char*)(w.acc + 4 * (size_t)V) - (char*)w.bound), st) != hipSuccess) return hip_status("tgs_meshshade_backward");
    if (zattr && (dL_dzattr || dL_drast)) {                                       // (dL_dvn alone needs none of the depth's three passes)
        shade_extremes(st, w, V, F, tri, zattr, n, rast);
        hipLaunchKernelGGL(k_shade_depth_partial, grid, blk, 0, st, V, F, tri, zattr, n, (const float4*)rast, dL_dout, w.ext, w.partial);
        hipLaunchKernelGGL(k_shade_depth_reduce, dim3(1), dim3(64), 0, st, (long long)grid.x, w.partial, w.sums);
    }
    const int want_vn = dL_dvn != nullptr, want_z = dL_dzattr != nullptr;
    const auto pixels = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, blk, 0, st, V, F, C, tri, vn, zattr, camera, rot, flip, n, (const float4*)rast, dL_dout, w.ext, w.sums, want_vn, want_z,
                           (float4*)dL_drast, w.acc, w.bound);
    };
    if (want_vn || want_z) pixels(k_shade_bwd<true>);
    pixels(k_shade_bwd<false>);
    if (want_vn) hipLaunchKernelGGL(k_grad_convert, dim3((unsigned)((3 * (size_t)V + 255) / 256)), blk, 0, st, 3ll * V, w.acc, w.bound, dL_dvn);
    if (want_z) hipLaunchKernelGGL(k_grad_convert, dim3((unsigned)(((size_t)V + 255) / 256)), blk, 0, st, (long long)V, w.acc + 3 * (size_t)V, w.bound + 1, dL_dzattr);
    return hip_status("tgs_meshshade_backward");
}
}
