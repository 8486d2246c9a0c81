// tgs_reg.hip -- the scaling regulariser of the trainers' step, fused and without a host read-back.
//
// Every iteration of the reference's refinement loops adds (Edit_core/tetgs_texture/refine.py:306-317, refine_3dgs.py:339-350)
//     radii = tetgs.radii                                                  (tetgs_model.py:299-310, tetgs_edit_3d.py:332-343: rebuilt from the mesh)
//     max_vals, min_vals = max / min of scaling over the three axes
//     thresh_idxs = (max_vals > radii * 1.0) & (max_vals / min_vals > 10.0)
//     if thresh_idxs.sum() > 0: loss = loss + max_vals[thresh_idxs].mean()
// -- a mesh walk, about a dozen framework kernels forward and as many backward, and a host synchronisation (the `if`) per step.  Here:
//   k_gaussian_radii      once per model: the circumradius of every Gaussian's face (utils/graphics_utils.py:109-116), one thread per Gaussian
//   k_scale_reg_fwd       one thread per Gaussian: the row's decision and argmax (reg_row, the ONLY place they are made), one code byte per row,
//                         one {double sum, u32 count} partial per workgroup
//   k_scale_reg_reduce    one workgroup, fixed order, double: value = sum / count (0 when count == 0), count, 1 / count (0 when count == 0)
//   k_scale_reg_bwd       reads the code byte (never decides again), writes or adds upstream * weight / count [* max] on the argmax component
// No float atomics: two calls give the same bits.  The raw form applies the activation (expf, as k_bind_fwd does) inside the kernels.
#include "tgs_device.hpp"
#include "../../include/tgs_raster.h"

namespace tgs {

// ---- radii ------------------------------------------------------------------------------------------------------------------------------
// a * b * c / (4 * sqrt(s (s - a) (s - b) (s - c))) in double, operation by operation as the reference's float64 evaluation (no contraction):
// a repeated vertex gives 0 / 0 = NaN, three collinear vertices x / 0 = inf (or NaN where the rounded product falls below zero) -- no clamp.
__device__ __forceinline__ double reg_dist(const double* p, const double* q)
{
#pragma clang fp contract(off)
    const double x = p[0] - q[0], y = p[1] - q[1], z = p[2] - q[2];
    return sqrt(x * x + y * y + z * z);
}
__device__ __forceinline__ double circumradius(const double A[3], const double B[3], const double C[3])
{
#pragma clang fp contract(off)
    const double a = reg_dist(B, C), b = reg_dist(A, C), c = reg_dist(A, B);
    const double s = (a + b + c) / 2;
    const double K = sqrt(s * (s - a) * (s - b) * (s - c));
    return (a * b * c) / (4 * K);
}

__global__ __launch_bounds__(256) void k_gaussian_radii(int V, int F, int P, const float* __restrict__ verts, const void* __restrict__ faces, int faces_i64,
                                                        const void* __restrict__ face_indices, int index_kind, float* __restrict__ radii, int* __restrict__ flag)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    long long f = -1;
    if (index_kind == TGS_INDEX_I32) f = static_cast<const int*>(face_indices)[i];
    else if (index_kind == TGS_INDEX_I64) f = static_cast<const long long*>(face_indices)[i];
    else {
        const float x = static_cast<const float*>(face_indices)[i];                       // Edit3DTetGS keeps float indices; .int() truncates (tetgs_edit_3d.py:341)
        if (x > -1.0f && x < (float)F) f = (long long)x;                                   // (NaN, inf and anything outside [0, F) stay -1)
    }
    bool ok = f >= 0 && f < F;
    long long v[3] = {0, 0, 0};
    if (ok) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            v[k] = faces_i64 ? static_cast<const long long*>(faces)[3 * f + k] : (long long)static_cast<const int*>(faces)[3 * f + k];
            ok = ok && v[k] >= 0 && v[k] < V;
        }
    }
    if (!ok) {                                             // nothing is read through a bad index; the caller reads the flag back
        *flag = 1;
        radii[i] = __builtin_nanf("");
        return;
    }
    double p[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int c = 0; c < 3; c++) p[k][c] = (double)verts[3 * v[k] + c];
    }
    radii[i] = (float)circumradius(p[0], p[1], p[2]);
}

// ---- the regulariser --------------------------------------------------------------------------------------------------------------------
struct RegPartial {
    double sum;
    uint32_t count;
    uint32_t pad;
};
struct RegOut {              // what k_scale_reg_reduce leaves for the caller and for the backward: 12 bytes
    float value;
    uint32_t count;
    float inv_count;
};

// THE decision of a row, forward and (through the code byte) backward: 0 = not selected, 1..3 = index of the maximum + 1, the LOWEST index
// among equal maxima (what torch.max(dim=-1) returns on the CPU).  Strict > on fp32 values, a correctly rounded division, no contraction; a
// NaN anywhere in the row or in the radius selects nothing, an inf radius selects nothing, min == 0 gives inf > threshold: selected.
__device__ __forceinline__ int reg_row(float s0, float s1, float s2, float radius, float max_factor, float ratio_threshold, float& mx)
{
#pragma clang fp contract(off)
    int arg = 0;
    mx = s0;
    if (s1 > mx) { mx = s1; arg = 1; }
    if (s2 > mx) { mx = s2; arg = 2; }
    float mn = s0;
    if (s1 < mn) mn = s1;
    if (s2 < mn) mn = s2;
    if (s0 != s0 || s1 != s1 || s2 != s2) return 0;        // torch.max / torch.min propagate a NaN, and every comparison with it is false
    const float thresh = radius * max_factor;
    const float ratio = __fdiv_rn(mx, mn);
    return (mx > thresh && ratio > ratio_threshold) ? arg + 1 : 0;
}

// One DPP step of a compensated (hi, lo) sum: fetch the partner's pair the way wave_sum's ladder does, TwoSum the high parts, carry the error.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ void pair_step(float& hi, float& lo)
{
#pragma clang fp contract(off)
    const float oh = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, hi), CTRL, ROWMASK, 0xf, false));
    const float ol = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, lo), CTRL, ROWMASK, 0xf, false));
    const float s = hi + oh;
    const float bb = s - hi;
    const float err = (hi - (s - bb)) + (oh - bb);
    hi = s;
    lo = (lo + ol) + err;
}
// Sum of one fp32 value per lane over the wave as a compensated pair (wave_sum's six DPP steps; the total is lane 63's), returned as a double
// in every lane.  A non-finite total comes back non-finite.
__device__ __forceinline__ double wave_sum_pair(float v)
{
    float hi = v, lo = 0.f;
    pair_step<0xB1, 0xf>(hi, lo);     // quad_perm [1,0,3,2]
    pair_step<0x4E, 0xf>(hi, lo);     // quad_perm [2,3,0,1]
    pair_step<0x141, 0xf>(hi, lo);    // row_half_mirror
    pair_step<0x140, 0xf>(hi, lo);    // row_mirror
    pair_step<0x142, 0xa>(hi, lo);    // row_bcast15 -> rows 1,3
    pair_step<0x143, 0xc>(hi, lo);    // row_bcast31 -> rows 2,3
    const float h = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hi), 63));
    const float l = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, lo), 63));
    return (h - h == 0.f) ? (double)h + (double)l : (double)h;          // (inf + (inf - inf) would turn an infinite total into NaN)
}

template <bool RAW>
__global__ __launch_bounds__(256) void k_scale_reg_fwd(int P, const float* __restrict__ scales, const float* __restrict__ radii, float max_factor, float ratio_threshold,
                                                       uint8_t* __restrict__ codes, RegPartial* __restrict__ partial)
{
    __shared__ double wsum[4];
    __shared__ uint32_t wcnt[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    int code = 0;
    float mx = 0.f;
    if (i < P) {
        const size_t i3 = 3 * (size_t)i;
        float s0 = scales[i3], s1 = scales[i3 + 1], s2 = scales[i3 + 2];
        const float r = radii[i];
        if (RAW) { s0 = expf(s0); s1 = expf(s1); s2 = expf(s2); }                          // scale_activation = torch.exp (tetgs_model.py:16), as k_bind_fwd
        code = reg_row(s0, s1, s2, r, max_factor, ratio_threshold, mx);
        codes[i] = (uint8_t)code;
    }
    const double sum = wave_sum_pair(code ? mx : 0.f);
    const uint32_t cnt = wave_sum_u32(code ? 1u : 0u);
    if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6] = sum; wcnt[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        RegPartial p;
        p.sum = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        p.count = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        p.pad = 0;
        partial[blockIdx.x] = p;
    }
}

// one workgroup over the n partials, double, fixed order (as k_pixel_reduce)
__global__ __launch_bounds__(256) void k_scale_reg_reduce(int n, const RegPartial* __restrict__ partial, RegOut* __restrict__ out)
{
    __shared__ double r[4];
    __shared__ uint32_t c[4];
    double a = 0.0;
    uint32_t k = 0;
    for (int i = threadIdx.x; i < n; i += 256) { a += partial[i].sum; k += partial[i].count; }
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    k = wave_sum_u32(k);
    if ((threadIdx.x & 63) == 0) { r[threadIdx.x >> 6] = a; c[threadIdx.x >> 6] = k; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double sum = ((r[0] + r[1]) + r[2]) + r[3];
        const uint32_t count = c[0] + c[1] + c[2] + c[3];
        RegOut o;
        o.value = count ? (float)(sum / (double)count) : 0.f;               // no row selected: the reference adds nothing (refine.py:315)
        o.count = count;
        o.inv_count = count ? (float)(1.0 / (double)count) : 0.f;
        *out = o;
    }
}

template <bool RAW, bool ACCUMULATE>
__global__ __launch_bounds__(256) void k_scale_reg_bwd(int P, const uint8_t* __restrict__ codes, const RegOut* __restrict__ out, const float* __restrict__ raw_scales,
                                                       const float* __restrict__ upstream, float weight, float* __restrict__ grad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const size_t i3 = 3 * (size_t)i;
    const int code = codes[i];
    if (ACCUMULATE && code == 0) return;                                                   // adds nothing to this row
    float g = ((upstream ? upstream[0] : 1.0f) * weight) * out->inv_count;
    if (RAW && code) g *= expf(raw_scales[i3 + code - 1]);                                 // d exp = exp: the row's maximum, the forward's own value
    const float g0 = code == 1 ? g : 0.f, g1 = code == 2 ? g : 0.f, g2 = code == 3 ? g : 0.f;
    if (ACCUMULATE) {
        float a0 = grad[i3], a1 = grad[i3 + 1], a2 = grad[i3 + 2];
        a0 += g0; a1 += g1; a2 += g2;
        grad[i3] = a0; grad[i3 + 1] = a1; grad[i3 + 2] = a2;
    } else {
        grad[i3] = g0; grad[i3 + 1] = g1; grad[i3 + 2] = g2;
    }
}

static unsigned reg_blocks(int P) { return (unsigned)(((long long)P + 255) / 256); }

}  // namespace tgs

extern "C" {

size_t tgs_scale_reg_workspace_bytes(int P)
{
    return P > 0 ? (size_t)tgs::reg_blocks(P) * sizeof(tgs::RegPartial) : 0;
}

int tgs_gaussian_radii(void* stream, int V, int F, int P, const float* verts, const void* faces, int faces_i64, const void* face_indices, int index_kind,
                       float* radii, int* invalid_flag)
{
    using namespace tgs;
    if (V < 0 || F < 0 || P < 0) return set_error(TGS_ERR_INVALID, "tgs_gaussian_radii: bad sizes");
    if (index_kind != TGS_INDEX_I32 && index_kind != TGS_INDEX_I64 && index_kind != TGS_INDEX_F32)
        return set_error(TGS_ERR_INVALID, "tgs_gaussian_radii: index_kind must be TGS_INDEX_I32, TGS_INDEX_I64 or TGS_INDEX_F32");
    if (P == 0) return TGS_OK;
    if (V == 0 || F == 0) return set_error(TGS_ERR_INVALID, "tgs_gaussian_radii: Gaussians bound to a mesh without vertices or faces (every index is out of range)");
    if (!verts || !faces || !face_indices || !radii || !invalid_flag) return set_error(TGS_ERR_INVALID, "tgs_gaussian_radii: NULL required pointer");
    const hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(invalid_flag, 0, sizeof(int), st) != hipSuccess) return hip_status("tgs_gaussian_radii");
    hipLaunchKernelGGL(k_gaussian_radii, dim3(reg_blocks(P)), dim3(256), 0, st, V, F, P, verts, faces, faces_i64 ? 1 : 0, face_indices, index_kind, radii, invalid_flag);
    return hip_status("tgs_gaussian_radii");
}

int tgs_scale_reg_forward(void* stream, int P, const float* scales, int raw, const float* radii, float max_factor, float ratio_threshold, uint8_t* codes, void* out3,
                          void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    if (P < 0) return set_error(TGS_ERR_INVALID, "tgs_scale_reg_forward: P < 0");
    if (!out3 || (P > 0 && (!scales || !radii || !codes || !workspace))) return set_error(TGS_ERR_INVALID, "tgs_scale_reg_forward: NULL required pointer");
    if (workspace_bytes < tgs_scale_reg_workspace_bytes(P)) return set_error(TGS_ERR_INVALID, "tgs_scale_reg_forward: workspace smaller than tgs_scale_reg_workspace_bytes(P)");
    const hipStream_t st = (hipStream_t)stream;
    if (P == 0) {                                          // value 0, count 0, 1 / count 0 (all-zero bits); no launch
        if (hipMemsetAsync(out3, 0, sizeof(RegOut), st) != hipSuccess) return hip_status("tgs_scale_reg_forward");
        return TGS_OK;
    }
    const unsigned blocks = reg_blocks(P);
    RegPartial* partial = static_cast<RegPartial*>(workspace);
    if (raw) hipLaunchKernelGGL(k_scale_reg_fwd<true>, dim3(blocks), dim3(256), 0, st, P, scales, radii, max_factor, ratio_threshold, codes, partial);
    else hipLaunchKernelGGL(k_scale_reg_fwd<false>, dim3(blocks), dim3(256), 0, st, P, scales, radii, max_factor, ratio_threshold, codes, partial);
    hipLaunchKernelGGL(k_scale_reg_reduce, dim3(1), dim3(256), 0, st, (int)blocks, partial, static_cast<RegOut*>(out3));
    return hip_status("tgs_scale_reg_forward");
}

int tgs_scale_reg_backward(void* stream, int P, const uint8_t* codes, const void* out3, const float* raw_scales, const float* upstream, float weight, int accumulate,
                           float* grad)
{
    using namespace tgs;
    if (P < 0) return set_error(TGS_ERR_INVALID, "tgs_scale_reg_backward: P < 0");
    if (P == 0) return TGS_OK;
    if (!codes || !out3 || !grad) return set_error(TGS_ERR_INVALID, "tgs_scale_reg_backward: NULL required pointer");
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(reg_blocks(P));
    const RegOut* o = static_cast<const RegOut*>(out3);
#define TGS_REG_BWD(RAW, ACC) hipLaunchKernelGGL((k_scale_reg_bwd<RAW, ACC>), grid, dim3(256), 0, st, P, codes, o, raw_scales, upstream, weight, grad)
    if (raw_scales) { if (accumulate) TGS_REG_BWD(true, true); else TGS_REG_BWD(true, false); }
    else { if (accumulate) TGS_REG_BWD(false, true); else TGS_REG_BWD(false, false); }
#undef TGS_REG_BWD
    return hip_status("tgs_scale_reg_backward");
}
}
