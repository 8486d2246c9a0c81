// tgs_mask_ops.hip -- the image morphology and the Gaussian blur of the painting stage, for gfx950: what prepare_mask_proj
// (tetgs_inpainter/mask_mesh_0822.py :153-207) and normal_based_inpaint (inpaint_utils.py :27-39) take from cv2.erode, cv2.dilate and
// cv2.GaussianBlur on the host, behind a PNG file and two copies.  Plain HIP, wave64.  include/tgs_raster.h ("mask morphology and blur") has the
// rules in full; tests/mask_ops_ref.py restates them.
//
//   tgs_maskops_morph    k_morph<T, MAX, false> (the row pass: the strided source -> the workspace) then k_morph<T, MAX, true> (the column pass:
//                        the workspace -> dst); each stages its tile and the halo of the rectangle in LDS, a position outside the image as the
//                        identity of the operation, and takes the exact min / max of the k values
//   tgs_maskops_blur     k_blur_rows (float -> double, the workspace) then k_blur_cols (double -> float, rounded once); the weights travel as
//                        kernel arguments; a fixed tap order
//
// An image is walked as H lines of W * C elements: a channel's neighbour in x is C elements away, so one kernel serves every C.  No atomics;
// an element is written by one lane: two runs give the same bits.
#include "tgs_device.hpp"
#include "../../include/tgs_raster.h"

#include <cstdio>

namespace tgs {

constexpr int MORPH_K_MAX = 64, MORPH_C_MAX = 4, BLUR_K_MAX = 31;
constexpr int MO_BLOCK = 256;
constexpr int MO_ROW_TW = 256;                                   // row pass: 256 elements of one line per workgroup
constexpr int MO_COL_TW = 64, MO_COL_TH = 16;                    // column pass: 64 elements x 16 lines, 4 lines per lane
constexpr int MO_ROW_LDS = MO_ROW_TW + (MORPH_K_MAX - 1) * MORPH_C_MAX;
constexpr int MO_COL_LDS = MO_COL_TW * (MO_COL_TH + MORPH_K_MAX - 1);

template <typename T, bool MAX> struct Identity;
template <> struct Identity<uint8_t, false> { static __device__ uint8_t value() { return 255; } };
template <> struct Identity<uint8_t, true> { static __device__ uint8_t value() { return 0; } };
template <> struct Identity<float, false> { static __device__ float value() { return __builtin_inff(); } };
template <> struct Identity<float, true> { static __device__ float value() { return -__builtin_inff(); } };

template <typename T, bool MAX> __device__ __forceinline__ T pick(T a, T b) { return MAX ? (b > a ? b : a) : (b < a ? b : a); }

// one pass of the rectangle: k values along x (VERT = false; sx, sc, sy: the source's strides in elements) or along y (VERT = true; the source
// is the contiguous workspace).  E = W * C elements per line; dst is contiguous.
template <typename T, bool MAX, bool VERT>
__global__ void __launch_bounds__(MO_BLOCK) k_morph(int H, int W, int C, const T* __restrict__ src, long long sy, long long sx, long long sc, int k, T* __restrict__ dst)
{
    __shared__ T tile[VERT ? MO_COL_LDS : MO_ROW_LDS];
    const int E = W * C, a = k / 2;
    const T none = Identity<T, MAX>::value();
    if (!VERT) {
        const int y = blockIdx.y, e0 = blockIdx.x * MO_ROW_TW;
        const int lo = e0 - a * C, n = MO_ROW_TW + (k - 1) * C;                                       // the staged stretch [lo, lo + n)
        for (int i = threadIdx.x; i < n; i += MO_BLOCK) {
            const int e = lo + i;
            T v = none;
            if (e >= 0 && e < E) { const int x = e / C, c = e - x * C; v = src[(long long)y * sy + (long long)x * sx + (long long)c * sc]; }
            tile[i] = v;
        }
        __syncthreads();
        const int e = e0 + threadIdx.x;
        if (e >= E) return;
        T r = none;
        for (int j = 0; j < k; j++) r = pick<T, MAX>(r, tile[threadIdx.x + j * C]);
        dst[(size_t)y * E + e] = r;
    } else {
        const int e0 = blockIdx.x * MO_COL_TW, y0 = blockIdx.y * MO_COL_TH;
        const int lo = y0 - a, n = MO_COL_TH + k - 1;                                                  // the staged lines [lo, lo + n)
        const int tx = threadIdx.x & (MO_COL_TW - 1), ty = threadIdx.x / MO_COL_TW;
        const int e = e0 + tx;
        for (int i = ty; i < n; i += MO_BLOCK / MO_COL_TW) {
            const int y = lo + i;
            tile[i * MO_COL_TW + tx] = (e < E && y >= 0 && y < H) ? src[(size_t)y * E + e] : none;
        }
        __syncthreads();
        if (e >= E) return;
        for (int q = ty; q < MO_COL_TH; q += MO_BLOCK / MO_COL_TW) {
            const int y = y0 + q;
            if (y >= H) break;
            T r = none;
            for (int j = 0; j < k; j++) r = pick<T, MAX>(r, tile[(q + j) * MO_COL_TW + tx]);
            dst[(size_t)y * E + e] = r;
        }
    }
}

struct BlurWeights { double w[BLUR_K_MAX]; };

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }           // -1 -> 1, n -> n - 2; n > k / 2

// the row pass: tmp[y][e] = sum over i = 0 .. k - 1, in that order, of w[i] * src(y, reflect(x + i - k / 2), c), in double
__global__ void __launch_bounds__(MO_BLOCK) k_blur_rows(int H, int W, int C, const float* __restrict__ src, long long sy, long long sx, long long sc, int k, BlurWeights wt,
                                                        double* __restrict__ tmp)
{
    const int E = W * C, y = blockIdx.y, e = blockIdx.x * MO_BLOCK + threadIdx.x;
    if (e >= E) return;
    const int x = e / C, c = e - x * C, r = k / 2;
    const float* line = src + (long long)y * sy + (long long)c * sc;
    double acc = 0.0;
    for (int i = 0; i < k; i++) acc += wt.w[i] * (double)line[(long long)reflect101(x + i - r, W) * sx];
    tmp[(size_t)y * E + e] = acc;
}
// the column pass: the same over the lines of tmp, rounded to float once
__global__ void __launch_bounds__(MO_BLOCK) k_blur_cols(int H, int E, const double* __restrict__ tmp, int k, BlurWeights wt, float* __restrict__ dst)
{
    const int y = blockIdx.y, e = blockIdx.x * MO_BLOCK + threadIdx.x;
    if (e >= E) return;
    const int r = k / 2;
    double acc = 0.0;
    for (int i = 0; i < k; i++) acc += wt.w[i] * tmp[(size_t)reflect101(y + i - r, H) * E + e];
    dst[(size_t)y * E + e] = (float)acc;
}

static int mo_refuse(const char* entry, const char* what)
{
    static thread_local char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", entry, what);
    return set_error(TGS_ERR_INVALID, msg);
}

static const char* mo_check_image(int H, int W, int C, const void* src, const void* dst, const void* workspace, size_t workspace_bytes, size_t need)
{
    if (H < 0 || W < 0) return "H >= 0 and W >= 0 are required";
    if (C < 1 || C > MORPH_C_MAX) return "1 <= C <= 4 is required";
    if ((long long)W * C > 0x7fffff00ll || H > 65535) return "the image is above the limit (W * C < 2^31 - 256, H <= 65535)";
    if ((size_t)H * W == 0) return nullptr;
    if (!src || !dst || !workspace) return "src, dst and workspace must be non-NULL";
    if (workspace_bytes < need) return "the workspace is smaller than tgs_maskops_workspace_bytes says";
    return nullptr;
}

template <typename T, bool MAX>
static void morph_launch(hipStream_t st, int H, int W, int C, const T* src, long long sy, long long sx, long long sc, int kh, int kw, T* dst, T* tmp)
{
    const int E = W * C;
    hipLaunchKernelGGL((k_morph<T, MAX, false>), dim3((E + MO_ROW_TW - 1) / MO_ROW_TW, H), dim3(MO_BLOCK), 0, st, H, W, C, src, sy, sx, sc, kw, tmp);
    hipLaunchKernelGGL((k_morph<T, MAX, true>), dim3((E + MO_COL_TW - 1) / MO_COL_TW, (H + MO_COL_TH - 1) / MO_COL_TH), dim3(MO_BLOCK), 0, st, H, W, C,
                       (const T*)tmp, 0ll, 0ll, 0ll, kh, dst);
}

}  // namespace tgs

extern "C" {

size_t tgs_maskops_workspace_bytes(int H, int W, int C, int elem_bytes)
{
    if (H < 0 || W < 0 || C < 1 || C > tgs::MORPH_C_MAX || (elem_bytes != 1 && elem_bytes != 4 && elem_bytes != 8)) return 0;
    return (size_t)H * W * C * elem_bytes + 256;
}

int tgs_maskops_morph(void* stream, int op, int dtype, int H, int W, int C, const void* src, int64_t stride_y, int64_t stride_x, int64_t stride_c, int kh, int kw,
                      void* dst, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    if (op != 0 && op != 1) return mo_refuse("tgs_maskops_morph", "op is 0 (erode) or 1 (dilate)");
    if (dtype != 0 && dtype != 1) return mo_refuse("tgs_maskops_morph", "dtype is 0 (uint8) or 1 (float32)");
    if (kh < 1 || kw < 1 || kh > MORPH_K_MAX || kw > MORPH_K_MAX) return mo_refuse("tgs_maskops_morph", "1 <= kh, kw <= 64 is required");
    if (const char* bad = mo_check_image(H, W, C, src, dst, workspace, workspace_bytes, tgs_maskops_workspace_bytes(H, W, C, dtype ? 4 : 1))) return mo_refuse("tgs_maskops_morph", bad);
    if ((size_t)H * W == 0) return TGS_OK;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 0) {
        if (op) morph_launch<uint8_t, true>(st, H, W, C, (const uint8_t*)src, stride_y, stride_x, stride_c, kh, kw, (uint8_t*)dst, (uint8_t*)workspace);
        else morph_launch<uint8_t, false>(st, H, W, C, (const uint8_t*)src, stride_y, stride_x, stride_c, kh, kw, (uint8_t*)dst, (uint8_t*)workspace);
    } else {
        if (op) morph_launch<float, true>(st, H, W, C, (const float*)src, stride_y, stride_x, stride_c, kh, kw, (float*)dst, (float*)workspace);
        else morph_launch<float, false>(st, H, W, C, (const float*)src, stride_y, stride_x, stride_c, kh, kw, (float*)dst, (float*)workspace);
    }
    return hip_status("tgs_maskops_morph");
}

int tgs_maskops_blur(void* stream, int H, int W, int C, const float* src, int64_t stride_y, int64_t stride_x, int64_t stride_c, int kw, int kh,
                     const double* weights_x, const double* weights_y, float* dst, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    if (kw < 1 || kh < 1 || kw > BLUR_K_MAX || kh > BLUR_K_MAX || !(kw & 1) || !(kh & 1)) return mo_refuse("tgs_maskops_blur", "kw and kh must be odd and at most 31");
    if (!weights_x || !weights_y) return mo_refuse("tgs_maskops_blur", "weights_x and weights_y must be non-NULL (host pointers)");
    if (const char* bad = mo_check_image(H, W, C, src, dst, workspace, workspace_bytes, tgs_maskops_workspace_bytes(H, W, C, 8))) return mo_refuse("tgs_maskops_blur", bad);
    if (H <= kh / 2 || W <= kw / 2) return mo_refuse("tgs_maskops_blur", "each dimension of the image must exceed k / 2 (the reflected border)");
    BlurWeights wx{}, wy{};
    for (int i = 0; i < kw; i++) wx.w[i] = weights_x[i];
    for (int i = 0; i < kh; i++) wy.w[i] = weights_y[i];
    hipStream_t st = (hipStream_t)stream;
    const int E = W * C;
    const dim3 grid((E + MO_BLOCK - 1) / MO_BLOCK, H), block(MO_BLOCK);
    hipLaunchKernelGGL(k_blur_rows, grid, block, 0, st, H, W, C, src, (long long)stride_y, (long long)stride_x, (long long)stride_c, kw, wx, (double*)workspace);
    hipLaunchKernelGGL(k_blur_cols, grid, block, 0, st, H, E, (const double*)workspace, kh, wy, dst);
    return hip_status("tgs_maskops_blur");
}

}  // extern "C"
