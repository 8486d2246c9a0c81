// tgs_optim.hip -- the last arrow of the trainers' step: optimizer.step() over every Gaussian parameter group, one launch.
//
// The reference builds torch.optim.Adam(l, lr=0.0, eps=1e-15) over up to six parameter groups (Edit_core/tetgs_scene/tetgs_optimizer.py:92,
// :167) and calls .step() once per iteration (:101-103, :176-178).  On a HIP device that is torch's foreach path: about seven multi-tensor
// element-wise kernels, each streaming every parameter-sized tensor again -- 18 element passes (72 bytes per parameter float).  k_adam_step
// does torch's non-capturable single-tensor Adam for ALL tensors of a step in one pass: 4 reads (p, m, v, grad) and 3 writes (p, m, v), 28
// bytes per parameter float.
//
//   g = grad * grad_scale
//   m = m + (g - m) * (1 - beta1)                      exp_avg.lerp_(grad, 1 - beta1)        (weight < 0.5: torch's lerp takes this form)
//   v = v * beta2 + g * g * (1 - beta2)                exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
//   p = p - step_size * (m / (sqrt(v) / bc2_sqrt + eps))
//
// with step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) computed by the caller in double from the tensor's own step count t
// (torch does the same in Python floats) and handed over as fp32.  Division and square root are the correctly rounded ones (hipcc's
// default); fp32 denormals are kept (g * g * (1 - beta2) is one for |g| < 3e-18).
//
// The tensor table travels BY VALUE in the kernel argument (AdamArgs, 2.9 KB of the 4 KB a kernel argument block holds): no host-to-device
// copy, no workspace, nothing written on the device but p, m and v.  A block owns one chunk of 4096 elements of one tensor and finds them from
// the prefix of block counts with scalar (wave-uniform) arithmetic on blockIdx.x.  TGS_ADAM_MAX_TENSORS = 48 tensors fit one launch; a step
// with more becomes ceil(count / 48) launches.
//
// Memory access, like tgs_bind.hip (its header says why): every load of a thread first -- 16 loads of 16 bytes when the four pointers are
// 16-byte aligned, else 64 of 4 bytes, coalesced either way --, then the arithmetic, then every store.  A last chunk whose length is not a
// multiple of 4 floats goes element by element as a whole.  No atomics; no LDS on the contiguous path (the dynamic LDS size of a launch without a level-major tensor is 0).
//
// Level-major gradients (multiview.FlatGradients(level_major=True)): p, m, v are row-major [P, M, 3], the gradient of element (p, k, c) is
// at grad[k * plane_stride + 3 p + c].  A block owns a run of G Gaussians (G = 4096 / (3 M) rounded down to a multiple of 64: 64 at M = 15
// and 16, 320 at M = 4): its p / m / v elements are ONE contiguous run of 3 M G floats, its gradients M contiguous runs of 3 G floats, loaded
// as 16-byte pieces into an LDS image [M][3 G + 4] and read back transposed (ds_read_b32: at 16 reads per thread against 112 bytes of HBM
// traffic per element the LDS is nowhere near a limit).  Both sides stay coalesced; there is no 12-byte gather.
#include "tgs_device.hpp"
#include "../../include/tgs_raster.h"

namespace tgs {

constexpr int ADAM_CHUNK = 4096;                 // elements of one block: 256 threads x 16
constexpr int ADAM_LDS_PAD = 4;                  // floats between the planes of the LDS image (keeps 16-byte alignment, staggers the banks)
constexpr int ADAM_MAX_PLANES = 64;              // level-major: M <= 64 (the SH parameters have 1, 15 or 16)
constexpr size_t ADAM_LDS_BYTES = (ADAM_CHUNK + ADAM_LDS_PAD * ADAM_MAX_PLANES) * sizeof(float);

struct AdamTensor {
    float *p, *m, *v;
    const float* g;
    unsigned n;                                  // elements
    unsigned plane;                              // level-major: floats between coefficient planes; 0: the gradient is laid out like p
    int M, G;                                    // level-major: coefficients per Gaussian, Gaussians per block
    float step_size, bc2_sqrt;
};

struct AdamArgs {
    AdamTensor t[TGS_ADAM_MAX_TENSORS];
    unsigned first_block[TGS_ADAM_MAX_TENSORS];  // prefix of block counts; unused entries hold 2^32-1 (above every block index)
    float w1, beta2, w2, eps, grad_scale;        // w1 = 1 - beta1, w2 = 1 - beta2, rounded once from double
};
static_assert(sizeof(AdamArgs) <= 4096, "the tensor table must fit one kernel argument block");

// One block's run of `len` elements.  VEC: 16-byte accesses (every pointer 16-byte aligned and every run a multiple of 4 floats): one pass of
// 4 accesses per thread and array; else 4-byte accesses in two passes of 8 (the unaligned slice, a tensor's last odd chunk: 64 values per
// array in flight at once would spill).  LM: level-major gradient.  Loads are never predicated: a slot past the end of the run reads the
// run's last piece again (a predicated load merges with a default value, and that merge is waited for before the next load is issued);
// only the stores and the LDS writes are guarded.
template <bool LM, bool VEC>
__device__ __forceinline__ void adam_block(const AdamArgs& a, const AdamTensor& t, unsigned chunk, size_t base, unsigned len, float* lds)
{
    constexpr int W = VEC ? 4 : 1, SLOTS = VEC ? 4 : 8, PASSES = 16 / (W * SLOTS), N = W * SLOTS;
    const unsigned tid = threadIdx.x;
    float* __restrict__ P = t.p + base;
    float* __restrict__ Mo = t.m + base;
    float* __restrict__ V = t.v + base;
    const float* __restrict__ Gc = t.g + base;                        // (contiguous gradient)
    const unsigned S = 3 * (unsigned)t.G + ADAM_LDS_PAD, row = 3 * (unsigned)t.M;       // LM: the LDS image is [M][S], a Gaussian has `row` floats
    // ---- LM: the block's pieces of the M gradient planes, loaded here, written to the LDS image below ----
    float stage[16];
    unsigned stage_at[16 / W];
    if (LM) {
        const unsigned run = len / (unsigned)t.M;                     // floats of one plane segment: 3 * Gaussians of this block
        const unsigned pieces = run / W;
        const float* gb = t.g + 3 * (size_t)chunk * (unsigned)t.G;    // the block's first Gaussian in plane 0
#pragma unroll
        for (int k = 0; k < 16 / W; k++) {
            const unsigned q0 = tid + 256 * k, q = min(q0, pieces * (unsigned)t.M - 1);
            const unsigned pl = q / pieces, r = W * (q - pl * pieces);
            const float* src = gb + (size_t)pl * t.plane + r;
            if (VEC) {
                const float4 x = *reinterpret_cast<const float4*>(src);
                stage[4 * k] = x.x; stage[4 * k + 1] = x.y; stage[4 * k + 2] = x.z; stage[4 * k + 3] = x.w;
            } else
                stage[k] = *src;
            stage_at[k] = q0 == q ? pl * S + r : 0xffffffffu;
        }
    }
    auto write_image = [&]() {
#pragma unroll
        for (int k = 0; k < 16 / W; k++)
            if (stage_at[k] != 0xffffffffu) {
                if (VEC) *reinterpret_cast<float4*>(lds + stage_at[k]) = make_float4(stage[4 * k], stage[4 * k + 1], stage[4 * k + 2], stage[4 * k + 3]);
                else lds[stage_at[k]] = stage[k];
            }
        __syncthreads();                                              // (LM is the same for every thread of the block)
    };
    if (LM && !VEC) write_image();
#pragma unroll 1
    for (int pass = 0; pass < PASSES; pass++) {
        float p[N], m[N], v[N], g[N];
        unsigned at[SLOTS];                                           // first element of the slot, clamped into the run
        bool live[SLOTS];
        // ---- every load ----
#pragma unroll
        for (int k = 0; k < SLOTS; k++) {
            const unsigned e = W * (tid + 256 * (k + SLOTS * pass));
            live[k] = e < len;
            at[k] = min(e, len - W);
            if (VEC) {
                const float4 p4 = *reinterpret_cast<const float4*>(P + at[k]), m4 = *reinterpret_cast<const float4*>(Mo + at[k]), v4 = *reinterpret_cast<const float4*>(V + at[k]);
                p[4 * k] = p4.x; p[4 * k + 1] = p4.y; p[4 * k + 2] = p4.z; p[4 * k + 3] = p4.w;
                m[4 * k] = m4.x; m[4 * k + 1] = m4.y; m[4 * k + 2] = m4.z; m[4 * k + 3] = m4.w;
                v[4 * k] = v4.x; v[4 * k + 1] = v4.y; v[4 * k + 2] = v4.z; v[4 * k + 3] = v4.w;
                if (!LM) {
                    const float4 g4 = *reinterpret_cast<const float4*>(Gc + at[k]);
                    g[4 * k] = g4.x; g[4 * k + 1] = g4.y; g[4 * k + 2] = g4.z; g[4 * k + 3] = g4.w;
                }
            } else {
                p[k] = P[at[k]]; m[k] = Mo[at[k]]; v[k] = V[at[k]];
                if (!LM) g[k] = Gc[at[k]];
            }
        }
        if (LM) {                                                     // written by plane, read by Gaussian
            if (VEC) write_image();                                   // (one pass: behind every load of the thread)
#pragma unroll
            for (int k = 0; k < N; k++) {
                const unsigned e = at[k / W] + k % W;                 // element (gl, pl, c) of the block's row-major run
                const unsigned gl = e / row, w = e - gl * row, pl = w / 3, c = w - 3 * pl;
                g[k] = lds[pl * S + 3 * gl + c];
            }
        }
        // ---- the arithmetic ----
#pragma unroll
        for (int k = 0; k < N; k++) {
            const float gs = g[k] * a.grad_scale;
            m[k] = m[k] + (gs - m[k]) * a.w1;
            v[k] = v[k] * a.beta2 + gs * gs * a.w2;
            p[k] = p[k] - t.step_size * (m[k] / (sqrtf(v[k]) / t.bc2_sqrt + a.eps));
        }
        // ---- every store ----
#pragma unroll
        for (int k = 0; k < SLOTS; k++) {
            if (!live[k]) continue;
            if (VEC) {
                *reinterpret_cast<float4*>(P + at[k]) = make_float4(p[4 * k], p[4 * k + 1], p[4 * k + 2], p[4 * k + 3]);
                *reinterpret_cast<float4*>(Mo + at[k]) = make_float4(m[4 * k], m[4 * k + 1], m[4 * k + 2], m[4 * k + 3]);
                *reinterpret_cast<float4*>(V + at[k]) = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
            } else {
                P[at[k]] = p[k]; Mo[at[k]] = m[k]; V[at[k]] = v[k];
            }
        }
    }
}

__global__ __launch_bounds__(256, 4) void k_adam_step(const AdamArgs a)
{
    extern __shared__ float4 lds4[];
    const unsigned b = blockIdx.x;
    int ti = 0;
#pragma unroll
    for (int i = 1; i < TGS_ADAM_MAX_TENSORS; i++) ti += b >= a.first_block[i] ? 1 : 0;       // scalar unit: b and the table are wave-uniform
    const AdamTensor& t = a.t[ti];
    const unsigned chunk = b - a.first_block[ti];
    const bool lm = t.plane != 0;
    // the block's run of p / m / v: `len` elements from `base`
    const unsigned per_block = lm ? (unsigned)(3 * t.M * t.G) : (unsigned)ADAM_CHUNK;
    const size_t base = (size_t)chunk * per_block;
    const unsigned len = (size_t)t.n - base < per_block ? (unsigned)((size_t)t.n - base) : per_block;
    const bool aligned = ((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.m) | reinterpret_cast<uintptr_t>(t.v) | reinterpret_cast<uintptr_t>(t.g)) & 15) == 0;
    // a run that is not a multiple of 4 floats -- the last chunk of a tensor, the last Gaussians of a level-major one -- goes by element as a whole
    if (!lm) {
        if (aligned && len % 4 == 0) adam_block<false, true>(a, t, chunk, base, len, nullptr);
        else adam_block<false, false>(a, t, chunk, base, len, nullptr);
    } else {
        float* lds = reinterpret_cast<float*>(lds4);
        if (aligned && (len / (unsigned)t.M) % 4 == 0) adam_block<true, true>(a, t, chunk, base, len, lds);
        else adam_block<true, false>(a, t, chunk, base, len, lds);
    }
}

}  // namespace tgs

extern "C" {

int tgs_adam_step(void* stream, const tgs_adam_tensor_t* tensors, int count, double beta1, double beta2, float eps, float grad_scale)
{
    using namespace tgs;
    if (count == 0) return TGS_OK;
    if (count < 0 || !tensors) return set_error(TGS_ERR_INVALID, "tgs_adam_step: bad arguments");
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.f))
        return set_error(TGS_ERR_INVALID, "tgs_adam_step: betas must lie in [0, 1) and eps must not be negative");
    for (int i = 0; i < count; i++) {
        const tgs_adam_tensor_t& s = tensors[i];
        if (s.numel < 0 || s.numel > 0x7fffffffLL) return set_error(TGS_ERR_INVALID, "tgs_adam_step: a tensor's numel must lie in [0, 2^31-1]");
        if (s.numel == 0) continue;
        if (!s.param || !s.grad || !s.exp_avg || !s.exp_avg_sq) return set_error(TGS_ERR_INVALID, "tgs_adam_step: NULL required pointer");
        if (((uintptr_t)s.param | (uintptr_t)s.grad | (uintptr_t)s.exp_avg | (uintptr_t)s.exp_avg_sq) & 3)
            return set_error(TGS_ERR_INVALID, "tgs_adam_step: pointers must be 4-byte aligned");
        if (s.grad_plane_stride != 0) {
            const int64_t rows = s.planes > 0 ? s.numel / (3 * (int64_t)s.planes) : 0;
            if (s.planes < 1 || s.planes > ADAM_MAX_PLANES || rows * 3 * s.planes != s.numel || s.grad_plane_stride < 3 * rows || (s.grad_plane_stride & 3) ||
                s.grad_plane_stride > 0x7fffffffLL || ((uintptr_t)s.grad & 15))
                return set_error(TGS_ERR_INVALID, "tgs_adam_step: a level-major gradient needs numel = 3 * planes * rows with 1 <= planes <= 64, a plane stride >= "
                                                  "3 * rows that is a multiple of 4 floats, and a 16-byte aligned grad");
        }
    }
    // one launch per TGS_ADAM_MAX_TENSORS tensors (empty ones take no slot)
    int i = 0;
    while (i < count) {
        AdamArgs a{};
        unsigned blocks = 0;
        bool lm = false;
        int k = 0;
        for (; i < count && k < TGS_ADAM_MAX_TENSORS; i++) {
            const tgs_adam_tensor_t& s = tensors[i];
            if (s.numel == 0) continue;
            AdamTensor& d = a.t[k];
            d.p = s.param; d.m = s.exp_avg; d.v = s.exp_avg_sq; d.g = s.grad;
            d.n = (unsigned)s.numel; d.plane = (unsigned)s.grad_plane_stride; d.step_size = s.step_size; d.bc2_sqrt = s.bc2_sqrt;
            unsigned nb;
            if (d.plane) {
                int G = ADAM_CHUNK / (3 * s.planes);
                G = G >= 64 ? G & ~63 : G & ~3;                       // a multiple of 4: the plane segments of every block start 16-byte aligned
                d.M = s.planes; d.G = G;
                const unsigned rows = d.n / (3u * (unsigned)s.planes);
                nb = (rows + (unsigned)G - 1) / (unsigned)G;
                lm = true;
            } else
                nb = (d.n + ADAM_CHUNK - 1) / ADAM_CHUNK;
            a.first_block[k] = blocks;
            blocks += nb;
            k++;
        }
        if (k == 0) break;
        for (int j = k; j < TGS_ADAM_MAX_TENSORS; j++) a.first_block[j] = 0xffffffffu;      // never reached by a block index
        a.w1 = (float)(1.0 - beta1); a.beta2 = (float)beta2; a.w2 = (float)(1.0 - beta2); a.eps = eps; a.grad_scale = grad_scale;
        hipLaunchKernelGGL(k_adam_step, dim3(blocks), dim3(256), lm ? ADAM_LDS_BYTES : 0, (hipStream_t)stream, a);
        const int r = hip_status("tgs_adam_step");
        if (r < 0) return r;
    }
    return TGS_OK;
}

int tgs_adam_max_tensors(void) { return TGS_ADAM_MAX_TENSORS; }
size_t tgs_sizeof_adam_tensor(void) { return sizeof(tgs_adam_tensor_t); }
}
