// tgs_hashgrid.hip -- the head of the geometry stage's chain, for gfx950: the multiresolution hash-grid encoding and the SDF field built on it
// (tetgs_spatial/models/geometry/implicit_sdf.py :26-41, forward_sdf / forward_field; models/networks.py :55-95, :151-188: a tcnn.Encoding hash grid
// followed by a bias-free VanillaMLP with one hidden layer), forward and backward.  Plain HIP, wave64, integer atomics only, no float atomics.
// include/tgs_raster.h ("hash-grid field") has the rules in full; tests/hashgrid_ref.py restates them in torch float64.
//
//   level table  computed once on the host and passed by value in the kernel argument (at most 16 records of 20 bytes): nothing is recomputed,
//                allocated or read back on the device.
//   cell         pos = x scale + 0.5 in double from the fp32 x and the fp32 scale (the product is exact), cell = floor(pos), frac = pos - cell;
//                the eight corners cell + {0,1}^3 as uint32; dense index cx + cy res + cz res^2, hashed index cx ^ cy 2654435761 ^ cz 805459861,
//                both in uint32 arithmetic, and then ALWAYS % size: no coordinate can address outside its level.
//   values       the eight 8-byte corner rows of a level are loaded before any is used; the trilinear sum is formed in double and rounded once.
//   k_hg_encode            one lane per (point, level), level-major over blockIdx.y: the workgroups of one level run together and share its
//                          slice of the table in L2 (a hashed level of the default config is 4 MiB).
//   k_hg_encode_bwd_x      one lane per point: the derivative of the trilinear weights, a gather, no scatter.
//   k_hg_encode_bwd_params one lane per (point, level): the fixed-point scatter of tgs_grad_fixed.hpp, bound = max |dL_denc|.
//   k_hg_field             one lane per point: the optional box map, the encoding in registers, h = relu(W1 enc), out = W2 h + bias as fp32 FMAs;
//                          W1 (zero-padded to [64,32]) and W2 are staged in LDS and read as broadcasts.  Nothing of size N x 32 or N x H is stored.
//   k_hg_field_bwd         recomputes enc and h per point.  dL_denc exists only in registers and goes through the same scatter, under the ANALYTIC
//                          bound max |g| max_j sum_k sum_o |W1[k,j]| |W2[o,k]| (k_hg_field_bound, rounded up).  dL_dW1 and dL_dW2: the workgroup's
//                          256 points meet in LDS, 8 hidden units at a time, every thread owns elements of the two matrices and adds the
//                          workgroup's points in a fixed order in double; a persistent grid of at most 1024 workgroups stores one partial slab
//                          each, and k_hg_field_reduce adds the slabs in ascending order and rounds once.
// Integer sums commute and every float sum has a fixed order: two runs give the same bits, forward and backward.
#include "tgs_grad_fixed.hpp"
#include "../../include/tgs_raster.h"

namespace tgs {

constexpr int HG_MAX_LEVELS = 16;
constexpr int HG_COLS = 2 * HG_MAX_LEVELS;              // columns of the padded W1
constexpr int HG_MAX_HIDDEN = 64;
constexpr int HG_MAX_OUT = 4;
constexpr long long HG_MAX_POINTS = 1ll << 25;          // 8 contributions per point and level: 2^28, the fixed point's headroom
constexpr int HG_BLOCK = 256;
constexpr int HG_MAX_SLABS = 1024;                      // workgroups of the fused backward: one partial slab each
constexpr int HG_KC = 8;                                // hidden units that meet in LDS at a time
constexpr int HG_ROW = HG_BLOCK + 1;                    // LDS row of one value per point, padded: rows j and j + 1 start one bank apart
constexpr int HG_SLAB = HG_MAX_HIDDEN * HG_COLS + HG_MAX_OUT * HG_MAX_HIDDEN;   // doubles per slab, the padded layout
constexpr float HG_MAX_COORD = 1024.f;                  // |x| above it (or not finite): a NaN row.  scale < 2^20 keeps |pos| < 2^31

struct HgTable { tgs_hashgrid_level_t lv[HG_MAX_LEVELS]; int n_levels; int active; };
struct HgBox { float mn[3], mx[3]; int on; };

struct HgWork {
    uint32_t* bound;                      // [64] bits of the bound (word 0)
    unsigned long long* acc;              // [n_params] fixed-point sums
    double* slabs;                        // [HG_MAX_SLABS * HG_SLAB] the fused backward's partial sums (hidden > 0)
};
__host__ __device__ inline size_t hg_carve(HgWork& w, char* base, size_t n_params, bool fused)
{
    char* p = base;
    carve(p, w.bound, 64); carve(p, w.acc, n_params); carve(p, w.slabs, fused ? (size_t)HG_MAX_SLABS * HG_SLAB : 0);
    return (size_t)(p - base) + 256;
}

// the point's coordinates (through the box map, every operation rounded to fp32 on its own) -> false: a NaN row
__device__ __forceinline__ bool hg_point(const float* __restrict__ x, long long p, const HgBox& box, float q[3])
{
#pragma clang fp contract(off)
    bool ok = true;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        float v = x[3 * p + d];
        if (box.on) v = (v - box.mn[d]) / (box.mx[d] - box.mn[d]);
        q[d] = v;
        ok = ok && fabsf(v) <= HG_MAX_COORD;                                      // (a NaN fails the comparison)
    }
    return ok;
}

struct HgCell { uint32_t c[3]; uint32_t idx[8]; double f[3]; };
__device__ __forceinline__ void hg_cell(const tgs_hashgrid_level_t& lv, const float q[3], HgCell& c)
{
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const double pos = (double)q[d] * (double)lv.scale + 0.5;
        const double fl = floor(pos);
        c.f[d] = pos - fl;
        c.c[d] = (uint32_t)(long long)fl;
    }
    const uint32_t res = lv.resolution, size = lv.size;
    const bool pow2 = (size & (size - 1u)) == 0u;                                  // (uniform)
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t cx = c.c[0] + (i & 1), cy = c.c[1] + ((i >> 1) & 1), cz = c.c[2] + (i >> 2);
        const uint32_t index = lv.dense ? cx + cy * res + cz * res * res : cx ^ (cy * 2654435761u) ^ (cz * 805459861u);
        c.idx[i] = pow2 ? index & (size - 1u) : index % size;
    }
}
__device__ __forceinline__ double hg_weight(const HgCell& c, int i)
{
    return ((i & 1) ? c.f[0] : 1.0 - c.f[0]) * ((i & 2) ? c.f[1] : 1.0 - c.f[1]) * ((i & 4) ? c.f[2] : 1.0 - c.f[2]);
}
__device__ __forceinline__ void hg_rows(const float2* __restrict__ params, const tgs_hashgrid_level_t& lv, const HgCell& c, float2 v[8])
{
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = params[(size_t)lv.offset + c.idx[i]];
}
__device__ __forceinline__ float2 hg_value(const float2* __restrict__ params, const tgs_hashgrid_level_t& lv, const float q[3])
{
    HgCell c;
    float2 v[8];
    hg_cell(lv, q, c);
    hg_rows(params, lv, c, v);
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const double w = hg_weight(c, i);
        a0 += w * (double)v[i].x; a1 += w * (double)v[i].y;
    }
    return make_float2((float)a0, (float)a1);
}

// One level's share of dL_dparams for the lane's point: d0, d1 arrive on the level's two columns.  Runs of lanes in one cell are added in
// integers first; the run's head issues the atomics.  Every lane of the wave calls it.
__device__ __forceinline__ void hg_scatter(const tgs_hashgrid_level_t& lv, const float q[3], bool on, double d0, double d1, double scale, int lane,
                                           unsigned long long* __restrict__ acc)
{
    HgCell c = {};
    if (on) hg_cell(lv, q, c);
    const int left_on = __shfl_up((int)on, 1, 64);
    uint32_t left[3];
#pragma unroll
    for (int d = 0; d < 3; d++) left[d] = __shfl_up(c.c[d], 1, 64);              // (every lane shuffles: no shuffle behind a lane's own condition)
    const bool same = on && left_on != 0 && left[0] == c.c[0] && left[1] == c.c[1] && left[2] == c.c[2];
    const WaveRuns runs = wave_runs_of_heads(lane == 0 || !same, lane);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const double w = hg_weight(c, i);
        const long long s0 = run_sum(on ? grad_fixed(w * d0, scale) : 0ll, lane, runs);
        const long long s1 = run_sum(on ? grad_fixed(w * d1, scale) : 0ll, lane, runs);
        if (runs.head && on) {
            unsigned long long* dst = acc + 2 * ((size_t)lv.offset + c.idx[i]);
            grad_add(dst, s0); grad_add(dst + 1, s1);
        }
    }
}

// ---- the encoding ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HG_BLOCK) void k_hg_encode(long long N, const float* __restrict__ x, const float2* __restrict__ params, HgTable t,
                                                        float2* __restrict__ enc)
{
    const long long p = (long long)blockIdx.x * HG_BLOCK + threadIdx.x;
    const int l = blockIdx.y;
    if (p >= N) return;
    const HgBox none = {};
    float q[3];
    float2 r = make_float2(0.f, 0.f);
    if (!hg_point(x, p, none, q)) r.x = r.y = __uint_as_float(0x7fc00000u);
    else if (l < t.active) r = hg_value(params, t.lv[l], q);
    enc[p * t.n_levels + l] = r;
}

__global__ __launch_bounds__(HG_BLOCK) void k_hg_encode_bwd_x(long long N, const float* __restrict__ x, const float2* __restrict__ params, HgTable t,
                                                              const float2* __restrict__ g, float* __restrict__ dx)
{
    const long long p = (long long)blockIdx.x * HG_BLOCK + threadIdx.x;
    if (p >= N) return;
    const HgBox none = {};
    float q[3];
    double d[3] = {0.0, 0.0, 0.0};
    if (!hg_point(x, p, none, q)) d[0] = d[1] = d[2] = (double)__uint_as_float(0x7fc00000u);
    else
        for (int l = 0; l < t.active; l++) {
            const tgs_hashgrid_level_t lv = t.lv[l];
            HgCell c;
            float2 v[8];
            hg_cell(lv, q, c);
            hg_rows(params, lv, c, v);
            const float2 gl = g[p * t.n_levels + l];
            double e[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const double s = (double)gl.x * (double)v[i].x + (double)gl.y * (double)v[i].y;
                const double wx = (i & 1) ? c.f[0] : 1.0 - c.f[0], wy = (i & 2) ? c.f[1] : 1.0 - c.f[1], wz = (i & 4) ? c.f[2] : 1.0 - c.f[2];
                e[0] += ((i & 1) ? s : -s) * wy * wz;
                e[1] += ((i & 2) ? s : -s) * wx * wz;
                e[2] += ((i & 4) ? s : -s) * wx * wy;
            }
#pragma unroll
            for (int k = 0; k < 3; k++) d[k] += (double)lv.scale * e[k];
        }
#pragma unroll
    for (int k = 0; k < 3; k++) dx[3 * p + k] = (float)d[k];
}

__global__ __launch_bounds__(HG_BLOCK) void k_hg_encode_bwd_params(long long N, const float* __restrict__ x, HgTable t, const float2* __restrict__ g,
                                                                   unsigned long long* __restrict__ acc, const uint32_t* __restrict__ bound)
{
    const long long p = (long long)blockIdx.x * HG_BLOCK + threadIdx.x;
    const int l = blockIdx.y, lane = threadIdx.x & 63;
    double scale = 0.0;
    if (!grad_scale(*bound, scale)) return;                                       // (uniform)
    const HgBox none = {};
    float q[3] = {0.f, 0.f, 0.f};
    const bool on = p < N && hg_point(x, p, none, q);
    const float2 gl = on ? g[p * t.n_levels + l] : make_float2(0.f, 0.f);
    hg_scatter(t.lv[l], q, on, (double)gl.x, (double)gl.y, scale, lane, acc);
}

// ---- the fused field -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void hg_stage_weights(const float* __restrict__ W1, const float* __restrict__ W2, int H, int C, int D, float* s_w1, float* s_w2)
{
    for (int i = threadIdx.x; i < HG_MAX_HIDDEN * HG_COLS; i += HG_BLOCK) {
        const int k = i / HG_COLS, j = i % HG_COLS;
        s_w1[i] = (k < H && j < C) ? W1[k * C + j] : 0.f;
    }
    for (int i = threadIdx.x; i < HG_MAX_OUT * HG_MAX_HIDDEN; i += HG_BLOCK) {
        const int o = i / HG_MAX_HIDDEN, k = i % HG_MAX_HIDDEN;
        s_w2[i] = (o < D && k < H) ? W2[o * H + k] : 0.f;
    }
}
__device__ __forceinline__ void hg_encode_point(const float2* __restrict__ params, const HgTable& t, const float q[3], bool on, float enc[HG_COLS])
{
#pragma unroll
    for (int l = 0; l < HG_MAX_LEVELS; l++) {
        float2 r = make_float2(0.f, 0.f);
        if (l < t.active && on) r = hg_value(params, t.lv[l], q);
        enc[2 * l] = r.x; enc[2 * l + 1] = r.y;
    }
}

__global__ __launch_bounds__(HG_BLOCK) void k_hg_field(long long N, const float* __restrict__ x, const float2* __restrict__ params, HgTable t, HgBox box,
                                                       const float* __restrict__ W1, const float* __restrict__ W2, int H, int D, float bias,
                                                       float* __restrict__ out)
{
    __shared__ float s_w1[HG_MAX_HIDDEN * HG_COLS];
    __shared__ float s_w2[HG_MAX_OUT * HG_MAX_HIDDEN];
    hg_stage_weights(W1, W2, H, 2 * t.n_levels, D, s_w1, s_w2);
    __syncthreads();
    const long long p = (long long)blockIdx.x * HG_BLOCK + threadIdx.x;
    if (p >= N) return;
    float q[3], enc[HG_COLS];
    const bool ok = hg_point(x, p, box, q);
    hg_encode_point(params, t, q, ok, enc);
    float o[HG_MAX_OUT] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < H; k++) {
        float z = 0.f;
#pragma unroll
        for (int j = 0; j < HG_COLS; j++) z = fmaf(s_w1[k * HG_COLS + j], enc[j], z);
        const float h = z <= 0.f ? 0.f : z;                                       // (a NaN passes, as torch.relu passes it)
#pragma unroll
        for (int c = 0; c < HG_MAX_OUT; c++) o[c] = fmaf(s_w2[c * HG_MAX_HIDDEN + k], h, o[c]);
    }
#pragma unroll
    for (int c = 0; c < HG_MAX_OUT; c++)
        if (c < D) out[p * D + c] = ok ? o[c] + bias : __uint_as_float(0x7fc00000u);
}

// bound[0] holds the bits of max |g| (k_grad_max_abs) -> the bits of B = max |g| max_j sum_k sum_o |W1[k,j]| |W2[o,k]|, rounded up.  One wave.
__global__ __launch_bounds__(64) void k_hg_field_bound(const float* __restrict__ W1, const float* __restrict__ W2, int H, int C, int D, uint32_t* __restrict__ bound)
{
    const int j = threadIdx.x;
    double s = 0.0;
    if (j < C)
        for (int k = 0; k < H; k++) {
            double w2 = 0.0;
            for (int o = 0; o < D; o++) w2 += fabs((double)W2[o * H + k]);
            s += fabs((double)W1[k * C + j]) * w2;
        }
    const uint32_t fbits = wave_max_u32(__float_as_uint(__double2float_ru(s)));
    if (j != 0) return;
    const uint32_t gbits = *bound;
    if (gbits == 0u) return;
    uint32_t b = 0x7fc00000u;
    if (gbits < GRAD_NONFINITE && fbits < GRAD_NONFINITE) b = __float_as_uint(__double2float_ru((double)__uint_as_float(gbits) * (double)__uint_as_float(fbits)));
    *bound = b;
}

__global__ __launch_bounds__(HG_BLOCK) void k_hg_field_bwd(long long N, const float* __restrict__ x, const float2* __restrict__ params, HgTable t, HgBox box,
                                                           const float* __restrict__ W1, const float* __restrict__ W2, int H, int D,
                                                           const float* __restrict__ g, unsigned long long* __restrict__ acc,
                                                           const uint32_t* __restrict__ bound, double* __restrict__ slabs)
{
    __shared__ float s_w1[HG_MAX_HIDDEN * HG_COLS];
    __shared__ float s_w2[HG_MAX_OUT * HG_MAX_HIDDEN];
    __shared__ float s_enc[HG_COLS * HG_ROW];
    __shared__ float s_dz[HG_KC * HG_ROW];
    __shared__ float s_h[HG_KC * HG_ROW];
    __shared__ float s_g[HG_MAX_OUT * HG_ROW];
    const int tid = threadIdx.x, lane = tid & 63;
    hg_stage_weights(W1, W2, H, 2 * t.n_levels, D, s_w1, s_w2);
    double scale = 0.0;
    const bool scatter = acc != nullptr && grad_scale(*bound, scale);             // (uniform)
    const int kl = tid / HG_COLS, jj = tid % HG_COLS;                             // the thread's element of dL_dW1 in every chunk: row 8 ch + kl, column jj
    const int o2 = tid / HG_KC, k2 = tid % HG_KC;                                 // tid < 32: its element of dL_dW2: row o2, column 8 ch + k2
    double a1[HG_MAX_HIDDEN / HG_KC], a2[HG_MAX_HIDDEN / HG_KC];
#pragma unroll
    for (int ch = 0; ch < HG_MAX_HIDDEN / HG_KC; ch++) a1[ch] = a2[ch] = 0.0;
    const long long n_tiles = (N + HG_BLOCK - 1) / HG_BLOCK;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {       // (uniform)
        const long long p = tile * HG_BLOCK + tid;
        float q[3] = {0.f, 0.f, 0.f}, enc[HG_COLS], denc[HG_COLS], gv[HG_MAX_OUT];
        const bool on = p < N && hg_point(x, p, box, q);
        hg_encode_point(params, t, q, on, enc);
#pragma unroll
        for (int c = 0; c < HG_MAX_OUT; c++) gv[c] = (on && c < D) ? g[p * D + c] : 0.f;
        __syncthreads();                                                          // the weights are staged; the last tile's readers are done
#pragma unroll
        for (int j = 0; j < HG_COLS; j++) { s_enc[j * HG_ROW + tid] = enc[j]; denc[j] = 0.f; }
#pragma unroll
        for (int c = 0; c < HG_MAX_OUT; c++) s_g[c * HG_ROW + tid] = gv[c];
#pragma unroll
        for (int ch = 0; ch < HG_MAX_HIDDEN / HG_KC; ch++) {
            if (ch * HG_KC >= H) break;                                           // (uniform)
            for (int kk = 0; kk < HG_KC; kk++) {
                const int k = ch * HG_KC + kk;
                float z = 0.f, up = 0.f;
#pragma unroll
                for (int j = 0; j < HG_COLS; j++) z = fmaf(s_w1[k * HG_COLS + j], enc[j], z);
#pragma unroll
                for (int c = 0; c < HG_MAX_OUT; c++) up = fmaf(s_w2[c * HG_MAX_HIDDEN + k], gv[c], up);
                const bool open = z > 0.f;
                const float dz = open ? up : 0.f;
                s_dz[kk * HG_ROW + tid] = dz;
                s_h[kk * HG_ROW + tid] = open ? z : 0.f;
#pragma unroll
                for (int j = 0; j < HG_COLS; j++) denc[j] = fmaf(s_w1[k * HG_COLS + j], dz, denc[j]);
            }
            __syncthreads();
            double s = a1[ch];
            for (int r = 0; r < HG_BLOCK; r++) s += (double)s_dz[kl * HG_ROW + r] * (double)s_enc[jj * HG_ROW + r];
            a1[ch] = s;
            if (tid < HG_MAX_OUT * HG_KC) {
                double u = a2[ch];
                for (int r = 0; r < HG_BLOCK; r++) u += (double)s_g[o2 * HG_ROW + r] * (double)s_h[k2 * HG_ROW + r];
                a2[ch] = u;
            }
            __syncthreads();
        }
        if (scatter) {
#pragma unroll
            for (int l = 0; l < HG_MAX_LEVELS; l++)
                if (l < t.active) hg_scatter(t.lv[l], q, on, (double)denc[2 * l], (double)denc[2 * l + 1], scale, lane, acc);
        }
    }
    double* slab = slabs + (size_t)blockIdx.x * HG_SLAB;
#pragma unroll
    for (int ch = 0; ch < HG_MAX_HIDDEN / HG_KC; ch++) {
        slab[(ch * HG_KC + kl) * HG_COLS + jj] = a1[ch];
        if (tid < HG_MAX_OUT * HG_KC) slab[HG_MAX_HIDDEN * HG_COLS + o2 * HG_MAX_HIDDEN + ch * HG_KC + k2] = a2[ch];
    }
}

// the slabs added in ascending order, one rounding: element e of dL_dW1[H,C] followed by dL_dW2[D,H]
__global__ __launch_bounds__(HG_BLOCK) void k_hg_field_reduce(int n_slabs, const double* __restrict__ slabs, int H, int C, int D, float* __restrict__ dW1,
                                                              float* __restrict__ dW2)
{
    const int e = blockIdx.x * HG_BLOCK + threadIdx.x;
    if (e >= H * C + D * H) return;
    const bool first = e < H * C;
    const int r = first ? e / C : (e - H * C) / H, c = first ? e % C : (e - H * C) % H;
    const int at = first ? r * HG_COLS + c : HG_MAX_HIDDEN * HG_COLS + r * HG_MAX_HIDDEN + c;
    double s = 0.0;
    for (int b = 0; b < n_slabs; b++) s += slabs[(size_t)b * HG_SLAB + at];
    if (first) { if (dW1) dW1[e] = (float)s; }
    else if (dW2) dW2[e - H * C] = (float)s;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
// the arguments every call shares -> NULL, the table and the number of entries; or what is wrong with them
static const char* hg_check(int64_t N, int n_input_dims, int n_levels, int n_features, int log2_hashmap_size, int active_levels,
                            const tgs_hashgrid_level_t* levels, HgTable& t, size_t& n_entries)
{
    if (n_input_dims != 3) return "3 input dimensions are served";
    if (n_features != 2) return "2 features per level are served";
    if (n_levels < 1 || n_levels > HG_MAX_LEVELS) return "1 <= n_levels <= 16 required";
    if (log2_hashmap_size < 3 || log2_hashmap_size > 24) return "3 <= log2_hashmap_size <= 24 required";
    if (N < 0 || N > HG_MAX_POINTS) return "0 <= N <= 2^25 points per call required (evaluate a larger set in chunks)";
    if (active_levels < 0 || active_levels > n_levels) return "0 <= active_levels <= n_levels required";
    if (!levels) return "non-NULL levels required";
    size_t offset = 0;
    for (int l = 0; l < n_levels; l++) {
        const tgs_hashgrid_level_t& lv = levels[l];
        const unsigned long long cube = (unsigned long long)lv.resolution * lv.resolution * lv.resolution;
        if (!(lv.scale >= 0.f && lv.scale < 1048576.f) || lv.resolution < 1u || lv.resolution > (1u << 20) || lv.size < 8u || lv.size % 8u != 0u ||
            lv.size > (1u << log2_hashmap_size) || lv.offset != offset || lv.dense > 1u || (lv.dense && cube > lv.size))
            return "a level record is inconsistent: 0 <= scale < 2^20, 1 <= resolution <= 2^20, 8 <= size <= 2^log2_hashmap_size a multiple of 8, offset the running "
                   "sum of the sizes, dense only where resolution^3 <= size";
        t.lv[l] = lv;
        offset += lv.size;
    }
    for (int l = n_levels; l < HG_MAX_LEVELS; l++) t.lv[l] = tgs_hashgrid_level_t{0.f, 1u, 8u, 0u, 0u};
    t.n_levels = n_levels; t.active = active_levels;
    n_entries = offset;
    return nullptr;
}
static int hg_fail(const char* fn, const char* why)
{
    char msg[512];
    snprintf(msg, sizeof(msg), "%s: %s", fn, why);
    return set_error(TGS_ERR_INVALID, msg);
}
static const char* hg_check_mlp(int hidden, int n_out)
{
    if (hidden != 16 && hidden != 32 && hidden != 64) return "hidden width 16, 32 or 64 required (one hidden layer, no layer biases)";
    if (n_out < 1 || n_out > HG_MAX_OUT) return "1 <= n_out <= 4 required";
    return nullptr;
}
static const char* hg_check_box(const float* bbox, HgBox& box)
{
    box = HgBox{};
    if (!bbox) return nullptr;
    for (int d = 0; d < 3; d++) {
        box.mn[d] = bbox[d]; box.mx[d] = bbox[3 + d];
        if (!(box.mx[d] > box.mn[d]) || !(fabsf(box.mn[d]) < 3.0e38f) || !(fabsf(box.mx[d]) < 3.0e38f)) return "bbox must hold finite min[3] < max[3]";
    }
    box.on = 1;
    return nullptr;
}
static inline dim3 hg_grid(int64_t N, int y = 1) { return dim3((unsigned)((N + HG_BLOCK - 1) / HG_BLOCK), (unsigned)y); }

}  // namespace tgs

extern "C" {

size_t tgs_hashgrid_workspace_bytes(int64_t n_params, int hidden, int n_out)
{
    tgs::HgWork w;
    if (n_params < 16 || n_params > 2ll * tgs::HG_MAX_LEVELS * (1ll << 24) || (hidden != 0 && (tgs::hg_check_mlp(hidden, n_out) != nullptr))) return 0;
    return tgs::hg_carve(w, nullptr, (size_t)n_params, hidden != 0);
}

int tgs_hashgrid_encode(void* stream, int64_t N, int n_input_dims, const float* x, const float* params, const tgs_hashgrid_level_t* levels, int n_levels,
                        int n_features, int log2_hashmap_size, int active_levels, float* enc)
{
    using namespace tgs;
    static const char* fn = "tgs_hashgrid_encode";
    HgTable t;
    size_t n_entries = 0;
    if (const char* why = hg_check(N, n_input_dims, n_levels, n_features, log2_hashmap_size, active_levels, levels, t, n_entries)) return hg_fail(fn, why);
    if (!params || (N > 0 && (!x || !enc))) return hg_fail(fn, "non-NULL x / params / enc required");
    if (N == 0) return TGS_OK;
    hipLaunchKernelGGL(k_hg_encode, hg_grid(N, n_levels), dim3(HG_BLOCK), 0, (hipStream_t)stream, (long long)N, x, (const float2*)params, t, (float2*)enc);
    return hip_status(fn);
}

int tgs_hashgrid_encode_backward(void* stream, int64_t N, int n_input_dims, const float* x, const float* params, const tgs_hashgrid_level_t* levels,
                                 int n_levels, int n_features, int log2_hashmap_size, int active_levels, const float* dL_denc, float* dL_dparams,
                                 float* dL_dx, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    static const char* fn = "tgs_hashgrid_encode_backward";
    hipStream_t st = (hipStream_t)stream;
    HgTable t;
    size_t n_entries = 0;
    if (const char* why = hg_check(N, n_input_dims, n_levels, n_features, log2_hashmap_size, active_levels, levels, t, n_entries)) return hg_fail(fn, why);
    if (!params || !workspace || (N > 0 && (!x || !dL_denc))) return hg_fail(fn, "non-NULL x / params / dL_denc / workspace required");
    HgWork w;
    const size_t n_params = 2 * n_entries;
    if (hg_carve(w, (char*)workspace, n_params, false) > workspace_bytes) return hg_fail(fn, "workspace smaller than tgs_hashgrid_workspace_bytes(n_params, 0, 0)");
    if (dL_dx && N > 0)
        hipLaunchKernelGGL(k_hg_encode_bwd_x, hg_grid(N), dim3(HG_BLOCK), 0, st, (long long)N, x, (const float2*)params, t, (const float2*)dL_denc, dL_dx);
    if (!dL_dparams) return hip_status(fn);
    if (N == 0 || active_levels == 0) {
        if (hipMemsetAsync(dL_dparams, 0, n_params * sizeof(float), st) != hipSuccess) return hip_status(fn);
        return hip_status(fn);
    }
    if (hipMemsetAsync(w.bound, 0, 64 * sizeof(uint32_t), st) != hipSuccess || hipMemsetAsync(w.acc, 0, n_params * sizeof(unsigned long long), st) != hipSuccess)
        return hip_status(fn);
    const long long n_up = (long long)N * 2 * n_levels;                           // (the weights lie in [0, 1]: the upstream's largest |g| is the bound)
    hipLaunchKernelGGL(k_grad_max_abs, dim3((unsigned)((n_up + 255) / 256)), dim3(256), 0, st, n_up, dL_denc, w.bound);
    hipLaunchKernelGGL(k_hg_encode_bwd_params, hg_grid(N, active_levels), dim3(HG_BLOCK), 0, st, (long long)N, x, t, (const float2*)dL_denc, w.acc, w.bound);
    hipLaunchKernelGGL(k_grad_convert, dim3((unsigned)((n_params + 255) / 256)), dim3(256), 0, st, (long long)n_params, w.acc, w.bound, dL_dparams);
    return hip_status(fn);
}

int tgs_hashgrid_field(void* stream, int64_t N, int n_input_dims, const float* x, const float* params, const tgs_hashgrid_level_t* levels, int n_levels,
                       int n_features, int log2_hashmap_size, int active_levels, const float* bbox, const float* W1, const float* W2, int hidden, int n_out,
                       float bias, float* out)
{
    using namespace tgs;
    static const char* fn = "tgs_hashgrid_field";
    HgTable t;
    HgBox box;
    size_t n_entries = 0;
    if (const char* why = hg_check(N, n_input_dims, n_levels, n_features, log2_hashmap_size, active_levels, levels, t, n_entries)) return hg_fail(fn, why);
    if (const char* why = hg_check_mlp(hidden, n_out)) return hg_fail(fn, why);
    if (const char* why = hg_check_box(bbox, box)) return hg_fail(fn, why);
    if (!params || !W1 || !W2 || (N > 0 && (!x || !out))) return hg_fail(fn, "non-NULL x / params / W1 / W2 / out required");
    if (N == 0) return TGS_OK;
    hipLaunchKernelGGL(k_hg_field, hg_grid(N), dim3(HG_BLOCK), 0, (hipStream_t)stream, (long long)N, x, (const float2*)params, t, box, W1, W2, hidden, n_out, bias, out);
    return hip_status(fn);
}

int tgs_hashgrid_field_backward(void* stream, int64_t N, int n_input_dims, const float* x, const float* params, const tgs_hashgrid_level_t* levels,
                                int n_levels, int n_features, int log2_hashmap_size, int active_levels, const float* bbox, const float* W1, const float* W2,
                                int hidden, int n_out, const float* dL_dout, float* dL_dparams, float* dL_dW1, float* dL_dW2, void* workspace,
                                size_t workspace_bytes)
{
    using namespace tgs;
    static const char* fn = "tgs_hashgrid_field_backward";
    hipStream_t st = (hipStream_t)stream;
    HgTable t;
    HgBox box;
    size_t n_entries = 0;
    if (const char* why = hg_check(N, n_input_dims, n_levels, n_features, log2_hashmap_size, active_levels, levels, t, n_entries)) return hg_fail(fn, why);
    if (const char* why = hg_check_mlp(hidden, n_out)) return hg_fail(fn, why);
    if (const char* why = hg_check_box(bbox, box)) return hg_fail(fn, why);
    if (!params || !W1 || !W2 || !workspace || (N > 0 && (!x || !dL_dout))) return hg_fail(fn, "non-NULL x / params / W1 / W2 / dL_dout / workspace required");
    HgWork w;
    const size_t n_params = 2 * n_entries;
    if (hg_carve(w, (char*)workspace, n_params, true) > workspace_bytes)
        return hg_fail(fn, "workspace smaller than tgs_hashgrid_workspace_bytes(n_params, hidden, n_out)");
    if (!dL_dparams && !dL_dW1 && !dL_dW2) return TGS_OK;
    const int C = 2 * n_levels;
    if (N == 0) {
        if ((dL_dparams && hipMemsetAsync(dL_dparams, 0, n_params * sizeof(float), st) != hipSuccess) ||
            (dL_dW1 && hipMemsetAsync(dL_dW1, 0, (size_t)hidden * C * sizeof(float), st) != hipSuccess) ||
            (dL_dW2 && hipMemsetAsync(dL_dW2, 0, (size_t)n_out * hidden * sizeof(float), st) != hipSuccess))
            return hip_status(fn);
        return hip_status(fn);
    }
    const bool scatter = dL_dparams && active_levels > 0;
    if (dL_dparams && !scatter && hipMemsetAsync(dL_dparams, 0, n_params * sizeof(float), st) != hipSuccess) return hip_status(fn);
    if (scatter) {
        if (hipMemsetAsync(w.bound, 0, 64 * sizeof(uint32_t), st) != hipSuccess || hipMemsetAsync(w.acc, 0, n_params * sizeof(unsigned long long), st) != hipSuccess)
            return hip_status(fn);
        const long long n_up = (long long)N * n_out;
        hipLaunchKernelGGL(k_grad_max_abs, dim3((unsigned)((n_up + 255) / 256)), dim3(256), 0, st, n_up, dL_dout, w.bound);
        hipLaunchKernelGGL(k_hg_field_bound, dim3(1), dim3(64), 0, st, W1, W2, hidden, C, n_out, w.bound);
    }
    const long long n_tiles = (N + HG_BLOCK - 1) / HG_BLOCK;
    const int n_slabs = (int)(n_tiles < HG_MAX_SLABS ? n_tiles : HG_MAX_SLABS);
    hipLaunchKernelGGL(k_hg_field_bwd, dim3((unsigned)n_slabs), dim3(HG_BLOCK), 0, st, (long long)N, x, (const float2*)params, t, box, W1, W2, hidden, n_out, dL_dout,
                       scatter ? w.acc : (unsigned long long*)nullptr, w.bound, w.slabs);
    if (dL_dW1 || dL_dW2)
        hipLaunchKernelGGL(k_hg_field_reduce, dim3((unsigned)((hidden * C + n_out * hidden + HG_BLOCK - 1) / HG_BLOCK)), dim3(HG_BLOCK), 0, st, n_slabs, w.slabs, hidden, C,
                           n_out, dL_dW1, dL_dW2);
    if (scatter) hipLaunchKernelGGL(k_grad_convert, dim3((unsigned)((n_params + 255) / 256)), dim3(256), 0, st, (long long)n_params, w.acc, w.bound, dL_dparams);
    return hip_status(fn);
}
}
