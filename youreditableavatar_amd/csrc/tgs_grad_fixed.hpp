// tgs_grad_fixed.hpp -- the fixed-point scatter of a gradient, shared by tgs_mesh_grad.hip, tgs_hashgrid.hip and tgs_mesh_shade.hip: one exponent per call from a
// device-side bound that is never read back, contributions as 64-bit integers, the lanes of a wave pre-reduced over runs of equal
// destination, one no-return integer atomic per run and element, one convert pass with one rounding.  No float atomics.  (The heads of the
// sources and include/tgs_raster.h have the reasons and the resolution.)
#pragma once
#include "tgs_device.hpp"

namespace tgs {

constexpr int GRAD_FRAC = 34;                          // fraction bits below the bound's exponent
constexpr uint32_t GRAD_NONFINITE = 0x7f800000u;       // bits of +inf: every NaN's |bits| lie above, so an integer max keeps "not finite"

// ---- fixed point -----------------------------------------------------------------------------------------------------------------------
// false: nothing is accumulated (the bound is 0: every contribution is; or it is not finite: k_grad_convert writes NaN)
__device__ __forceinline__ bool grad_scale(uint32_t bits, double& scale)
{
    if (bits == 0u || bits >= GRAD_NONFINITE) return false;
    int e;
    (void)frexpf(__uint_as_float(bits), &e);           // B = m 2^e, 0.5 <= m < 1
    scale = ldexp(1.0, GRAD_FRAC - e);
    return true;
}
__device__ __forceinline__ long long grad_fixed(double c, double scale) { return __double2ll_rn(c * scale); }
__device__ __forceinline__ uint32_t grad_abs_bits(double c) { return __float_as_uint(fabsf((float)c)); }

// the wave's largest bits -> one integer atomicMax.  Every lane of the wave calls it.
__device__ __forceinline__ void grad_bound_max(uint32_t bits, int lane, uint32_t* bound)
{
    const uint32_t m = wave_max_u32(bits);
    if (lane == 0 && m != 0u) atomicMax(bound, m);
}

// Runs of equal keys over the lanes of a wave: head = first lane of its run, end = one past its last lane, merged = some run is longer than
// one lane (wave-uniform).  Every lane of the wave calls it.
struct WaveRuns { bool head; int end; bool merged; };
__device__ __forceinline__ WaveRuns wave_runs_of_heads(bool head, int lane);
__device__ __forceinline__ WaveRuns wave_runs(long long key, int lane)
{
    const long long left = __shfl_up(key, 1, 64);
    return wave_runs_of_heads(lane == 0 || left != key, lane);
}
// the same from the heads themselves (a key wider than 64 bits: the caller compares).  Every lane of the wave calls it.
__device__ __forceinline__ WaveRuns wave_runs_of_heads(bool head, int lane)
{
    WaveRuns r;
    r.head = head;
    const unsigned long long heads = __builtin_amdgcn_ballot_w64(r.head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    r.end = above ? lane + __ffsll(above) : 64;
    r.merged = heads != ~0ull;
    return r;
}
// the sum of v over the lanes lane .. end - 1 of the lane's run: in a head, the run's total.  Every lane of the wave calls it.
__device__ __forceinline__ long long run_sum(long long v, int lane, const WaveRuns& r)
{
    if (!r.merged) return v;                                                      // (wave-uniform)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long t = __shfl_down(v, o, 64);
        if (lane + o < r.end) v += t;
    }
    return v;
}
__device__ __forceinline__ void grad_add(unsigned long long* dst, long long v)
{
    if (v != 0) atomicAdd(dst, (unsigned long long)v);                           // (result unused: a no-return atomic)
}

static __global__ __launch_bounds__(256) void k_grad_max_abs(long long n, const float* __restrict__ g, uint32_t* __restrict__ bound)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const uint32_t bits = e < n ? __float_as_uint(fabsf(g[e])) : 0u;
    grad_bound_max(bits, threadIdx.x & 63, bound);
}

// (an element nothing reached holds 0 and becomes +0: the z column of a pos gradient, a vertex no pixel shows)
static __global__ __launch_bounds__(256) void k_grad_convert(long long n, const unsigned long long* __restrict__ acc, const uint32_t* __restrict__ bound,
                                                      float* __restrict__ out)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const uint32_t bits = *bound;
    float res = 0.f;
    if (bits >= GRAD_NONFINITE) res = __uint_as_float(0x7fc00000u);
    else if (bits != 0u) {
        int ex;
        (void)frexpf(__uint_as_float(bits), &ex);
        res = (float)ldexp((double)(long long)acc[e], ex - GRAD_FRAC);
    }
    out[e] = res;
}

}  // namespace tgs
